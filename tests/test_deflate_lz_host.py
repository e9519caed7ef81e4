"""The device LZ deflate's model and host side, no device needed: the Python model of tests/deflate_lz_cases.py inflates through zlib
on every case; the stream it chooses is never longer than the run-length model's and a tenth of it where the data repeats far;
the rule on cases written out by hand; radnet_deflate_build_codes_lz gives complete codes of at most 15 bits whose header parses
back to them; radnet_deflate_stream_bits equals the model's count for both rules; radnet_deflate_lz_piece_cap bounds the model's
pieces; the mutants of the model are each caught by a named case; what encode_device refuses beside deflate="device-lz"."""
import zlib

import numpy as np
import pytest

import deflate_cases as D
import deflate_lz_cases as Z
from faster_rcnn import RADNet as R
from faster_rcnn import evaluate, png, utils_io
from radnet_hip import lib as L

CHUNK, TILE = L.header_constant("RADNET_DEFLATE_CHUNK"), L.header_constant("RADNET_DEFLATE_TILE")
RULE = dict(group=L.header_constant("RADNET_DEFLATE_LZ_GROUP"), far_min=L.header_constant("RADNET_DEFLATE_LZ_FAR_MIN"),
            far_min2=L.header_constant("RADNET_DEFLATE_LZ_FAR_MIN2"), far_d=L.header_constant("RADNET_DEFLATE_LZ_FAR_D"))
STREAMS = Z.streams(CHUNK, TILE, RULE)
NAMES = sorted(STREAMS)
_TOKENS = {}


def toks(name):
    """The rule's tokens of a case, made once."""
    if name not in _TOKENS:
        data, near = STREAMS[name]
        _TOKENS[name] = Z.tokens(data, CHUNK, TILE, near, RULE)
    return _TOKENS[name]


def matches(all_toks):
    return [t[1:] for chunk in all_toks for t in chunk if t[0] == "match"]


def product_codes(name):
    hist_ll, hist_d = Z.histograms(toks(name))
    code_ll, code_d, header, nbits = png.huffman_codes_lz(hist_ll, hist_d)
    return hist_ll, hist_d, code_ll, code_d, header, nbits


def test_the_header_states_the_models_constants_and_the_case_table_holds_what_it_promises():
    assert RULE == Z.RULE and L.header_constant("RADNET_DEFLATE_DIST_SYMBOLS") == Z.DIST_SYMBOLS == len(Z.DISTANCE_TABLE)
    assert [len(STREAMS["mixed " + k][0]) for k in ("1", "2", "3", "4", "5", "tile-1", "tile", "tile+1", "chunk-1", "chunk", "chunk+1", "2chunk+3")] == \
        [1, 2, 3, 4, 5, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    assert max(len(d) for d, _ in STREAMS.values()) <= 3 * CHUNK and {near for _, near in STREAMS.values()} == {1, 3}
    assert len(STREAMS["panel"][0]) == 120600 and len(STREAMS["rgb panel"][0]) == 180200 and len(STREAMS["period 7"][0]) == 140000
    assert len(STREAMS["repeated row"][0]) == 120300 and set(STREAMS["all byte values"][0]) == set(range(256)) and set(STREAMS["zeros"][0]) == {0}
    for d in range(1, 32769):                          # the distance table written out by hand against RFC 1951's construction
        s, eb, ev = Z.distance_symbol(d)
        assert Z.DISTANCE_TABLE[s][0] + ev == d and 0 <= ev < (1 << eb) and eb == Z.DISTANCE_TABLE[s][1] == max(0, s // 2 - 1)
    assert Z.distance_symbol(1)[0] == 0 and Z.distance_symbol(4)[0] == 3 and Z.distance_symbol(5) == (4, 1, 0) and Z.distance_symbol(32768) == (29, 13, 8191)


def test_the_rule_on_cases_written_out_by_hand():
    m = lambda name: matches(toks(name))      # noqa: E731
    assert m("match ends on the tile end") == [(40, 300)]
    assert m("match cut by the tile end") == [(25, 300), (15, 300)]                       # the rest is found again from the next tile's start
    assert m("match of 258") == [(258, TILE + 250)] and m("match of 259") == [(258, TILE + 250)]
    assert m("overlap distance 3 length 258") == [(258, 3)]
    assert m("source in the own group only") == [] and m("source in the group before") == [(40, 100)]
    assert m("equal hashes, different bytes") == [(RULE["far_min"] + 2, 1200)]                              # the colliding key is a literal, the bytes behind it match
    assert m("source 32768 back") == [(60, 32768)] and m("source 32769 back") == []
    assert m("repeat across a chunk boundary") == [] and m("keys in the last bytes of a chunk") == []
    # FAR_MIN bytes one beyond FAR_D are refused, FAR_MIN2 bytes are not
    assert m("short far matches") == [(RULE["far_min"], 300), (RULE["far_min2"], 3 * TILE + 40)]
    assert m("tie between distance 1 and near") == [(258, 1), (258, 1), (83, 1)]
    assert m("noise near 1") == [] and m("noise near 3") == []
    # zeros: distance 1 alone; a source may lie in the tile before (not in the chunk before), so a chunk has one literal, the first byte
    zeros = toks("zeros")
    per_tile = [("match", 258, 1)] * (TILE // 258) + [("match", TILE % 258, 1)]
    assert zeros[0] == [("lit", 0)] + per_tile[:-1] + [("match", TILE % 258 - 1, 1)] + per_tile * (CHUNK // TILE - 1)
    assert zeros[1] == [("lit", 0)] + per_tile[:-1] + [("match", TILE % 258 - 1, 1), ("match", 5, 1)]
    # the period's source is the nearest one in an earlier group; the row's is the row above
    assert all(d % 7 == 0 and d < RULE["group"] + 7 for _, d in m("period 7")) and {d for _, d in m("repeated row")} == {1203}
    assert all(d in (1, 3) or d >= 4 for _, d in m("rgb panel")) and any(d == 3 for _, d in m("rgb panel")) and any(d > 256 for _, d in m("rgb panel"))
    # the smallest lengths: nothing to match below 4 bytes but a run
    for k in ("1", "2", "3"):
        assert m("mixed " + k) == []
    table = Z.token_table(toks("match cut by the tile end"), 3 * TILE)
    assert table[2 * TILE - 25] == (1 << 31) | (25 << 16) | 299 and table[2 * TILE - 24] == 0 and table[2 * TILE] == (1 << 31) | (15 << 16) | 299
    assert table[0] == 1 << 31 and table.dtype == np.uint32


@pytest.mark.parametrize("name", NAMES)
def test_the_model_inflates_and_the_chosen_stream_is_never_longer_than_run_length(name):
    data, near = STREAMS[name]
    stream = Z.zlib_stream(data, CHUNK, TILE, near, RULE)
    assert zlib.decompress(stream) == data
    out, eof, unused = D.inflate(stream)
    assert out == data and eof and unused == b""
    which, chosen, bits_lz, bits_rle = Z.chosen_stream(data, CHUNK, TILE, near, RULE)
    rle = D.zlib_stream(data, CHUNK, TILE)
    assert zlib.decompress(chosen) == data and len(chosen) <= len(rle), (name, which, len(chosen), len(rle))
    assert chosen == (stream if which == "lz" else rle)
    if name in ("period 7", "repeated row"):
        assert which == "lz" and 10 * len(chosen) <= len(rle), (name, len(chosen), len(rle))
    if name in ("panel", "rgb panel", "match of 258", "source in the group before"):
        assert which == "lz"
    if name in ("noise near 1", "zeros", "mixed chunk"):
        assert which == "rle"


@pytest.mark.parametrize("name", NAMES)
def test_the_built_codes_are_complete_limited_and_described_by_their_header(name):
    hist_ll, hist_d, code_ll, code_d, header, nbits = product_codes(name)
    len_ll, len_d = [int(v) for v in code_ll["length"]], [int(v) for v in code_d["length"]]
    assert len(len_ll) == D.SYMBOLS and len(len_d) == Z.DIST_SYMBOLS and nbits == 1338
    for lengths, hist in ((len_ll, hist_ll), (len_d, hist_d)):
        assert D.kraft(lengths) == 1 << 15 and max(lengths) <= 15 and sum(1 for v in lengths if v) >= 2
        assert all(lengths[s] > 0 for s in range(len(lengths)) if hist[s])
    assert len_ll[D.EOB] > 0
    assert [int(v) for v in code_ll["bits"]] == D.canonical_codes(len_ll) and [int(v) for v in code_d["bits"]] == D.canonical_codes(len_d)
    assert D.parse_header(header, nbits) == (0, len_ll, len_d)
    assert (header, nbits) == Z.dynamic_header(len_ll, len_d)
    # the product's codes carry the model's tokens through zlib
    data, near = STREAMS[name]
    assert zlib.decompress(Z.zlib_stream(data, CHUNK, TILE, near, RULE, lengths=(len_ll, len_d), header=(header, nbits))) == data
    # never cheaper than the optimal limited codes, and as cheap where Huffman's own tree fits 15 bits
    best_ll, best_d = Z.model_lengths(hist_ll, hist_d)
    cost = int((hist_ll * np.array(len_ll)).sum() + (hist_d * np.array(len_d)).sum())
    optimal = int((hist_ll * np.array(best_ll)).sum() + (hist_d * np.array(best_d)).sum())
    assert cost >= optimal
    if max(D.limited_lengths(np.maximum(hist_ll, np.eye(D.SYMBOLS, dtype=np.int64)[0]), 40)) <= 15:
        assert cost == optimal


def test_build_codes_lz_on_degenerate_counts_and_its_refusals():
    import ctypes
    one = lambda n, s, v=5: (np.eye(n, dtype=np.uint32)[s] * v).astype(np.uint32)      # noqa: E731
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for hist_ll, hist_d in ((np.zeros(286, np.uint32), np.zeros(30, np.uint32)), (one(286, 77), one(30, 0)), (one(286, 256), one(30, 1)), (one(286, 285), one(30, 29)),
                            (np.ones(286, np.uint32), np.ones(30, np.uint32)), (np.full(286, 0xFFFFFFFF, np.uint32), np.full(30, 0xFFFFFFFF, np.uint32)),
                            (np.ones(286, np.uint32), np.array(fib, np.uint32))):
        code_ll, code_d, header, nbits = png.huffman_codes_lz(hist_ll, hist_d)
        len_ll, len_d = [int(v) for v in code_ll["length"]], [int(v) for v in code_d["length"]]
        assert D.kraft(len_ll) == 1 << 15 and D.kraft(len_d) == 1 << 15 and max(len_ll + len_d) <= 15 and len_ll[D.EOB] > 0
        assert all(len_d[s] for s in range(30) if hist_d[s]) and sum(1 for v in len_d if v) >= 2
        assert D.parse_header(header, nbits) == (0, len_ll, len_d)
    assert [int(v) for v in png.huffman_codes_lz(np.zeros(286, np.uint32), one(30, 0))[1]["length"]][:3] == [1, 1, 0]      # symbol 1 joins symbol 0
    assert [int(v) for v in png.huffman_codes_lz(np.zeros(286, np.uint32), one(30, 7))[1]["length"]][:2] == [1, 0]         # symbol 0 joins the others
    with pytest.raises(ValueError, match="histograms"):
        png.huffman_codes_lz(np.zeros(286, np.uint32), np.zeros(29, np.uint32))
    lib = L.load_library()
    hl, hd = np.ones(286, np.uint32), np.ones(30, np.uint32)
    cl, cd, header, nbits = np.full(286, 0x5A5A5A5A, np.uint32), np.full(30, 0x5A5A5A5A, np.uint32), np.full(256, 0x5A, np.uint8), ctypes.c_int32(-7)
    good = [hl.ctypes.data, hd.ctypes.data, cl.ctypes.data, cd.ctypes.data, header.ctypes.data, 256, ctypes.byref(nbits)]
    for k in (0, 1, 2, 3, 4, 6):
        assert lib.radnet_deflate_build_codes_lz(*[None if i == k else v for i, v in enumerate(good)]) == -1, k
    assert lib.radnet_deflate_build_codes_lz(*[167 if i == 5 else v for i, v in enumerate(good)]) == -1
    assert (cl == 0x5A5A5A5A).all() and (cd == 0x5A5A5A5A).all() and (header == 0x5A).all() and nbits.value == -7
    assert lib.radnet_deflate_build_codes_lz(*[168 if i == 5 else v for i, v in enumerate(good)]) == 0 and nbits.value == 1338 and (header[168:] == 0x5A).all()


@pytest.mark.parametrize("name", NAMES)
def test_stream_bits_and_piece_cap_against_the_model(name):
    data, near = STREAMS[name]
    chunks = -(-len(data) // CHUNK)
    hist_ll, hist_d, code_ll, code_d, header, nbits = product_codes(name)
    len_ll, len_d = [int(v) for v in code_ll["length"]], [int(v) for v in code_d["length"]]
    bits_lz = png.stream_bits(hist_ll, code_ll, nbits, chunks, hist_d, code_d)
    assert bits_lz == Z.stream_bits(hist_ll, hist_d, len_ll, len_d, 0, nbits, chunks)
    pieces = Z.pieces(toks(name), len_ll, len_d, header, nbits)
    # the pieces hold exactly these bits, and behind them the flush (35 bits and the zero bits up to a byte) or the last piece's padding
    assert bits_lz + 35 * (chunks - 1) <= 8 * sum(len(p) for p in pieces) <= bits_lz + 35 * (chunks - 1) + 7 * chunks
    cap = int(L.load_library().radnet_deflate_lz_piece_cap(code_ll.ctypes.data, code_d.ctypes.data, nbits))
    assert max(len(p) for p in pieces) <= cap
    rle_hist = D.histogram(data, CHUNK, TILE)
    hc = png.huffman_code(rle_hist)
    rle_len = [int(v) for v in hc.code["length"]]
    bits_rle = png.stream_bits(rle_hist, hc.code, hc.header_nbits, chunks, dist_nbits=hc.dist_nbits)
    assert bits_rle == Z.stream_bits(rle_hist, None, rle_len, None, 1, hc.header_nbits, chunks)
    rle_pieces = D.pieces(data, CHUNK, TILE, rle_len, hc.header, hc.header_nbits, 1)
    assert bits_rle + 35 * (chunks - 1) <= 8 * sum(len(p) for p in rle_pieces) <= bits_rle + 35 * (chunks - 1) + 7 * chunks


def test_stream_bits_and_piece_cap_refusals():
    lib = L.load_library()
    hist_ll, hist_d = np.ones(286, np.uint32), np.ones(30, np.uint32)
    code_ll, code_d, header, nbits = png.huffman_codes_lz(hist_ll, hist_d)
    p = lambda a: a.ctypes.data      # noqa: E731
    assert lib.radnet_deflate_stream_bits(p(hist_ll), p(hist_d), p(code_ll), p(code_d), 0, nbits, 1) > 0
    bad = code_d.copy()
    bad["length"][3] = 16
    for args in ((None, p(hist_d), p(code_ll), p(code_d), 0, nbits, 1), (p(hist_ll), p(hist_d), None, p(code_d), 0, nbits, 1),
                 (p(hist_ll), None, p(code_ll), p(code_d), 0, nbits, 1), (p(hist_ll), p(hist_d), p(code_ll), None, 0, nbits, 1),
                 (p(hist_ll), p(hist_d), p(code_ll), p(bad), 0, nbits, 1), (p(hist_ll), p(hist_d), p(code_ll), p(code_d), 16, nbits, 1),
                 (p(hist_ll), p(hist_d), p(code_ll), p(code_d), 0, 2, 1), (p(hist_ll), p(hist_d), p(code_ll), p(code_d), 0, nbits, 0),
                 (p(hist_ll), p(hist_d), p(code_ll), p(code_d), 0, nbits, 65537)):
        assert lib.radnet_deflate_stream_bits(*args) == -1
    # equal counts: lengths 8 and 9, 4 and 5; the longest match is 9 + 5 extra + 5 + 13 extra = 32 bits on three bytes, 11 a byte
    assert max(code_ll["length"]) == 9 and max(code_d["length"]) == 5
    assert lib.radnet_deflate_lz_piece_cap(p(code_ll), p(code_d), nbits) == 168 + 11 * CHUNK // 8 + 16
    for args in ((None, p(code_d), nbits), (p(code_ll), None, nbits), (p(code_ll), p(bad), nbits), (p(code_ll), p(code_d), 2), (p(code_ll), p(code_d), 2049)):
        assert lib.radnet_deflate_lz_piece_cap(*args) == -1
    no_eob = code_ll.copy()
    no_eob["length"][256], no_eob["bits"][256] = 0, 0
    assert lib.radnet_deflate_lz_piece_cap(p(no_eob), p(code_d), nbits) == -1


def test_each_mutant_is_caught_by_its_case():
    def tokens_of(name, **mutant):
        data, near = STREAMS[name]
        return Z.tokens(data, CHUNK, TILE, near, RULE, **mutant)

    def inflates(name, **mutant):
        data, near = STREAMS[name]
        try:
            return zlib.decompress(Z.zlib_stream(data, CHUNK, TILE, near, RULE, **mutant)) == data
        except (zlib.error, ValueError):             # ValueError: the model has no symbol for a distance of 32769
            return False

    assert set(Z.MUTANTS) == {"far32769", "no_tile_cut", "own_group", "dist_msb", "tie_larger"}
    # a distance of 32769: the tokens differ and zlib refuses the stream
    assert matches(tokens_of("source 32769 back", far32769=True)) == [(60, 32769)] and not inflates("source 32769 back", far32769=True)
    assert inflates("source 32769 back")
    # the length not cut at the tile: one match of 40 where the rule has 25 (zlib reads both: only the model tells)
    assert matches(tokens_of("match cut by the tile end", no_tile_cut=True))[0] == (40, 300) != matches(toks("match cut by the tile end"))[0]
    # the own group visible: a match where the rule has none
    assert matches(tokens_of("source in the own group only", own_group=True)) == [(40, 100)] and matches(toks("source in the own group only")) == []
    # the distance's extra bits most significant bit first: the stream no longer inflates to the input
    assert not inflates("source in the group before", dist_msb=True) and inflates("source in the group before")
    # the larger distance on a tie
    assert matches(tokens_of("tie between distance 1 and near", tie_larger=True))[1] == (258, 236) != matches(toks("tie between distance 1 and near"))[1]


def test_what_encode_device_refuses_beside_device_lz():
    img = np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match="fixed"):
        png.encode_device(img, deflate="device-lz", huffman="fixed")
    for kw in (dict(level=6), dict(strategy="default"), dict(workers=2), dict(chunk_bytes=1 << 16)):
        with pytest.raises(ValueError, match="host deflate"):
            png.encode_device(img, deflate="device-lz", **kw)
    with pytest.raises(ValueError, match="device-lz"):
        png.encode_device(img, deflate="device-lzz")
    with pytest.raises(ValueError, match="crc"):
        png.encode_device(img, deflate="host", crc="device")


def test_the_mode_goes_through_imwrite_write_predictions_and_evaluate_scans(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(png, "encode_device", lambda img, **kw: seen.append(kw) or b"PNG")
    report = {}
    assert utils_io.imwrite(str(tmp_path / "a.png"), "img", deflate="device-lz", report=report) is True
    assert seen == [dict(deflate="device-lz", report=report)] and seen[0]["report"] is report
    del seen[:]

    class _Config:
        class_mapping = {"boat": 0, "human": 1, "bg": 2}

    net = R.RADNet(_Config(), None, None, None)
    monkeypatch.setattr(R, "draw_rects_device", lambda img, rects, inplace=False, ctx=None: img)
    dets = [{'class': 'boat', 'prob': 0.5, 'x1': 1, 'y1': 2, 'x2': 30, 'y2': 40}]
    net.write_predictions(dets, "map", str(tmp_path / "p1"), deflate="device-lz")
    net.write_predictions(dets, "map", str(tmp_path / "p2"), deflate="device-lz", crc="device")
    assert seen == [dict(deflate="device-lz", huffman="dynamic")] * 4 + [dict(deflate="device-lz", huffman="dynamic", crc="device")] * 4

    writes = []
    monkeypatch.setattr(utils_io, "get_image", lambda path, types, random_type=False, to_host=True: "map")
    monkeypatch.setattr(utils_io, "imwrite", lambda path, img, **kw: writes.append(kw) or True)

    class _Net:
        def predict_from_path(self, path):
            return [dict(dets[0])]

        def draw_detections(self, img, dets, **kw):
            return img

    records = [{'filepath': 'scan', 'bboxes': [{'class': 'boat', 'x1': 1, 'y1': 2, 'x2': 30, 'y2': 40}]}]
    evaluate.evaluate_scans(_Net(), records, str(tmp_path / "e1"), deflate="device-lz")
    assert writes == [dict(deflate="device-lz", huffman="dynamic")]


def test_the_library_exports_the_entries_and_the_mirrors_match():
    declared = L.declared_symbols()
    lib = L.load_library()
    for name in ("radnet_deflate_lz_scan_u8", "radnet_deflate_lz_emit_u8", "radnet_deflate_build_codes_lz", "radnet_deflate_lz_piece_cap",
                 "radnet_deflate_stream_bits"):
        assert name in declared and hasattr(lib, name)
    assert png.DEFLATE_DIST_SYMBOLS == Z.DIST_SYMBOLS and TILE % RULE["group"] == 0 and 4 <= RULE["far_min"] <= RULE["far_min2"]
