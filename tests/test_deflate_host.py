"""The device deflate's host side and its model, no device needed: the Python model of tests/deflate_cases.py inflates through zlib
for every case and both Huffman modes; radnet_deflate_build_code (png.huffman_code) gives complete codes of at most 15 bits whose
header parses back to them and which zlib accepts; png.assemble_pieces wraps a stream the tests' own PNG decoder reads; the
mutants of the model are caught; the dynamic mode stays within 5 % of zlib's level 1 Z_RLE on the panel; the new arguments go
through imwrite, write_predictions and evaluate_scans and the defaults pass none."""
import zlib

import numpy as np
import pytest

import deflate_cases as D
import png_write_cases as W
from faster_rcnn import RADNet as R
from faster_rcnn import evaluate, png, utils_io
from radnet_hip import lib as L

CHUNK, TILE = L.header_constant("RADNET_DEFLATE_CHUNK"), L.header_constant("RADNET_DEFLATE_TILE")
STREAMS = D.streams(CHUNK, TILE)
NAMES = sorted(STREAMS)
SMALL = (777, 64)                                  # a second cut: chunks and tiles no power of two, many pieces


@pytest.fixture(scope="module")
def hists():
    return {name: D.histogram(STREAMS[name], CHUNK, TILE) for name in NAMES}


def product_code(hist):
    hc = png.huffman_code(hist)
    return hc, [int(v) for v in hc.code["length"]]


def test_the_case_table_holds_what_it_promises(hists):
    assert [len(STREAMS["mixed " + k]) for k in ("1", "tile-1", "tile", "tile+1", "chunk-1", "chunk", "chunk+1", "2chunk+3")] == \
        [1, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    assert set(STREAMS["all byte values"]) == set(range(256)) and set(STREAMS["zeros"]) == {0}
    assert len(STREAMS["zeros"]) > CHUNK and len(STREAMS["noise"]) > CHUNK
    used = [w for w in hists["skewed"] if w]
    assert max(D.limited_lengths(hists["skewed"], 40)) > 15 and len(used) <= 1 << 15      # the unlimited tree is deeper than 15
    assert len(STREAMS["panel"]) == 300 * 402


def test_the_rule_on_runs_written_out_by_hand():
    for length, want in D.RUN_TOKENS.items():
        want = [("lit", 9) if t == "l" else ("match", int(t)) for t in want.split()]
        assert D.run_tokens(9, length) == want, length
        assert D.tokens(bytes([9]) * length, CHUNK, TILE) == [want], length
    # a run over a tile boundary is two runs, over a chunk boundary two runs in two pieces
    assert D.tokens(bytes([3]) * (TILE + 4), CHUNK, TILE) == [D.run_tokens(3, TILE) + [("lit", 3), ("match", 3)]]
    assert D.tokens(bytes([3]) * (CHUNK + 2), CHUNK, TILE) == [D.run_tokens(3, TILE) * (CHUNK // TILE), [("lit", 3), ("lit", 3)]]
    for length in range(3, 259):
        symbol, extra_bits, extra = D.length_symbol(length)
        assert D.LENGTH_TABLE[symbol - 257][0] + extra == length and extra < (1 << extra_bits) or length == 258
    assert D.length_symbol(258) == (285, 0, 0) and D.length_symbol(257) == (284, 5, 30)


@pytest.mark.parametrize("name", NAMES)
def test_the_model_inflates_to_the_input(name, hists):
    data = STREAMS[name]
    hc, lengths = product_code(hists[name])
    for what, stream in (("model code", D.zlib_stream(data, CHUNK, TILE)), ("fixed", D.zlib_stream(data, CHUNK, TILE, "fixed")),
                         ("product code", D.zlib_stream(data, CHUNK, TILE, lengths=lengths, header=(hc.header, hc.header_nbits)))):
        out, eof, unused = D.inflate(stream)
        assert out == data and eof and unused == b"", (name, what)
    if len(data) <= 2 * TILE + 1 or name in ("runs", "all byte values"):      # the small cut on the small cases: many pieces
        for mode in ("dynamic", "fixed"):
            out, eof, unused = D.inflate(D.zlib_stream(data, SMALL[0], SMALL[1], mode))
            assert out == data and eof and unused == b"", (name, mode, "small cut")


@pytest.mark.parametrize("name", NAMES)
def test_the_built_code_is_complete_limited_and_described_by_its_header(name, hists):
    hist = hists[name]
    hc, lengths = product_code(hist)
    assert hc.dist_nbits == 1 and hc.code.dtype.itemsize == 4 and len(lengths) == D.SYMBOLS
    assert D.kraft(lengths) == 1 << 15 and max(lengths) <= 15
    assert all(lengths[s] > 0 for s in range(D.SYMBOLS) if hist[s]) and lengths[D.EOB] > 0
    assert [int(v) for v in hc.code["bits"]] == D.canonical_codes(lengths)
    bfinal, lit, dist = D.parse_header(hc.header, hc.header_nbits)
    assert (bfinal, lit, dist) == (0, lengths, [1])
    assert (hc.header, hc.header_nbits) == D.dynamic_header(lengths)
    # against the optimal limited code: never cheaper, and as cheap where Huffman's own tree fits 15 bits (both are optimal then)
    best = D.limited_lengths(hist)
    cost, optimal = int((hist * np.array(lengths)).sum()), int((hist * np.array(best)).sum())
    assert cost >= optimal
    if max(D.limited_lengths(hist, 40)) <= 15:
        assert cost == optimal
    assert png.huffman_code(hist).code.tobytes() == hc.code.tobytes()                           # deterministic


def test_build_code_on_degenerate_counts_and_its_refusals():
    import ctypes
    for hist in (np.zeros(286, np.uint32), np.eye(286, dtype=np.uint32)[0] * 5, np.eye(286, dtype=np.uint32)[77] * 9,
                 np.eye(286, dtype=np.uint32)[256], np.full(286, 0xFFFFFFFF, np.uint32), np.ones(286, np.uint32)):
        hc, lengths = product_code(hist)
        assert D.kraft(lengths) == 1 << 15 and lengths[D.EOB] > 0 and sum(1 for v in lengths if v) >= 2
        assert all(lengths[s] for s in range(286) if hist[s])
        assert D.parse_header(hc.header, hc.header_nbits)[1] == lengths
    with pytest.raises(ValueError, match="histogram"):
        png.huffman_code(np.zeros(285, np.uint32))
    lib = L.load_library()
    hist, code, header, nbits = np.ones(286, np.uint32), np.full(286, 0x5A5A5A5A, np.uint32), np.full(256, 0x5A, np.uint8), ctypes.c_int32(-7)
    for args in ((None, code.ctypes.data, header.ctypes.data, 256, ctypes.byref(nbits)), (hist.ctypes.data, None, header.ctypes.data, 256, ctypes.byref(nbits)),
                 (hist.ctypes.data, code.ctypes.data, None, 256, ctypes.byref(nbits)), (hist.ctypes.data, code.ctypes.data, header.ctypes.data, 256, None),
                 (hist.ctypes.data, code.ctypes.data, header.ctypes.data, 152, ctypes.byref(nbits))):
        assert lib.radnet_deflate_build_code(*args) == -1
    assert (code == 0x5A5A5A5A).all() and (header == 0x5A).all() and nbits.value == -7
    assert lib.radnet_deflate_build_code(hist.ctypes.data, code.ctypes.data, header.ctypes.data, 153, ctypes.byref(nbits)) == 0 and nbits.value == 1222
    assert (header[153:] == 0x5A).all()


def test_piece_cap_is_the_stated_bound_and_refuses_bad_tables():
    lib = L.load_library()
    fixed = png.fixed_code()
    assert ([int(v) for v in fixed.code["length"]], [int(v) for v in fixed.code["bits"]]) == D.fixed_code()
    assert (fixed.header, fixed.header_nbits, fixed.dist_nbits) == D.fixed_header() + (5,)
    assert lib.radnet_deflate_piece_cap(fixed.code.ctypes.data, 3, 5) == 1 + 9 * CHUNK // 8 + 16
    hc = png.huffman_code(D.histogram(STREAMS["skewed"], CHUNK, TILE))
    assert lib.radnet_deflate_piece_cap(hc.code.ctypes.data, hc.header_nbits, 1) == 153 + 15 * CHUNK // 8 + 16
    two = np.zeros(286, png.DEFLATE_CODE)                                                     # literal 0 and end-of-block, one bit each
    two["length"][[0, 256]], two["bits"][256] = 1, 1
    assert lib.radnet_deflate_piece_cap(two.ctypes.data, 3, 1) == 1 + 2 * CHUNK // 8 + 16     # a match without a code: (0 + 5 + 1) / 3 bits a byte
    for what, edit in (("length 16", lambda c: c["length"].__setitem__(5, 16)), ("bits beyond the length", lambda c: c["bits"].__setitem__(256, 2)),
                       ("no end-of-block", lambda c: (c["length"].__setitem__(256, 0), c["bits"].__setitem__(256, 0)))):
        bad = two.copy()
        edit(bad)
        assert lib.radnet_deflate_piece_cap(bad.ctypes.data, 3, 1) == -1, what
    for nbits, dist in ((2, 1), (2049, 1), (3, -1), (3, 16)):
        assert lib.radnet_deflate_piece_cap(two.ctypes.data, nbits, dist) == -1
    assert lib.radnet_deflate_piece_cap(None, 3, 1) == -1


# no image has a stream of one byte (the filter-type byte and one sample at least): that case has no file
@pytest.mark.parametrize("name", [n for n in NAMES if len(STREAMS[n]) >= 2])
def test_assemble_pieces_is_read_by_the_independent_decoder(name):
    data = bytearray(STREAMS[name])
    data[0] = 0                                                                                 # one row of filter type None: the bytes are the samples
    data = bytes(data)
    for mode in ("dynamic", "fixed"):
        stream = D.zlib_stream(data, CHUNK, TILE, mode)
        adler = int.from_bytes(stream[-4:], "big")
        assert adler == zlib.adler32(data) == png.adler32_of_parts(np.array(D.adler_parts(data, CHUNK), np.uint64), len(data))
        blob = png.assemble_pieces(stream[2:-4], adler, len(data) - 1, 1, 0)
        d = W.decode(blob)
        assert d.stream == data and d.kinds == [b"IHDR", b"IDAT", b"IEND"] and (d.width, d.height, d.color_type) == (len(data) - 1, 1, 0)
        assert d.samples.tobytes() == data[1:]
    rgb = bytes([0]) + STREAMS["noise"][:3 * 50]
    d = W.decode(png.assemble_pieces(D.zlib_stream(rgb, CHUNK, TILE)[2:-4], zlib.adler32(rgb), 50, 1, 2))
    assert d.color_type == 2 and d.stream == rgb


def test_the_chunk_crc_summed_in_ranges_is_zlibs():
    rs = np.random.RandomState(3)
    for n in (0, 1, 5, 4097, (3 << 20) + 11):
        a, b = rs.randint(0, 256, n).astype(np.uint8).tobytes(), rs.randint(0, 256, 77).astype(np.uint8).tobytes()
        assert png.crc32_combine(zlib.crc32(b), zlib.crc32(a), n) == zlib.crc32(b + a), n
        assert png.crc32_combine(zlib.crc32(a), zlib.crc32(b), 77) == zlib.crc32(a + b), n
    big = rs.randint(0, 256, (9 << 20) + 5).astype(np.uint8).tobytes()                          # nine ranges' worth: eight threads
    blob = png.assemble_pieces(big, 7, 3, 2, 2)
    assert [k for k, _ in W.chunks(blob)] == [b"IHDR", b"IDAT", b"IEND"]                        # W.chunks checks every CRC with zlib.crc32
    assert W.chunks(blob)[1][1] == b"\x78\x01" + big + b"\x00\x00\x00\x07"


def test_assemble_pieces_refusals():
    for args in ((b"x", 1, 5, 5, 3), (b"x", 1, 0, 5, 0), (b"x", 1, 5, 0, 2), (b"x", -1, 5, 5, 0), (b"x", 1 << 32, 5, 5, 0)):
        with pytest.raises(ValueError, match="PNG"):
            png.assemble_pieces(*args)


def fails(data, chunk, tile, mode, **mutant):
    """Does this mutant of the model fail the inflate check on this stream?"""
    try:
        out, eof, unused = D.inflate(D.zlib_stream(data, chunk, tile, mode, **mutant))
    except (zlib.error, ValueError, AssertionError):
        return True
    return not (out == data and eof and unused == b"")


def test_every_mutant_is_caught():
    assert set(D.MUTANTS) == {"cut259", "rest2_match", "lsb_codes", "no_sync", "adler_no_length"}
    multi = [n for n in NAMES if len(STREAMS[n]) > CHUNK]
    # a run cut at 259 still inflates: the hand-written token lists are what catches it
    want = [("lit", 9), ("match", 258), ("match", 258)]
    assert D.run_tokens(9, 517) == want != D.run_tokens(9, 517, cut259=True)
    assert D.tokens(STREAMS["runs"], CHUNK, TILE) != D.tokens(STREAMS["runs"], CHUNK, TILE, cut259=True)
    # a rest of 2 as a match has no length symbol
    assert D.run_tokens(9, 261, rest2_match=True) != [("lit", 9), ("match", 258), ("lit", 9), ("lit", 9)]
    assert fails(STREAMS["runs"], CHUNK, TILE, "dynamic", rest2_match=True) and fails(STREAMS["runs"], CHUNK, TILE, "fixed", rest2_match=True)
    for mode in ("dynamic", "fixed"):
        assert all(fails(STREAMS[n], CHUNK, TILE, mode, lsb_codes=True) for n in ("runs", "noise", "panel")), mode
        assert any(fails(STREAMS[n], CHUNK, TILE, mode, no_sync=True) for n in multi), mode
        assert all(fails(STREAMS[n], CHUNK, TILE, mode, adler_no_length=True) for n in ("noise", "straddle")), mode
        assert not any(fails(STREAMS[n], CHUNK, TILE, mode) for n in ("runs", "noise", "straddle"))      # and the model itself passes
    assert fails(STREAMS["runs"], *SMALL, "dynamic", no_sync=True) and fails(STREAMS["runs"], *SMALL, "dynamic", adler_no_length=True)


def test_the_dynamic_mode_stays_within_five_percent_of_zlib_rle_on_the_panel():
    data = STREAMS["panel"]
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    host = len(c.compress(data) + c.flush())
    hc, lengths = product_code(D.histogram(data, CHUNK, TILE))
    dynamic = len(D.zlib_stream(data, CHUNK, TILE, lengths=lengths, header=(hc.header, hc.header_nbits)))
    fixed = len(D.zlib_stream(data, CHUNK, TILE, "fixed"))
    print("panel: zlib level 1 Z_RLE %d bytes, dynamic %d (%.4f), fixed %d (%.4f)" % (host, dynamic, dynamic / host, fixed, fixed / host))
    assert dynamic <= 1.05 * host


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
def test_encode_device_refuses_host_deflate_arguments_with_the_device_deflate():
    img = np.zeros((4, 5, 3), np.uint8)
    for kw in (dict(level=6), dict(strategy="default"), dict(workers=2), dict(chunk_bytes=100), dict(level=1, workers=1)):
        with pytest.raises(ValueError, match="host deflate"):
            png.encode_device(img, deflate="device", **kw)
    with pytest.raises(ValueError, match="deflate"):
        png.encode_device(img, deflate="gpu")
    with pytest.raises(ValueError, match="huffman"):
        png.encode_device(img, deflate="device", huffman="static")
    with pytest.raises(ValueError, match="filter"):
        png.encode_device(img, filter="best", deflate="device")


def test_the_new_arguments_go_through_and_the_defaults_pass_none(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(png, "encode_device", lambda img, **kw: seen.append(kw) or b"PNG")
    assert utils_io.imwrite(str(tmp_path / "a.png"), "img", deflate="device", huffman="fixed") is True
    assert utils_io.imwrite(str(tmp_path / "b.png"), "img") is True
    assert seen == [dict(deflate="device", huffman="fixed"), {}]
    del seen[:]

    class _Config:
        class_mapping = {"boat": 0, "human": 1, "bg": 2}

    net = R.RADNet(_Config(), None, None, None)
    monkeypatch.setattr(R, "draw_rects_device", lambda img, rects, inplace=False, ctx=None: img)
    dets = [{'class': 'boat', 'prob': 0.5, 'x1': 1, 'y1': 2, 'x2': 30, 'y2': 40}]
    net.write_predictions(dets, "map", str(tmp_path / "p1"))
    net.write_predictions(dets, "map", str(tmp_path / "p2"), deflate="device")
    net.write_predictions(dets, "map", str(tmp_path / "p3"), deflate="device", huffman="fixed")
    assert seen == [{}] * 4 + [dict(deflate="device", huffman="dynamic")] * 4 + [dict(deflate="device", huffman="fixed")] * 4

    writes = []
    monkeypatch.setattr(utils_io, "get_image", lambda path, types, random_type=False, to_host=True: "map")
    monkeypatch.setattr(utils_io, "imwrite", lambda path, img, **kw: writes.append(kw) or True)

    class _Net:
        def predict_from_path(self, path):
            return [dict(dets[0])]

        def draw_detections(self, img, dets, **kw):
            return img

    records = lambda: [{'filepath': 'scan', 'bboxes': [{'class': 'boat', 'x1': 1, 'y1': 2, 'x2': 30, 'y2': 40}]}]      # noqa: E731
    evaluate.evaluate_scans(_Net(), records(), str(tmp_path / "e1"))
    evaluate.evaluate_scans(_Net(), records(), str(tmp_path / "e2"), deflate="device", huffman="fixed")
    assert writes == [{}, dict(deflate="device", huffman="fixed")]


def test_the_library_exports_the_entries_and_the_mirrors_match():
    declared = L.declared_symbols()
    lib = L.load_library()
    for name in ("radnet_deflate_rle_scan_u8", "radnet_deflate_rle_emit_u8", "radnet_deflate_pack", "radnet_deflate_build_code", "radnet_deflate_piece_cap"):
        assert name in declared and hasattr(lib, name)
    assert CHUNK % TILE == 0 and L.header_constant("RADNET_DEFLATE_SYMBOLS") == D.SYMBOLS == png.DEFLATE_SYMBOLS
    assert png.DEFLATE_CODE.itemsize == 4 and list(png.DEFLATE_CODE.names) == ["bits", "length"]
