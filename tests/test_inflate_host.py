"""The device inflate's Python model (tests/inflate_cases.py) against zlib, and its host entry against the model -- no GPU:
every eligible case chains to zlib.decompress's bytes and its candidates hold every true dynamic block; the header rule agrees with
zlib.decompressobj(-15) on bit-flipped real headers; radnet_inflate_chain equals the model's chain with every refusal code; each
mutant of the model is caught by a named case; the header's constants are the model's."""
import ctypes
import zlib

import numpy as np
import pytest

import inflate_cases as I

ELIGIBLE = I.ELIGIBLE + ("g png.assemble",)
HEADER_MESSAGES = ("invalid block type", "too many length or distance symbols", "invalid code lengths set", "invalid bit length repeat",
                   "invalid code -- missing end-of-block", "invalid literal/lengths set", "invalid distances set")


def case(name):
    return {**I.cases(), **(I.package_cases() if name == "g png.assemble" else {})}[name]


@pytest.mark.parametrize("name", ELIGIBLE)
def test_the_model_inflates_every_eligible_case(name):
    c = case(name)
    out, reason, stats = I.model(name)
    assert reason is None and out == c.data == zlib.decompress(c.z), (name, reason)
    assert stats["units"] >= 1 and stats["blocks"] >= stats["units"]


@pytest.mark.parametrize("name", ELIGIBLE)
def test_the_candidates_hold_every_true_dynamic_block(name):
    c = case(name)
    true = I.true_dynamic_starts(c.z)
    cands = I.find_blocks(c.z, 16)
    assert set(true) <= set(cands), (name, sorted(set(true) - set(cands)))
    assert cands == sorted(cands) and len(set(cands)) == len(cands)
    if name != "d stored with buried headers":
        assert cands == true, name                                       # and nothing else, in these streams


def test_what_the_cases_are_made_to_show():
    cs = I.cases()
    ends = {u[1] % 8 for u in I.model_units("b memlevel 1")[2]}
    assert ends == set(range(8)), "memLevel 1: block ends on every bit phase"
    assert len(I.model_units("b memlevel 1")[0]) > 100
    assert (cs["c flushes"].z[2] >> 1) & 3 == 0, "the first block of the flush case is stored"
    assert I.model("c flushes")[2]["blocks"] > I.model("c flushes")[2]["units"], "units with stored tails"
    assert I.model("d stored with buried headers")[2]["false_candidates"] > 0
    units = I.model_units("e long runs")[2]
    inherit = [u for u in units if u[6] & I.LEAD_MATCH and not u[6] & I.LAST_KNOWN]
    assert len(inherit) >= 2, "units of matches alone: the byte in front is inherited through several"
    assert I.model("g deflate model fixed")[2]["candidates"] == 0 and I.model("g deflate model fixed")[2]["blocks"] >= 3
    for name in ("h unit cap", "i level 6", "i distance 2", "j bytes behind the final block", "j wrong adler", "k incomplete header"):
        out, reason, _ = I.model(name)
        assert out is None and reason == cs[name].reason, (name, reason)
    for name in ("j flipped bit", "j truncated"):
        assert I.model(name)[0] is None and I.model(name)[1], name
    assert zlib.decompress(cs["j bytes behind the final block"].z) == cs["a cv2-like"].data      # zlib ignores what stands behind
    rec = I.decode_unit(cs["h unit cap"].z, 16, cap=I.MAX_SYMBOLS + 41)
    assert rec[5] == I.OK and rec[3] == I.MAX_SYMBOLS + 41, "one symbol under the cap the same unit decodes"


def zlib_verdict(bits_from_header):
    """'accept' when zlib.decompressobj(-15) reads past the header, 'reject' on one of its header messages."""
    d = zlib.decompressobj(-15)
    try:
        d.decompress(bits_from_header)
    except zlib.error as e:
        if any(m in str(e) for m in HEADER_MESSAGES):
            return "reject"
    return "accept"


def realign(z, bit, take_bits):
    """take_bits bits of z from bit offset `bit` on as bytes that start at bit 0."""
    v = int.from_bytes(z, "little") >> bit
    return (v & ((1 << take_bits) - 1)).to_bytes((take_bits + 7) // 8, "little")


def test_the_header_rule_agrees_with_zlib_on_bit_flipped_headers():
    rs = np.random.RandomState(12)
    z = I.cases()["a cv2-like"].z
    starts = [s for s in I.model_units("a cv2-like")[0] if s + 3000 + 6000 < 8 * len(z)]
    headers = [bytearray(realign(z, s, 12000)) for s in starts]         # the header (at most 4,509 bits) and more than 6,000 bits behind it
    for h in headers:
        h[0] &= 0xFE                                                     # BFINAL 0: zlib goes on reading
        assert I.parse_dynamic(bytes(h), 3, 8 * len(h))[0] == I.OK and zlib_verdict(bytes(h)) == "accept"
    tried = accepted = 0
    for k in range(2400):
        h = bytearray(headers[k % len(headers)])
        end = I.parse_dynamic(bytes(h), 3, 8 * len(h))[1]
        for _ in range(rs.randint(1, 4)):
            bit = rs.randint(0, end)
            h[bit >> 3] ^= 1 << (bit & 7)
        h = bytes(h)
        mine = "accept" if (h[0] >> 1) & 3 == 2 and I.parse_dynamic(h, 3, 8 * len(h))[0] == I.OK else "reject"
        if (h[0] >> 1) & 3 != 2:
            continue                                                     # the flip made another block type of it: not a header any more
        tried += 1
        accepted += mine == "accept"
        assert mine == zlib_verdict(h), (k, mine)
    assert tried >= 2000 and accepted >= 10, (tried, accepted)


def chain_native(units, first_bit, n, expected):
    from faster_rcnn import png
    from radnet_hip import lib as L
    table = np.array([tuple(u) for u in units], png.INFLATE_UNIT)
    links = np.zeros(len(units), png.INFLATE_LINK)
    nl, nf, bad = ctypes.c_int32(-9), ctypes.c_int32(-9), ctypes.c_int32(-9)
    rc = L.load_library().radnet_inflate_chain(table.ctypes.data, len(table), first_bit, n, expected, links.ctypes.data, len(links), ctypes.byref(nl),
                                               ctypes.byref(nf), ctypes.byref(bad))
    got = [(int(l["out_offset"]), int(l["start_bit"]), int(l["out_bytes"]), int(l["prev_byte"])) for l in links[:max(nl.value, 0)]]
    return rc, bad.value, got, nf.value


def test_the_native_chain_equals_the_model():
    seen = set()
    for name, c in {**I.cases(), **I.package_cases()}.items():
        if name == "g png.assemble":
            cands = I.find_blocks(c.z, 16)
            starts = sorted(set(cands) | {16})
            units = I.measure(c.z, starts)
        else:
            _, starts, units = I.model_units(name)
        want = I.chain(units, 16, len(c.z), c.expected)
        got = chain_native(units, 16, len(c.z), c.expected)
        assert got == want, (name, got[:2], want[:2])
        seen.add(want[0])
        for first_bit, n, expected in ((17, len(c.z), c.expected), (16, len(c.z) + 1, c.expected), (16, len(c.z), c.expected + 1)):
            want = I.chain(units, first_bit, n, expected)
            assert chain_native(units, first_bit, n, expected) == want, (name, first_bit, n, expected)
            seen.add(want[0])
    # a stream whose first unit begins with a match: the long-runs case entered at its second unit
    c = I.cases()["e long runs"]
    _, starts, units = I.model_units("e long runs")
    want = I.chain(units[1:], starts[1], len(c.z), c.expected)
    assert want[0] == I.CHAIN_LEAD_MATCH and chain_native(units[1:], starts[1], len(c.z), c.expected) == want
    seen.add(want[0])
    assert seen == {I.CHAIN_OK, I.CHAIN_NO_START, I.CHAIN_BAD_UNIT, I.CHAIN_LEAD_MATCH, I.CHAIN_LENGTH, I.CHAIN_TRAILER}, seen


CAUGHT_BY = {"end_off_by_one": "a cv2-like", "no_inherit": "e long runs", "no_stored_tail": "c flushes", "accept_incomplete": "k incomplete header",
             "ignore_distance": "i distance 2"}


@pytest.mark.parametrize("mutant", I.MUTANTS)
def test_every_mutant_of_the_model_is_caught(mutant):
    c = I.cases()[CAUGHT_BY[mutant]]
    right = I.model(c.name)
    wrong = I.inflate(c.z, c.expected, **{mutant: True})
    assert (right[0], right[1]) == (c.data if c.reason is None else None, c.reason)
    assert (wrong[0], wrong[1]) != (right[0], right[1]), mutant
    if mutant == "accept_incomplete":
        assert wrong[2]["candidates"] == 1 and right[2]["candidates"] == 0 and zlib_verdict(c.z[2:]) == "reject"
    if mutant == "ignore_distance":
        assert wrong[1] == "adler", "the wrong bytes come out and only the checksum sees it"


def test_the_header_states_the_models_constants():
    from faster_rcnn import png
    from radnet_hip import lib as L
    assert L.header_constant("RADNET_INFLATE_UNIT_MAX_SYMBOLS") == I.MAX_SYMBOLS == 1 << 18
    for k, name in enumerate(("OK", "BAD_HEADER", "BAD_CODE", "NOT_RLE", "STORED_MISMATCH", "PAST_END", "TOO_LONG")):
        assert L.header_constant("RADNET_INFLATE_" + name) == k
    for k, name in enumerate(("OK", "NO_START", "BAD_UNIT", "LEAD_MATCH", "LENGTH", "TRAILER")):
        assert L.header_constant("RADNET_INFLATE_CHAIN_" + name) == k
    assert [L.header_constant("RADNET_INFLATE_FLAG_" + n) for n in ("FINAL", "LEAD_MATCH", "LAST_KNOWN")] == [I.FINAL, I.LEAD_MATCH, I.LAST_KNOWN]
    assert png.INFLATE_UNIT.itemsize == 32 and png.INFLATE_LINK.itemsize == 24 and png.INFLATE_UNIT.names == I.UNIT_FIELDS
    assert png.INFLATE_STATUS == I.STATUS_NAMES and png.INFLATE_CHAIN == I.CHAIN_NAMES


def test_parse_compressed_is_the_container_walk_of_parse():
    import png_cases as K
    from faster_rcnn import png
    rs = np.random.RandomState(3)
    for color, depth, interlace in ((2, 8, False), (3, 4, True), (6, 16, False)):
        pal = rs.randint(0, 256, (16, 3)) if color == 3 else None
        enc = K.encode(K.draw(rs, 9, 14, color, depth), color, depth, filters=rs, interlace=interlace, palette=pal, idat_sizes=[7, 1, 30])
        comp, img = png.parse_compressed(np.frombuffer(enc.data, np.uint8)), png.parse(enc.data)
        assert (comp.header, comp.passes, comp.bpp, comp.expected) == (img.header, img.passes, img.bpp, len(img.stream))
        assert np.array_equal(comp.palette, img.palette) and np.array_equal(comp.staged.numpy()[comp.n:], img.palette.reshape(-1))
        assert zlib.decompress(comp.staged.numpy()[:comp.n].tobytes()) == img.stream
        bad = bytearray(enc.data)
        bad[len(bad) - 20] ^= 4
        with pytest.raises(ValueError) as a:
            png.parse(bytes(bad))
        with pytest.raises(ValueError) as b:
            png.parse_compressed(bytes(bad))
        assert str(a.value) == str(b.value) and "CRC" in str(a.value)
    enc = K.encode(K.draw(rs, 5, 5, 0, 8), 0, 8)
    idat = enc.data.index(b"IDAT")
    for first, second in ((0x79, 0x9C), (0x78, 0x9D), (0x78, 0xBB)):       # CM 9; FCHECK; a preset dictionary (FCHECK right)
        payload = bytes([first, second]) + enc.data[idat + 6:enc.data.index(b"IEND") - 8]
        data = enc.data[:idat - 4] + K.chunk(b"IDAT", payload) + K.chunk(b"IEND")
        with pytest.raises(ValueError, match="zlib header"):
            png.parse_compressed(data)


def test_the_native_chunk_crcs_equal_zlib():
    import png_cases as K
    from faster_rcnn import png
    from radnet_hip import lib as L
    rs = np.random.RandomState(17)
    chunks = [K.chunk(b"IDAT", rs.randint(0, 256, n).astype(np.uint8).tobytes()) for n in (0, 1, 7, 8, 9, 8192, 100000, 33)] + [K.chunk(b"IEND")]
    blob = np.frombuffer(b"".join(chunks), np.uint8).copy()
    at = np.cumsum([0] + [len(c) for c in chunks[:-1]]).astype(np.int64)
    end = (at + np.array([len(c) for c in chunks]) - 4).astype(np.int64)
    check = lambda workers: L.load_library().radnet_png_check_crcs(blob.ctypes.data, len(blob), at.ctypes.data, end.ctypes.data, len(chunks), workers)      # noqa: E731
    assert [check(w) for w in (1, 2, 8, 99)] == [len(chunks)] * 4
    for k in range(len(chunks)):
        blob[at[k] + 4] ^= 0x20
        assert check(3) == k
        blob[at[k] + 4] ^= 0x20
    # through parse_compressed: a file above the 1 MiB where the native sums take over, cut into 8 KiB chunks
    samples = K.draw(rs, 700, 700, 2, 8)
    enc = K.encode(samples, 2, 8, filters=0, idat_sizes=[8192] * 150, level=1)
    assert len(enc.data) > 1 << 20
    comp = png.parse_compressed(enc.data)
    assert zlib.decompress(comp.staged.numpy()[:comp.n].tobytes()) == enc.stream
    bad = bytearray(enc.data)
    bad[len(bad) // 2] ^= 1
    with pytest.raises(ValueError) as a:
        png.parse(bytes(bad))
    with pytest.raises(ValueError) as b:
        png.parse_compressed(bytes(bad))
    assert str(a.value) == str(b.value) and "CRC" in str(a.value)


def test_two_faults_in_one_file_are_reported_in_each_parsers_order():
    """parse() sums a chunk's CRC before it looks at the next chunk; parse_compressed() judges the whole structure before any sum."""
    import png_cases as K
    from faster_rcnn import png
    enc = K.encode(K.draw(np.random.RandomState(5), 6, 7, 3, 8), 3, 8, palette=np.arange(30).reshape(10, 3))
    plte, idat = enc.data.index(b"PLTE") - 4, enc.data.index(b"IDAT") - 4
    head, pal, z, end = enc.data[:33], enc.data[plte:idat], enc.data[idat:-12], enc.data[-12:]
    assert head + pal + z + end == enc.data and (plte, idat, len(z)) == (33, 75, 71)
    bad = lambda chunk: chunk[:-1] + bytes([chunk[-1] ^ 1])      # noqa: E731  (the CRC field)
    for what, data, from_parse, from_parse_compressed in (
            ("a bad CRC in chunk 2, chunk 3 truncated", head + bad(pal) + z[:-3],
             "PNG: CRC mismatch in the b'PLTE' chunk at byte 33", "PNG: truncated file (b'IDAT' chunk of 59 bytes at byte 75)"),
            ("a second IHDR after a bad-CRC PLTE", head + bad(pal) + head[8:] + z + end,
             "PNG: CRC mismatch in the b'PLTE' chunk at byte 33", "PNG: a second IHDR chunk"),
            ("no IEND after a bad-CRC IDAT", head + pal + bad(z),
             "PNG: CRC mismatch in the b'IDAT' chunk at byte 75", "PNG: truncated file (no IEND chunk)")):
        for parser, want in ((png.parse, from_parse), (png.parse_compressed, from_parse_compressed)):
            with pytest.raises(ValueError) as e:
                parser(data)
            assert str(e.value) == want, (what, parser.__name__)


def test_the_modes_are_stated_once():
    from faster_rcnn import png, utils_io
    needs_inflate = "PNG: crc=\"device\" sums the uploaded IDAT stream and needs inflate=\"device\" or \"device-lz\", not inflate=\"host\""
    for kw, want in ((dict(inflate="gpu"), "PNG: inflate='gpu' (\"host\", \"device\" or \"device-lz\")"),
                     (dict(unfilter="rows"), "PNG: unfilter='rows' (\"band\" or \"tiles\")"),
                     (dict(crc="gpu"), "PNG: crc='gpu' (\"host\" or \"device\")"),
                     (dict(inflate="host", crc="device"), needs_inflate)):
        for taker in (png.check_modes, utils_io.DeviceImageLoader, lambda **k: png.decode_device(b"", **k)):
            with pytest.raises(ValueError) as e:
                taker(**kw)
            assert str(e.value) == want, kw
    for inflate, unfilter, crc in (("host", "band", "host"), ("device", "tiles", "device"), ("device-lz", "band", "device"), ("device-lz", "tiles", "host")):
        png.check_modes(inflate, unfilter, crc)
        utils_io.DeviceImageLoader(inflate=inflate, unfilter=unfilter, crc=crc)
    png.check_modes()
