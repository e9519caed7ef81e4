"""The host half of crc="device" (no device needed): the model of tests/crc32_cases.py against zlib.crc32 and its five mutants against
the cases named for them; radnet_crc32_shift, radnet_crc32_combine and the grain plan (csrc/crc32_plan.cpp over csrc/crc32_rule.h)
against the model and png.crc32_combine; parse_compressed(crc="device")'s segment table; assemble_pieces(idat_crc=); the options'
ValueErrors."""
import struct
import zlib

import numpy as np
import pytest

import crc32_cases as CC
import png_cases
from faster_rcnn import png, utils_io
from radnet_hip import lib as L

ERR_ARG, ERR_UNSUPPORTED = -1, -3
CASES = CC.cases()
BY_NAME = {c[0]: c for c in CASES}


def test_the_constants_the_abi_mirror_and_the_binding():
    assert L.header_constant("RADNET_CRC32_GRAIN") == CC.GRAIN and L.header_constant("RADNET_CRC32_SPAN_GRAINS") == CC.SPAN_GRAINS
    assert png.CRC_SEGMENT == CC.SEGMENT and png.CRC_SEGMENT.itemsize == 24
    for name in ("radnet_crc32_shift", "radnet_crc32_combine", "radnet_crc32_plan_segments", "radnet_crc32_segments"):
        assert name in L.declared_symbols()
    assert CC.DEEP <= 2 << 20 and CC.cut(0, CC.DEEP)[1] > CC.SPAN_GRAINS


def test_the_model_equals_zlib_on_every_case():
    for name, kind, length, init, at in CASES:
        data = CC.content(kind, length)
        assert CC.model(data, init, at) == zlib.crc32(data.tobytes(), init), name


@pytest.mark.parametrize("mutant", CC.MUTANTS)
def test_every_mutant_is_caught_by_its_case(mutant):
    name, kind, length, init, at = BY_NAME[CC.CAUGHT_BY[mutant]]
    data = CC.content(kind, length)
    assert CC.model(data, init, at) == zlib.crc32(data.tobytes(), init)
    assert CC.model(data, init, at, mutant=mutant) != zlib.crc32(data.tobytes(), init)


LENGTHS = sorted({0, 1} | {(1 << k) + d for k in range(1, 41) for d in (-1, 0, 1)})


def test_shift_equals_the_model():
    for n in LENGTHS:
        assert L.crc32_shift(n) == CC.shift(n), n
    assert L.crc32_shift(0) == L.crc32_shift(-5) == CC.ONE and L.crc32_shift(1) == CC.X8


def test_combine_equals_the_model_and_the_python_operator():
    rng = np.random.RandomState(5)
    for n in LENGTHS:
        c1, c2 = (int(v) for v in rng.randint(0, 1 << 32, size=2, dtype=np.uint64))
        want = png.crc32_combine(c1, c2, n)
        assert L.crc32_combine(c1, c2, n) == want, n
        assert (CC.times_int(c1, CC.shift(n)) ^ c2 if n else c1) == want, n
    a, b = rng.bytes(1000), rng.bytes(777)
    assert L.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)
    assert L.crc32_combine(zlib.crc32(a), zlib.crc32(b""), 0) == zlib.crc32(a)


def test_the_plan_equals_the_model():
    rng = np.random.RandomState(6)
    n = 3 * CC.SPAN * CC.SPAN_GRAINS
    for at in (0, 1, 7, 15):
        table = np.zeros(64, CC.SEGMENT)
        table["offset"] = rng.randint(0, n // 2, size=64)
        table["length"] = rng.randint(0, n // 2, size=64)
        table["length"][:8] = [0, 1, 15, 16, 17, CC.SPAN - 1, CC.SPAN, CC.SPAN + 1]
        rc, spans, ws_bytes, bad, msg = L.crc32_plan_segments(table, n, at)
        assert (rc, bad, msg) == (0, -1, "")
        assert spans == sum(CC.cut(at + int(s["offset"]), int(s["length"]))[1] for s in table)
        assert ws_bytes == 4 * (64 + 1 + spans)
    assert L.crc32_plan_segments(None, 0, 0)[:3] == (0, 0, 4)


def test_the_plan_refuses():
    one = np.zeros(1, CC.SEGMENT)
    for field, value, n in (("offset", -1, 10), ("length", -1, 10), ("offset", 11, 10), ("length", 11, 10)):
        t = one.copy()
        t[field] = value
        rc, _, _, bad, msg = L.crc32_plan_segments(t, n)
        assert (rc, bad) == (ERR_ARG, 0) and "segment 0" in msg
    t = one.copy()
    t[0] = (5, 6, 0, 0)
    assert L.crc32_plan_segments(t, 10)[0] == ERR_ARG and L.crc32_plan_segments(t, 11)[0] == 0
    big = (1 << 63) - 1
    t[0] = (big, big, 0, 0)                         # offset + length leaves 64 bits
    assert L.crc32_plan_segments(t, big)[0] == ERR_ARG
    t[0] = (0, big, 0, 0)
    assert L.crc32_plan_segments(t, big)[0] == ERR_UNSUPPORTED
    for kw in (dict(n=-1), dict(n=10, misalign=16), dict(n=10, misalign=-1), dict(n=10, count=-1)):
        rc, _, _, bad, msg = L.crc32_plan_segments(one, **kw)
        assert (rc, bad) == (ERR_ARG, -1) and msg
    assert L.crc32_plan_segments(None, 10, count=3)[0] == ERR_ARG


def files():
    """(name, file bytes, the idat_sizes asked for): chunks of 0 bytes, of 1 byte and a large one among them."""
    rng = np.random.RandomState(11)
    out = []
    s = png_cases.draw(rng, 40, 50, 2, 8)
    out.append(("rgb_one_idat", png_cases.encode(s, 2, 8, filters="adaptive").data))
    out.append(("rgb_many_idat", png_cases.encode(s, 2, 8, filters=rng, idat_sizes=[1, 0, 7, 3000, 0, 1, 16]).data))
    pal = rng.randint(0, 256, size=(200, 3))
    s = rng.randint(0, 200, size=(33, 70, 1))
    out.append(("palette_zero_first", png_cases.encode(s, 3, 8, filters=1, palette=pal, idat_sizes=[0, 1, 1, 500]).data))
    return out


def chunks_of(data):
    pos, out = 8, []
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        out.append((kind, pos, pos + 8 + length))
        pos += 12 + length
    return out


@pytest.mark.parametrize("name,data", files())
def test_parse_compressed_builds_the_segment_table(name, data):
    ref = png.parse_compressed(data)
    assert ref.crc_segments is None and ref.staged.numel() == ref.n + 768
    comp = png.parse_compressed(data, crc="device")
    idat = [(at, end) for kind, at, end in chunks_of(data) if kind == b"IDAT"]
    table = comp.crc_segments
    assert table.dtype == png.CRC_SEGMENT and len(table) == len(idat)
    assert (0 in table["length"]) == (name != "rgb_one_idat")
    assert (comp.n, comp.header, comp.passes, comp.bpp, comp.expected) == (ref.n, ref.header, ref.passes, ref.bpp, ref.expected)
    assert np.array_equal(comp.palette, ref.palette)
    joined = comp.staged.numpy()[:comp.n].tobytes()
    assert joined == ref.staged.numpy()[:ref.n].tobytes() == b"".join(data[at + 8:end] for at, end in idat)
    at_joined = 0
    for row, (at, end) in zip(table, idat):
        assert (int(row["offset"]), int(row["length"]), int(row["init"])) == (at_joined, end - at - 8, zlib.crc32(b"IDAT"))
        assert int(row["expect"]) == struct.unpack(">I", data[end:end + 4])[0]
        assert zlib.crc32(joined[at_joined:at_joined + end - at - 8], int(row["init"])) == int(row["expect"])
        at_joined += end - at - 8
    table_at, sums_at, result_at, total = png.crc_layout(comp.n, len(idat))
    staged = comp.staged.numpy()
    assert table_at % 8 == 0 and total == len(staged) and staged[comp.n:comp.n + 768].tobytes() == comp.palette.tobytes()
    assert staged[table_at:sums_at].tobytes() == table.tobytes() and not staged[sums_at:].any()


def flip(data, at):
    out = bytearray(data)
    out[at] ^= 0x10
    return bytes(out)


def test_a_corrupt_plte_crc_still_raises_on_the_host_and_a_corrupt_idat_crc_does_not():
    data = dict(files())["palette_zero_first"]
    where = {kind: (at, end) for kind, at, end in chunks_of(data) if kind != b"IDAT"}
    bad_plte = flip(data, where[b"PLTE"][1] + 2)
    for mode in png.CRC_MODES:
        with pytest.raises(ValueError, match="CRC mismatch in the b'PLTE' chunk"):
            png.parse_compressed(bad_plte, crc=mode)
    idat = [(at, end) for kind, at, end in chunks_of(data) if kind == b"IDAT"]
    for bad in (flip(data, idat[3][1] + 1), flip(data, idat[3][0] + 8 + 100), flip(data, idat[0][1])):      # a CRC field, a payload byte, an empty chunk's CRC
        with pytest.raises(ValueError, match="CRC mismatch in the b'IDAT' chunk"):
            png.parse_compressed(bad)
        comp = png.parse_compressed(bad, crc="device")
        sums = [zlib.crc32(comp.staged.numpy()[int(r["offset"]):int(r["offset"] + r["length"])].tobytes(), int(r["init"])) for r in comp.crc_segments]
        assert sum(s != int(r["expect"]) for s, r in zip(sums, comp.crc_segments)) == 1


def test_assemble_pieces_takes_the_running_value():
    rng = np.random.RandomState(12)
    for size in (1, 5, 70000):
        packed = rng.bytes(size)
        running = zlib.crc32(packed, zlib.crc32(b"IDAT" + png._zlib_header(1)))
        want = png.assemble_pieces(packed, 0x12345678, 31, 17, 2)
        assert png.assemble_pieces(packed, 0x12345678, 31, 17, 2, idat_crc=running) == want
        assert png.assemble_pieces(packed, 0x12345678, 31, 17, 2, idat_crc=None) == want
        assert png.assemble_pieces(packed, 0x12345678, 31, 17, 2, idat_crc=running ^ 1) != want
    for bad in (-1, 1 << 32):
        with pytest.raises(ValueError, match="running CRC-32"):
            png.assemble_pieces(b"x", 1, 1, 1, 0, idat_crc=bad)


def test_the_options_are_checked_before_any_device_work():
    img = np.zeros((4, 5, 3), np.uint8)
    data = files()[0][1]
    with pytest.raises(ValueError, match="crc='disk'"):
        png.encode_device(img, crc="disk")
    with pytest.raises(ValueError, match="cannot be set with deflate=\"host\""):
        png.encode_device(img, crc="device")
    with pytest.raises(ValueError, match="crc='disk'"):
        png.decode_device(data, crc="disk")
    with pytest.raises(ValueError, match="not inflate=\"host\""):
        png.decode_device(data, crc="device")
    with pytest.raises(ValueError, match="crc='disk'"):
        png.parse_compressed(data, crc="disk")
    with pytest.raises(ValueError, match="crc='disk'"):
        utils_io.DeviceImageLoader(crc="disk")
    with pytest.raises(ValueError, match="not inflate=\"host\""):
        utils_io.DeviceImageLoader(crc="device")
    loader = utils_io.DeviceImageLoader(inflate="device-lz", crc="device")
    assert (loader.inflate, loader.crc, loader.unfilter) == ("device-lz", "device", "band")
    from faster_rcnn.RADNet import RADNet
    assert RADNet.png_crc == "host"
