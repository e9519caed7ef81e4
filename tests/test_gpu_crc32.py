"""CRC-32 on the device: radnet_crc32_segments through the C ABI (csrc/crc32.hip) against zlib.crc32 on the cases of
tests/crc32_cases.py -- every buffer between sentinels, the input, the bytes behind the sums and behind the result compared after
the call --, tables of thousands of segments, the refusals; then png.crc32_device and crc="device" of png.encode_device and
png.decode_device against the defaults, byte for byte, good files and corrupt ones."""
import struct
import zlib

import numpy as np
import pytest

import crc32_cases as CC
import png_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5
ERR_ARG = -1
GUARD = 64                       # sentinel bytes in front of and behind every buffer


@pytest.fixture(scope="module")
def png():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from faster_rcnn import png
    return png


@pytest.fixture(scope="module")
def ctx(png):
    from radnet_hip import runtime as rt
    return rt.default_context()


def guarded(payload, at=0):
    """`payload` between sentinels in device memory, its first byte `at` bytes behind a 16-byte boundary: (tensor, offset of the payload)."""
    host = np.full(GUARD + 16 + len(payload) + GUARD, SENTINEL, np.uint8)
    dev = torch.from_numpy(host).cuda()
    start = GUARD + (at - (dev.data_ptr() + GUARD)) % 16
    host[start:start + len(payload)] = payload
    dev.copy_(torch.from_numpy(host))
    return dev, start, host


def run(ctx, data, table, at=0, count=None, handle=True, null=()):
    """One call on `data` (uint8 array) and `table` (CC.SEGMENT rows): (rc, message, sums, result, True when nothing but the sums and
    the result was written).  null: names among buf, host, dev, crc, result passed as null pointers."""
    count = len(table) if count is None else count
    buf, start, buf_host = guarded(data, at)
    assert (buf.data_ptr() + start) % 16 == at
    rows = max(len(table), 1)
    table_host = np.zeros(rows, CC.SEGMENT)
    table_host[:len(table)] = table
    table_dev, t0, table_was = guarded(table_host.view(np.uint8))
    out, o0, out_was = guarded(np.full(4 * rows + 8, SENTINEL, np.uint8))      # the sums, then the result: sentinels until written
    assert (table_dev.data_ptr() + t0) % 8 == 0 and (out.data_ptr() + o0) % 4 == 0
    ptr = dict(buf=buf.data_ptr() + start, host=table_host.ctypes.data, dev=table_dev.data_ptr() + t0, crc=out.data_ptr() + o0,
               result=out.data_ptr() + o0 + 4 * rows)
    for name in null:
        ptr[name] = None
    rc = ctx.lib.radnet_crc32_segments(ctx.h if handle else None, ptr["buf"], len(data), ptr["host"], ptr["dev"], count, ptr["crc"], ptr["result"])
    msg = ctx.lib.radnet_last_error(ctx.h)
    ctx.sync()
    got = out.cpu().numpy()
    written = np.zeros(len(got), bool)
    if rc == 0:
        written[o0:o0 + 4 * count] = True
        written[o0 + 4 * rows:o0 + 4 * rows + 8] = True
    clean = (np.array_equal(buf.cpu().numpy(), buf_host) and np.array_equal(table_dev.cpu().numpy(), table_was)
             and np.array_equal(got[~written], out_was[~written]))
    sums = got[o0:o0 + 4 * count].view(np.uint32).copy() if rc == 0 else None
    result = got[o0 + 4 * rows:o0 + 4 * rows + 8].view(np.int32).tolist() if rc == 0 else None
    return rc, (msg.decode() if msg else ""), sums, result, clean


def one(kind, length, init, expect=None):
    data = CC.content(kind, length)
    want = zlib.crc32(data.tobytes(), init)
    return data, np.array([(0, length, init, want if expect is None else expect)], CC.SEGMENT), want


CASES = CC.cases()
GROUPS = dict(small=lambda c: c[2] in CC.SMALL and c[4] == 0, misaligned=lambda c: c[4] != 0 and c[2] != CC.DEEP,
              edges=lambda c: c[2] in CC.EDGES and c[4] == 0, deep=lambda c: c[2] == CC.DEEP)


@pytest.mark.parametrize("group", ["small", "misaligned", "edges", "deep"])
def test_single_segments_equal_zlib(ctx, group):
    """Lengths round the grain, the span and through Horner's rule; every content and init; base pointers 1, 3, 7 and 13 bytes off a
    16-byte boundary.  Nothing but the sum and the result is written."""
    chosen = [c for c in CASES if GROUPS[group](c)]
    assert len(chosen) >= 6 and sum(len([c for c in CASES if pick(c)]) for pick in GROUPS.values()) == len(CASES)      # the groups are the whole table
    for name, kind, length, init, at in chosen:
        data, table, want = one(kind, length, init)
        rc, msg, sums, result, clean = run(ctx, data, table, at)
        assert rc == 0, (name, msg)
        assert int(sums[0]) == want, (name, hex(int(sums[0])), hex(want))
        assert result == [1, 0] and clean, (name, result, clean)


def test_the_mutants_cases_run_on_the_device(ctx):
    """The cases that tell the model's five mutants from zlib.crc32 are among those above; here by name, so that a renamed case shows."""
    by_name = {c[0]: c for c in CASES}
    for mutant in CC.MUTANTS:
        name, kind, length, init, at = by_name[CC.CAUGHT_BY[mutant]]
        data, table, want = one(kind, length, init)
        rc, msg, sums, result, clean = run(ctx, data, table, at)
        assert rc == 0 and int(sums[0]) == want and want != CC.model(data, init, at, mutant=mutant), (mutant, name)


def table_sums(data, table):
    return np.array([zlib.crc32(data[int(s["offset"]):int(s["offset"] + s["length"])].tobytes(), int(s["init"])) for s in table], np.uint32)


def test_three_thousand_small_segments_in_shuffled_order(ctx):
    rs = np.random.RandomState(21)
    data = rs.randint(0, 256, size=50000).astype(np.uint8)
    table = np.zeros(3000, CC.SEGMENT)
    table["length"] = rs.randint(0, 41, size=3000)
    table["length"][:41] = np.arange(41)
    at = np.concatenate([[0], np.cumsum(table["length"][:1499])])               # 1500 adjacent ones ...
    table["offset"][:1500] = at
    table["offset"][1500:] = rs.randint(0, 50000 - 40, size=1500)                # ... and 1500 anywhere: overlapping
    table["init"] = rs.randint(0, 1 << 32, size=3000, dtype=np.uint64)
    table["init"][::3] = CC.IDAT
    table = table[rs.permutation(3000)]
    want = table_sums(data, table)
    table["expect"] = want
    for at in (0, 5):
        rc, msg, sums, result, clean = run(ctx, data, table, at)
        assert rc == 0, msg
        bad = np.flatnonzero(sums != want)
        assert bad.size == 0, (at, bad[:8].tolist(), table[bad[:3]].tolist())
        assert result == [3000, 0] and clean


def test_one_long_segment_between_tiny_ones_and_the_result_words(ctx):
    rs = np.random.RandomState(22)
    data = rs.randint(0, 256, size=(2 << 20) + 300).astype(np.uint8)
    table = np.zeros(9, CC.SEGMENT)
    table["offset"] = [0, 7, 30, 100, 100, 150, (2 << 20) + 250, 0, (2 << 20) + 300]
    table["length"] = [7, 20, 0, 2 << 20, 50, 4100, 50, 1, 0]
    table["init"] = rs.randint(0, 1 << 32, size=9, dtype=np.uint64)
    want = table_sums(data, table)
    table["expect"] = want
    rc, msg, sums, result, clean = run(ctx, data, table, 3)
    assert rc == 0 and np.array_equal(sums, want) and result == [9, 0] and clean, (msg, result)
    # one bad segment; several (the smallest index and the count); all of them
    for bad in ([3], [6, 2, 8], list(range(9))):
        t = table.copy()
        t["expect"][bad] ^= 0x00010000
        rc, msg, sums, result, clean = run(ctx, data, t, 3)
        assert rc == 0 and np.array_equal(sums, want) and result == [min(bad), len(bad)] and clean, (bad, result)


def test_an_empty_table(ctx):
    data = np.arange(40, dtype=np.uint8)
    rc, msg, sums, result, clean = run(ctx, data, np.zeros(0, CC.SEGMENT))
    assert (rc, result, clean) == (0, [0, 0], True), msg
    rc, msg, sums, result, clean = run(ctx, data, np.zeros(0, CC.SEGMENT), null=("host", "dev", "crc"))
    assert (rc, result, clean) == (0, [0, 0], True), msg
    rc, msg, sums, result, clean = run(ctx, np.zeros(0, np.uint8), np.zeros(1, CC.SEGMENT), null=("buf",))       # an empty buffer: its one empty segment
    assert (rc, result, clean) == (0, [1, 0], True) and int(sums[0]) == 0 == zlib.crc32(b""), msg


def test_refusals_launch_nothing(ctx):
    data = np.arange(200, dtype=np.uint8)
    good = np.array([(0, 200, 0, 0), (10, 20, 1, 2)], CC.SEGMENT)

    def refused(table=good, want=ERR_ARG, say="crc32_segments", **kw):
        rc, msg, sums, result, clean = run(ctx, data, table, **kw)
        assert rc == want and clean, (rc, msg, kw)
        assert say in msg, msg
    for name in ("buf", "host", "dev", "crc", "result"):
        refused(null=(name,), say="null pointer")
    refused(count=-1, say="-1 segments")
    for row, field, value in ((1, "offset", -1), (1, "length", -1), (1, "offset", 201), (1, "length", 191), (0, "length", 201),
                              (1, "offset", (1 << 63) - 1), (1, "length", (1 << 63) - 1)):
        t = good.copy()
        t[field][row] = value
        refused(t, say="segment %d" % row)
    rc, msg, sums, result, clean = run(ctx, data, good, handle=False)
    assert rc == ERR_ARG and clean
    # odd addresses for the device table, the sums and the result
    buf, table_dev, out = torch.from_numpy(data).cuda(), torch.from_numpy(np.concatenate([good.view(np.uint8), np.zeros(8, np.uint8)])).cuda(), torch.zeros(32, dtype=torch.uint8, device="cuda")
    for dt, dc, dr in ((4, 0, 8), (0, 2, 8), (0, 0, 9)):
        rc = ctx.lib.radnet_crc32_segments(ctx.h, buf.data_ptr(), 200, good.ctypes.data, table_dev.data_ptr() + dt, 2, out.data_ptr() + dc, out.data_ptr() + dr)
        assert rc == ERR_ARG and b"aligned" in ctx.lib.radnet_last_error(ctx.h)
    ctx.sync()
    assert not out.cpu().numpy().any()
    rc, msg, sums, result, clean = run(ctx, data, good)                   # and the context still works
    assert rc == 0 and np.array_equal(sums, table_sums(data, good)) and result == [0, 2]


def test_crc32_device_equals_zlib(png):
    rs = np.random.RandomState(23)
    for n in (0, 1, 16, 4095, 70001):
        host = rs.randint(0, 256, size=n + 3).astype(np.uint8)
        t = torch.from_numpy(host).cuda()
        assert png.crc32_device(t[:n]) == zlib.crc32(host[:n].tobytes())
        assert png.crc32_device(t[3:], 0xDEADBEEF) == zlib.crc32(host[3:].tobytes(), 0xDEADBEEF)        # a view: an odd base address
    with pytest.raises(TypeError):
        png.crc32_device(torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(TypeError):
        png.crc32_device(torch.zeros((4, 4), dtype=torch.uint8, device="cuda")[:, 1])
    with pytest.raises(ValueError):
        png.crc32_device(torch.zeros(4, dtype=torch.uint8, device="cuda"), -1)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_the_writer_gives_the_same_file(png):
    rs = np.random.RandomState(24)
    for shape in ((37, 53, 3), (41, 29)):
        img = torch.from_numpy(rs.randint(0, 4, size=shape).astype(np.uint8) * 60).cuda()
        for kw in (dict(), dict(huffman="fixed"), dict(filter="none")):
            want = png.encode_device(img, deflate="device", **kw)
            assert png.encode_device(img, deflate="device", crc="host", **kw) == want
            got = png.encode_device(img, deflate="device", crc="device", **kw)
            assert got == want, (shape, kw)
        assert torch.equal(png.decode_device(got), img if img.dim() == 3 else img[:, :, None].expand(-1, -1, 3))
    with pytest.raises(ValueError, match="cannot be set with deflate=\"host\""):
        png.encode_device(img, crc="device")


def recompressed(data, idat_sizes=(), rle=True):
    """The PNG file `data` with its IDAT stream compressed again -- rle: as a run-length stream (level 1, Z_RLE), else at level 6 --
    and cut into IDAT chunks of idat_sizes and the rest."""
    pos, parts, idat = 8, [K.SIGNATURE], b""
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + length]
        elif kind == b"IEND":
            c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE) if rle else zlib.compressobj(6)
            z = c.compress(zlib.decompress(idat)) + c.flush()
            for size in idat_sizes:
                parts.append(K.chunk(b"IDAT", z[:size]))
                z = z[size:]
            parts += [K.chunk(b"IDAT", z), K.chunk(b"IEND")]
        else:
            parts.append(data[pos:pos + 12 + length])
        pos += 12 + length
    return b"".join(parts)


def idat_chunks(data):
    pos, out = 8, []
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            out.append((pos + 8, pos + 8 + length))
        pos += 12 + length
    return out


def outcome(f):
    try:
        return "image", f().cpu().numpy()
    except ValueError as e:
        return "ValueError", str(e)


@pytest.fixture(scope="module")
def read_files():
    rs = np.random.RandomState(25)
    rgb = K.encode(K.draw(rs, 60, 70, 2, 8, "low"), 2, 8, filters="adaptive").data
    pal = rs.randint(0, 256, size=(16, 3))
    indexed = K.encode(rs.randint(0, 16, size=(45, 64, 1)), 3, 4, filters=rs, palette=pal).data
    return {"one idat": (rgb, ()), "many idat": (rgb, (100, 1, 300, 7, 50)), "a zero-length idat": (indexed, (0, 20, 0, 1)),
            "zero-length first and 8-byte ones": (rgb, (0,) + (8,) * 40)}


@pytest.mark.parametrize("inflate", ["device", "device-lz"])
@pytest.mark.parametrize("name", ["one idat", "many idat", "a zero-length idat", "zero-length first and 8-byte ones"])
def test_the_reader_gives_the_same_image_and_the_same_errors(png, read_files, inflate, name):
    source, sizes = read_files[name]
    data = recompressed(source, sizes, rle=inflate == "device")
    chunks = idat_chunks(data)
    assert len(chunks) == len(sizes) + 1 and (0 in sizes) == (0 in [e - s for s, e in chunks])
    want = png.decode_device(data)
    plain = {}
    assert torch.equal(png.decode_device(data, inflate=inflate, report=plain), want) and "crc" not in plain and plain["path"] == "device"
    for unfilter in ("band", "tiles"):
        report = {}
        got = png.decode_device(data, inflate=inflate, crc="device", unfilter=unfilter, report=report)
        assert torch.equal(got, want), (name, unfilter, report)
        assert report["path"] == "device" and report["crc"] == "device" and report["reason"] is None, report
    # one flipped payload byte, one flipped CRC field: in the largest chunk and in the first one (which may be empty)
    big = max(range(len(chunks)), key=lambda k: chunks[k][1] - chunks[k][0])
    spoiled = [(big, chunks[big][0] + (chunks[big][1] - chunks[big][0]) // 2), (big, chunks[big][1] + 3), (0, chunks[0][1])]
    for k, at in spoiled:
        bad = bytearray(data)
        bad[at] ^= 0x04
        bad = bytes(bad)
        expected = outcome(lambda: png.decode_device(bad))
        assert expected[0] == "ValueError" and "CRC mismatch in the b'IDAT' chunk" in expected[1]
        report = {}
        assert outcome(lambda: png.decode_device(bad, inflate=inflate, crc="device", report=report)) == expected
        assert report["path"] == "host" and report["crc"] == "host" and report["reason"] == "crc: IDAT chunk %d" % k, (name, k, report)
    with pytest.raises(ValueError, match="not inflate=\"host\""):
        png.decode_device(data, crc="device")


def test_get_image_and_the_loader_pass_the_option_on(png, tmp_path, monkeypatch):
    from faster_rcnn import utils_io
    rs = np.random.RandomState(26)
    data = recompressed(K.encode(K.draw(rs, 30, 40, 2, 8, "low"), 2, 8, filters="adaptive").data, (5, 0, 9))
    (tmp_path / "maps" / "grey").mkdir(parents=True)
    (tmp_path / "maps" / "grey" / "scan.png").write_bytes(data)
    monkeypatch.chdir(tmp_path)
    want = png.decode_device(data)
    path = "maps/scan.png"                                                # image_path: maps/<type>/scan.png
    got = utils_io.get_image(path, ["grey"], to_host=False, inflate="device", crc="device")
    assert torch.equal(got, want)
    assert np.array_equal(utils_io.get_image(path, ["grey"], inflate="device-lz", crc="device"), want.cpu().numpy())
    with pytest.raises(ValueError, match="not inflate=\"host\""):
        utils_io.get_image(path, ["grey"], crc="device")
    loader = utils_io.DeviceImageLoader(inflate="device", crc="device")
    assert torch.equal(loader(dict(filepath=path), "grey"), want) and loader.misses == 1
