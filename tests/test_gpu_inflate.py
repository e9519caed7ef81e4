"""The device inflate against its Python model (tests/inflate_cases.py) over whole sentinel-prefilled buffers: the candidate sets of
radnet_inflate_find_blocks, the unit records of radnet_inflate_rle_measure and the bytes of radnet_inflate_rle_emit with the sentinels
behind them, the stream at misaligned device addresses; a small cand_cap; what the entries refuse; png.decode_device(inflate="device")
byte for byte against the default on every colour type and depth, with report["path"] == "device" asserted (a test that passes
through the fallback proves nothing); the fallbacks with their reasons and the default path's result or exception; get_image and
predict_from_path."""
import copy
import os
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as I
import png_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5
ERR_ARG, ERR_UNSUPPORTED = -1, -3
NAMES = sorted(I.cases())


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


def last_error(ctx):
    msg = ctx.lib.radnet_last_error(ctx.h)
    return msg.decode() if msg else ""


def upload(data, offset=0):
    """(buffer, pointer): the bytes on the device at `offset` of an allocation, sentinels round them."""
    buf = torch.full((offset + len(data) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    buf[offset:offset + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    return buf, buf.data_ptr() + offset


def find(ctx, z, ptr, cap, first_bit=16):
    """(rc, count, the candidates kept, in the order they were appended): nothing behind the cap or the count may be written."""
    cand = torch.full((cap + 8,), -1, dtype=torch.int32, device="cuda")
    count = torch.tensor([0, -1], dtype=torch.int32, device="cuda")
    rc = ctx.lib.radnet_inflate_find_blocks(ctx.h, ptr, len(z), first_bit, cand.data_ptr(), cap, count.data_ptr())
    ctx.sync()
    c, n = cand.cpu().numpy(), count.cpu().numpy()
    assert n[1] == -1 and (c[cap:] == -1).all(), "written behind the count or the cap"
    kept = min(int(n[0]), cap)
    assert (c[kept:] == -1).all(), "written behind the candidates"
    return rc, int(n[0]), c[:kept].view(np.uint32).tolist()


def measure(ctx, png, z, ptr, starts):
    """(rc, the records as tuples): one sentinel record stands behind the table."""
    table = np.zeros(len(starts) + 1, png.INFLATE_UNIT)
    table.view(np.uint8)[:] = SENTINEL
    table["start_bit"][:len(starts)] = starts
    dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    rc = ctx.lib.radnet_inflate_rle_measure(ctx.h, ptr, len(z), dev.data_ptr(), len(starts))
    ctx.sync()
    got = dev.cpu().numpy().view(png.INFLATE_UNIT)
    assert (got[len(starts):].view(np.uint8) == SENTINEL).all(), "written behind the unit table"
    return rc, [tuple(int(v) for v in u) for u in got[:len(starts)]]


def emit(ctx, png, z, ptr, links, out_len, table_len=None):
    """(rc, the output buffer's bytes): out_len bytes and 64 sentinels behind them, all prefilled."""
    table = np.zeros(len(links), png.INFLATE_LINK)
    for k, (offset, start, out_bytes, prev) in enumerate(links):
        table[k] = (offset, start, out_bytes, prev, 0)
    dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    out = torch.full((out_len + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = ctx.lib.radnet_inflate_rle_emit(ctx.h, ptr, len(z), dev.data_ptr(), len(links), out.data_ptr(), out_len if table_len is None else table_len)
    ctx.sync()
    return rc, bytes(out.cpu().numpy())


# ---- the three kernels against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_find_measure_and_emit_match_the_model(ctx, png, name):
    c = I.cases()[name]
    cands, starts, units = I.model_units(name)
    offset = 1 + 2 * (NAMES.index(name) % 4)                           # 1, 3, 5, 7 bytes off an aligned address
    buf, ptr = upload(c.z, offset)
    rc, count, got = find(ctx, c.z, ptr, len(cands) + 8)
    assert rc == 0, last_error(ctx)
    assert count == len(cands) and sorted(got) == cands, (name, count, len(cands))
    rc, records = measure(ctx, png, c.z, ptr, starts)
    assert rc == 0, last_error(ctx)
    for got_u, want_u in zip(records, units):
        assert got_u == want_u, (name, dict(zip(I.UNIT_FIELDS, got_u)), dict(zip(I.UNIT_FIELDS, want_u)))
    code, bad, links, false_count = I.chain(units, 16, len(c.z), c.expected)
    assert (code == I.CHAIN_OK) == (c.reason in (None, "adler")) or c.corrupt, name
    if code == I.CHAIN_OK:
        want = I.emit(c.z, links, c.expected, fill=SENTINEL) + bytes([SENTINEL]) * 64
        rc, out = emit(ctx, png, c.z, ptr, links, c.expected)
        assert rc == 0, last_error(ctx)
        assert out == want, (name, "first difference at byte %d" % next(i for i in range(len(want)) if out[i] != want[i]))
        if c.reason is None and not c.corrupt:
            assert out[:c.expected] == c.data
        # a short output cuts the units there and nothing is written behind it
        short = c.expected - min(c.expected, 5)
        rc, out = emit(ctx, png, c.z, ptr, links, c.expected, table_len=short)
        assert rc == 0 and out == want[:short] + bytes([SENTINEL]) * (len(want) - short), name
    assert bytes(buf.cpu().numpy()[offset:offset + len(c.z)]) == c.z, "the stream was written"


def test_units_entered_anywhere_measure_like_the_model(ctx, png):
    """Starts that are no block starts at all -- every 997th bit of the cv2-like stream and the bits round its end: garbage decodes to
    the model's status, whatever it is."""
    z = I.cases()["a cv2-like"].z
    starts = sorted(set(range(16, 8 * len(z), 997)) | set(range(8 * len(z) - 40, 8 * len(z))))
    buf, ptr = upload(z, 3)
    rc, records = measure(ctx, png, z, ptr, starts)
    assert rc == 0, last_error(ctx)
    want = I.measure(z, starts)
    assert records == want, [(dict(zip(I.UNIT_FIELDS, g)), dict(zip(I.UNIT_FIELDS, w))) for g, w in zip(records, want) if g != w][:3]
    assert len({u[5] for u in want}) >= 3, "several statuses are met"


def test_a_small_cand_cap_is_reported_through_the_count(ctx):
    c = I.cases()["b memlevel 1"]
    cands = I.model_units("b memlevel 1")[0]
    buf, ptr = upload(c.z, 5)
    for cap in (10, 1, 0):
        rc, count, got = find(ctx, c.z, ptr, cap)
        assert rc == 0 and count == len(cands) > 100 and len(got) == cap and set(got) <= set(cands) and len(set(got)) == cap, cap


def test_find_blocks_from_a_later_first_bit(ctx):
    c = I.cases()["c flushes"]
    cands = I.model_units("c flushes")[0]
    buf, ptr = upload(c.z)
    rc, count, got = find(ctx, c.z, ptr, 64, first_bit=cands[2] + 1)
    assert rc == 0 and sorted(got) == cands[3:] == I.find_blocks(c.z, cands[2] + 1)


def test_refused_arguments_leave_the_buffers_untouched(ctx, png):
    lib = ctx.lib
    z = I.cases()["f 300 bytes"].z
    n = len(z)
    buf, ptr = upload(z)
    cand = torch.full((8,), -1, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    for what, args, code in (("null stream", (None, n, 16, cand.data_ptr(), 8, count.data_ptr()), ERR_ARG), ("n = 2", (ptr, 2, 16, cand.data_ptr(), 8, count.data_ptr()), ERR_ARG),
                             ("null candidates", (ptr, n, 16, None, 8, count.data_ptr()), ERR_ARG), ("null count", (ptr, n, 16, cand.data_ptr(), 8, None), ERR_ARG),
                             ("a negative cap", (ptr, n, 16, cand.data_ptr(), -1, count.data_ptr()), ERR_ARG),
                             ("a negative first bit", (ptr, n, -1, cand.data_ptr(), 8, count.data_ptr()), ERR_ARG),
                             ("first bit = 8 n", (ptr, n, 8 * n, cand.data_ptr(), 8, count.data_ptr()), ERR_ARG),
                             ("n = 2^29", (ptr, 1 << 29, 16, cand.data_ptr(), 8, count.data_ptr()), ERR_UNSUPPORTED)):
        assert lib.radnet_inflate_find_blocks(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_inflate_find_blocks(None, ptr, n, 16, cand.data_ptr(), 8, count.data_ptr()) == ERR_ARG
    units = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    for what, args, code in (("null stream", (None, n, units.data_ptr(), 1), ERR_ARG), ("null table", (ptr, n, None, 1), ERR_ARG), ("no units", (ptr, n, units.data_ptr(), 0), ERR_ARG),
                             ("n = 0", (ptr, 0, units.data_ptr(), 1), ERR_ARG), ("n = 2^29", (ptr, 1 << 29, units.data_ptr(), 1), ERR_UNSUPPORTED)):
        assert lib.radnet_inflate_rle_measure(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_inflate_rle_measure(None, ptr, n, units.data_ptr(), 1) == ERR_ARG
    links = torch.zeros((24,), dtype=torch.uint8, device="cuda")
    out = torch.full((512,), SENTINEL, dtype=torch.uint8, device="cuda")
    for what, args, code in (("null stream", (None, n, links.data_ptr(), 1, out.data_ptr(), 300), ERR_ARG), ("null table", (ptr, n, None, 1, out.data_ptr(), 300), ERR_ARG),
                             ("null output", (ptr, n, links.data_ptr(), 1, None, 300), ERR_ARG), ("no units", (ptr, n, links.data_ptr(), 0, out.data_ptr(), 300), ERR_ARG),
                             ("a negative length", (ptr, n, links.data_ptr(), 1, out.data_ptr(), -1), ERR_ARG),
                             ("n = 2^29", (ptr, 1 << 29, links.data_ptr(), 1, out.data_ptr(), 300), ERR_UNSUPPORTED)):
        assert lib.radnet_inflate_rle_emit(ctx.h, *args) == code and last_error(ctx), what
    assert lib.radnet_inflate_rle_emit(None, ptr, n, links.data_ptr(), 1, out.data_ptr(), 300) == ERR_ARG
    column = torch.full((16,), SENTINEL, dtype=torch.uint8, device="cuda")
    offsets, rows, rowbytes = np.array([0], np.int64), np.array([3], np.int32), np.array([99], np.int32)
    good = (out.data_ptr(), 300, offsets.ctypes.data, rows.ctypes.data, rowbytes.ctypes.data, 1, column.data_ptr())
    for what, change, code in (("null stream", {0: None}, ERR_ARG), ("a pass beyond the stream", {1: 299}, ERR_ARG), ("no passes", {5: 0}, ERR_ARG), ("eight passes", {5: 8}, ERR_ARG),
                               ("null column", {6: None}, ERR_ARG)):
        args = tuple(change.get(k, v) for k, v in enumerate(good))
        assert lib.radnet_png_gather_column_u8(ctx.h, *args) == code and last_error(ctx), what
    ctx.sync()
    assert (cand.cpu().numpy() == -1).all() and count.cpu().numpy()[0] == -1 and (units.cpu().numpy() == SENTINEL).all()
    assert (out.cpu().numpy() == SENTINEL).all() and (column.cpu().numpy() == SENTINEL).all()
    out[::100] = torch.tensor([1, 4, 2, 9, 9, 9], dtype=torch.uint8, device="cuda")
    assert lib.radnet_png_gather_column_u8(ctx.h, *good) == 0                                # and the arguments they were derived from pass
    ctx.sync()
    assert column.cpu().numpy().tolist() == [1, 4, 2] + [SENTINEL] * 13


def test_the_column_planner_equals_the_stream_planner(png):
    import ctypes
    from radnet_hip import lib as L
    lib = L.load_library()
    rs = np.random.RandomState(9)
    for rows, rowbytes, target, cap in ((300, 5, 0, 20), (300, 5, 7, 300), (64, 3, 0, 1), (500, 2, 16, 9)):
        column = rs.randint(0, 5, rows).astype(np.uint8)
        stream = np.zeros((rows, 1 + rowbytes), np.uint8)
        stream[:, 0] = column
        a, b = np.zeros(cap, png.SEGMENT), np.zeros(cap, png.SEGMENT)
        na = lib.radnet_png_plan_segments(stream.ctypes.data, 11, rows, rowbytes, target, a.ctypes.data_as(ctypes.c_void_p), cap)
        nb = lib.radnet_png_plan_segments_column(column.ctypes.data, 11, rows, rowbytes, target, b.ctypes.data_as(ctypes.c_void_p), cap)
        assert na == nb > 0 and np.array_equal(a, b) and int(a["rows"].sum()) == rows
    column[5] = 5
    assert lib.radnet_png_plan_segments_column(column.ctypes.data, 0, rows, rowbytes, 0, b.ctypes.data_as(ctypes.c_void_p), cap) == ERR_ARG


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def rle_file(data, idat_sizes=(), mem=8):
    """The PNG file `data` with its IDAT stream compressed again as a run-length stream (level 1, Z_RLE), cut into IDAT chunks of
    idat_sizes and the rest."""
    pos, parts, idat, done = 8, [K.SIGNATURE], b"", False
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + length]
        elif kind == b"IEND":
            c = zlib.compressobj(1, zlib.DEFLATED, 15, mem, zlib.Z_RLE)
            z = c.compress(zlib.decompress(idat)) + c.flush()
            for size in idat_sizes:
                parts.append(K.chunk(b"IDAT", z[:size]))
                z = z[size:]
            parts += [K.chunk(b"IDAT", z), K.chunk(b"IEND")]
            done = True
        else:
            parts.append(data[pos:pos + 12 + length])
        pos += 12 + length
    assert done
    return b"".join(parts)


def wrap(z, expected):
    """A one-row 8-bit grey PNG whose IDAT stream is z: 1 + width = expected bytes."""
    return b"".join([K.SIGNATURE, K.ihdr(expected - 1, 1, 8, 0), K.chunk(b"IDAT", z), K.chunk(b"IEND")])


def outcome(f):
    try:
        return "image", f().cpu().numpy()
    except ValueError as e:
        return "ValueError", str(e)


def same_outcome(a, b):
    return a[0] == b[0] and (np.array_equal(a[1], b[1]) if a[0] == "image" else a[1] == b[1])


def test_every_colour_type_and_depth_decodes_on_the_device(png):
    rs = np.random.RandomState(31)
    ways = set()
    files = [(color, depth, interlace, 13, 17, rs) for color, depth in K.LEGAL for interlace in (False, True)]
    files += [(2, 8, False, 200, 40, rs), (0, 8, False, 150, 33, 1), (6, 16, True, 70, 90, "adaptive")]      # passes long enough to be cut into segments
    for color, depth, interlace, h, w, filters in files:
        pal = rs.randint(0, 256, (1 << min(depth, 8), 3)) if color == 3 else None
        samples = K.draw(rs, h, w, color, depth)
        enc = K.encode(samples, color, depth, filters=filters, interlace=interlace, palette=pal)
        data = rle_file(enc.data, idat_sizes=(3, 1, 40) if interlace else ())
        report = {}
        got = png.decode_device(data, inflate="device", report=report)
        want = png.decode_device(data)
        assert report["path"] == "device" and report["reason"] is None, (color, depth, interlace, report)
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got, want), (color, depth, interlace)
        assert np.array_equal(want.cpu().numpy(), K.expand(samples, color, depth, pal)), (color, depth, interlace)
        assert report["units"] >= 1 and report["blocks"] >= report["units"] and report["candidates"] >= report["units"] - 1 and report["false_candidates"] >= 0
        ways.add(report["reconstruction"])
        as_array = png.decode_device(np.frombuffer(data, np.uint8), inflate="device")     # the bytes as np.fromfile gives them
        assert torch.equal(as_array, want)
    assert ways == {"segments", "unfilter"}, ways


def test_many_blocks_and_the_packages_own_writers_decode_on_the_device(png):
    rs = np.random.RandomState(5)
    img = K.draw(rs, 120, 160, 2, 8, "low").astype(np.uint8)
    enc = K.encode(img, 2, 8, filters="adaptive")
    data = rle_file(enc.data, mem=1)                                    # blocks of 128 symbols: hundreds of units, ends on every bit phase
    report = {}
    got = png.decode_device(data, inflate="device", report=report)
    assert report["path"] == "device" and report["units"] > 50 and torch.equal(got, png.decode_device(data)), report
    dev = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
    for kw in (dict(), dict(deflate="device"), dict(deflate="device", huffman="fixed"), dict(chunk_bytes=5000)):
        data = png.encode_device(dev, **kw)
        report = {}
        got = png.decode_device(data, inflate="device", report=report)
        assert report["path"] == "device" and torch.equal(got, dev), (kw, report)


@pytest.mark.parametrize("name", ["h unit cap", "i level 6", "i distance 2", "j flipped bit", "j truncated", "j bytes behind the final block", "j wrong adler",
                                  "k incomplete header"])
def test_what_the_device_cannot_take_goes_to_the_host_path(png, name):
    c = I.cases()[name]
    data = wrap(c.z, c.expected)
    want = outcome(lambda: png.decode_device(data))
    report = {}
    got = outcome(lambda: png.decode_device(data, inflate="device", report=report))
    assert same_outcome(got, want), (name, got[0], want[0], got[1] if got[0] != "image" else "", want[1] if want[0] != "image" else "")
    assert report["path"] == "host" and report["reason"] == I.model(name)[1], (name, report)
    assert report["reason"] == c.reason or c.reason is None
    assert report["units"] == 0 and report["reconstruction"] is None
    assert (want[0] == "image") == (name in ("h unit cap", "i level 6", "i distance 2", "j bytes behind the final block")), (name, want)


def test_other_fallbacks_and_the_default(png):
    rs = np.random.RandomState(8)
    samples = K.draw(rs, 40, 50, 2, 8, "low")                           # four values: level 6 finds matches at every distance
    enc = K.encode(samples, 2, 8, filters=rs)                           # level 6, as other tools write
    report = {}
    got = png.decode_device(enc.data, inflate="device", report=report)
    assert report["path"] == "host" and "not run-length" in report["reason"], report
    assert np.array_equal(got.cpu().numpy(), K.expand(samples, 2, 8))
    report = {}
    want = png.decode_device(enc.data, report=report)                    # the default: the host path, nothing searched
    assert report == dict(path="host", reason=None, candidates=0, false_candidates=0, units=0, blocks=0, reconstruction=None)
    assert torch.equal(want, got) and torch.equal(png.decode_device(enc.data, None, "host"), want)
    # a broken container, a filter type above 4, a zlib header the device path does not take: the default's exception or image
    rle = rle_file(enc.data)
    broken = bytearray(rle)
    broken[len(broken) - 30] ^= 1
    lines = bytearray(enc.stream)
    lines[151 * 3] = 5
    type5 = rle_file(b"".join([K.SIGNATURE, K.ihdr(50, 40, 8, 2), K.chunk(b"IDAT", zlib.compress(bytes(lines))), K.chunk(b"IEND")]))
    c = zlib.compressobj(1, zlib.DEFLATED, 9, 8, zlib.Z_RLE)             # a 512-byte window: still a header the device takes
    small_window = b"".join([K.SIGNATURE, K.ihdr(50, 40, 8, 2), K.chunk(b"IDAT", c.compress(enc.stream) + c.flush()), K.chunk(b"IEND")])
    for what, data, path in (("CRC", bytes(broken), "host"), ("filter type 5", type5, "host"), ("small window", small_window, "device")):
        want = outcome(lambda: png.decode_device(data))
        report = {}
        got = outcome(lambda: png.decode_device(data, inflate="device", report=report))
        assert same_outcome(got, want) and report["path"] == path and (report["reason"] is None) == (path == "device"), (what, report, got[0], want[0])
    with pytest.raises(ValueError, match="inflate="):
        png.decode_device(enc.data, inflate="gpu")


def test_get_image_and_predict_from_path_inflate_on_the_device(png, tmp_path, monkeypatch):
    from faster_rcnn import models as M
    from faster_rcnn import utils_io
    from faster_rcnn.base_models import resnet50 as base
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    from oracle import dense
    Cc = Config()
    Cc.img_size = 300
    ms = M.build_models(Cc, weights=copy.deepcopy(dense.init_params(seed=3)), workload="predict")
    rnet = RADNet(Cc, ms[3], ms[4], base.preprocess)
    Cc.tile_size, Cc.tile_overlap, Cc.include_full_img, Cc.use_img_type = 400, 250, True, False
    Cc.img_types = ["blended_grey"]
    rnet.bbox_threshold, rnet.device_tail, rnet.device_resident = 0.0, True, True
    assert rnet.png_inflate == "host" and RADNet.png_inflate == "host"
    img = np.random.RandomState(41).randint(0, 256, (420, 460, 3)).astype(np.uint8)
    os.makedirs(tmp_path / "blended_grey")
    (tmp_path / "blended_grey" / "scan.png").write_bytes(rle_file(K.encode(img[:, :, ::-1], 2, 8, filters="adaptive").data))
    monkeypatch.chdir(tmp_path.parent)
    rel = tmp_path.name + "/scan.png"
    reports, decode = [], png.decode_device

    def watched(data, ctx=None, inflate="host", report=None):
        report = {} if report is None else report
        reports.append((inflate, report))
        return decode(data, ctx, inflate, report)
    monkeypatch.setattr(png, "decode_device", watched)
    assert np.array_equal(utils_io.get_image(rel, Cc.img_types), img)                                 # the default, as before
    assert [(i, r["path"]) for i, r in reports] == [("host", "host")]
    del reports[:]
    assert np.array_equal(utils_io.get_image(rel, Cc.img_types, inflate="device"), img)
    on_device = utils_io.get_image(rel, Cc.img_types, to_host=False, inflate="device")
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), img)
    assert [(i, r["path"]) for i, r in reports] == [("device", "device")] * 2
    del reports[:]
    want = rnet.predict_from_path(rel)
    assert len(want) > 0 and [(i, r["path"]) for i, r in reports] == [("host", "host")]
    rnet.png_inflate = "device"
    got = rnet.predict_from_path(rel)
    assert [(i, r["path"]) for i, r in reports[1:]] == [("device", "device")]
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert list(x) == list(y) and all(type(x[k]) is type(y[k]) and np.array_equal(x[k], y[k]) for k in x), (x, y)
