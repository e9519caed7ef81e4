"""The tiled PNG reconstruction on the device (radnet_png_unfilter_tiles_u8 through the C ABI, then unfilter="tiles" of
png.decode_device, png.decode_device_many, utils_io.get_image and RADNet.predict_from_path).  The kernel entry runs on raw filtered
streams in sentinel-prefilled buffers, and the whole buffer is compared byte for byte with the raw rows the streams were filtered
from (tests/png_tiles_cases.py, tests/png_cases.py): the data, the untouched filter-type bytes, the untouched bytes in front of,
between and behind the segments.  The decoders are compared with png_cases.expand of the source samples."""
import copy
import os
import struct
import zlib

import numpy as np
import pytest

import png_cases as K
import png_tiles_cases as TC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0xA5


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


def tiles_call(ctx, dev, base_len, table, table_dev, count, bpp, handle=True):
    fn = ctx.lib.radnet_png_unfilter_tiles_u8
    rc = fn(ctx.h if handle else None, dev.data_ptr() if dev is not None else None, base_len, table.ctypes.data if table is not None else None,
            table_dev.data_ptr() if table_dev is not None else None, count, bpp)
    msg = ctx.lib.radnet_last_error(ctx.h)
    return rc, (msg.decode() if msg else "")


def packed(png, rs, shapes, bpp, kind, shuffle=True):
    """One sentinel-prefilled buffer holding a filtered segment per (rows, pixels) of `shapes`, 1 to 7 sentinels in front of, between
    and behind them: (the buffer as uploaded, the buffer as it must come back, the table in shuffled order)."""
    parts, want, segs, at = [], [], [], 0
    for rows, pixels in shapes:
        gap = np.full(int(rs.randint(1, 8)), SENTINEL, np.uint8)
        lines, raw = TC.draw_segment(rs, rows, pixels, bpp, kind)
        done = lines.copy()
        done[:, 1:] = raw                                                  # the filter-type bytes stay
        segs.append((at + gap.size, rows, pixels * bpp))
        parts += [gap, lines.reshape(-1)]
        want += [gap, done.reshape(-1)]
        at += gap.size + lines.size
    tail = np.full(5, SENTINEL, np.uint8)
    table = np.array(segs, png.SEGMENT)
    if shuffle:
        table = table[rs.permutation(len(table))]
    return np.concatenate(parts + [tail]), np.concatenate(want + [tail]), table


def run_table(ctx, buf, table, bpp):
    dev = torch.from_numpy(buf).cuda()
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    rc, msg = tiles_call(ctx, dev, buf.size, table, table_dev, len(table), bpp)
    assert rc == 0, msg
    ctx.sync()
    return dev.cpu().numpy()


@pytest.mark.parametrize("bpp", TC.BPPS)
def test_every_shape_and_filter_through_the_kernel_entry(png, ctx, bpp):
    """Rows around one band and two, widths around the lane skew and the block, each filter type on every row and a seeded mix: all
    shapes of one filter kind in ONE table in shuffled order, so short and long segments of different sweep counts share each launch."""
    T = png.TILE_PIXELS
    shapes = TC.shapes(T)
    assert {r for r, _ in shapes} == {1, 63, 64, 65, 128, 129} and {1, 2, 62, 63, 64, 65, T - 63, T - 1, T, T + 1, 2 * T + 1} == {p for _, p in shapes}
    sweeps = {png.plan_tiles(r, p * bpp, bpp).sweeps for r, p in shapes}
    assert len(sweeps) > 3                                                # hence grids whose segments end on different sweeps
    rs = np.random.RandomState(100 + bpp)
    for kind in TC.FILTER_KINDS:
        buf, want, table = packed(png, rs, shapes, bpp, kind)
        got = run_table(ctx, buf, table, bpp)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (kind, bad[:8].tolist(), table[:3].tolist())
        assert kind == 0 or not np.array_equal(got, buf)


def test_one_pass_is_a_table_of_one_entry_and_equals_the_band_kernel(png, ctx):
    """A whole pass of 200 rows by 2 T + 70 pixels: the raw rows, and byte for byte radnet_png_unfilter_u8 on a copy; a filter type
    above 4 is treated as None by both."""
    T = png.TILE_PIXELS
    rs = np.random.RandomState(9)
    for bpp, kind in ((3, "mix"), (4, 4), (1, 3)):
        buf, want, table = packed(png, rs, [(200, 2 * T + 70)], bpp, kind)
        assert np.array_equal(run_table(ctx, buf, table, bpp), want), (bpp, kind)
        at, rows, rowbytes = (int(v) for v in table[0])
        odd = buf.copy()
        odd[at + 3 * (1 + rowbytes)] = 7                                   # a filter type above 4 on row 3
        ref = torch.from_numpy(odd).cuda()
        ctx.call("radnet_png_unfilter_u8", ref.data_ptr() + at, rows, rowbytes, bpp)
        assert np.array_equal(run_table(ctx, odd, table, bpp), ref.cpu().numpy()), (bpp, kind)


def test_refusals_leave_the_buffer_as_it_was(png, ctx):
    T = png.TILE_PIXELS
    rs = np.random.RandomState(77)
    buf, _, table = packed(png, rs, [(70, 12), (130, T + 1), (5, 40)], 3, 4)
    dev = torch.from_numpy(buf).cuda()
    table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
    n = len(table)

    def refused(what, rc, msg, mention=None):
        assert rc != 0 and msg, what
        assert mention is None or mention in msg, (what, msg)
        ctx.sync()
        assert np.array_equal(dev.cpu().numpy(), buf), what               # nothing ran, not even the segments in front of the bad one

    def with_entry(i, **fields):
        t = table.copy()
        for k, v in fields.items():
            t[k][i] = v
        return t

    last, far = n - 1, int(np.argmax(table["offset"]))
    for what, t in (("offset beyond the buffer", with_entry(last, offset=buf.size - 3)),
                    ("offset far beyond the buffer", with_entry(last, offset=1 << 62)),
                    ("negative offset", with_entry(last, offset=-1)),
                    ("one row too many", with_entry(far, rows=int(table["rows"][far]) + 2)),
                    ("rowbytes % bpp", with_entry(last, rowbytes=13)),
                    ("zero rowbytes", with_entry(last, rowbytes=0)),
                    ("zero rows", with_entry(last, rows=0)),
                    ("negative rows", with_entry(last, rows=-5))):
        bad = int(np.flatnonzero((t != table))[0])
        refused(what, *tiles_call(ctx, dev, buf.size, t, table_dev, n, 3), mention="segment %d" % bad)
    refused("a buffer shorter than the segments", *tiles_call(ctx, dev, 100, table, table_dev, n, 3), mention="segment")
    refused("bpp", *tiles_call(ctx, dev, buf.size, table, table_dev, n, 5))
    refused("null buffer", *tiles_call(ctx, None, buf.size, table, table_dev, n, 3))
    refused("null host table", *tiles_call(ctx, dev, buf.size, None, table_dev, n, 3))
    refused("null device table", *tiles_call(ctx, dev, buf.size, table, None, n, 3))
    refused("negative count", *tiles_call(ctx, dev, buf.size, table, table_dev, -1, 3))
    fn = ctx.lib.radnet_png_unfilter_tiles_width_u8
    for width in (0, 32, 63, 100, 8192):
        assert fn(ctx.h, dev.data_ptr(), buf.size, table.ctypes.data, table_dev.data_ptr(), n, 3, width) != 0, width
    assert tiles_call(ctx, dev, buf.size, table, table_dev, n, 3, handle=False)[0] != 0
    assert tiles_call(ctx, dev, buf.size, table, table_dev, 0, 3)[0] == 0      # count == 0: RADNET_OK, no launch, whatever the pointers
    assert tiles_call(ctx, None, 0, None, None, 0, 3)[0] == 0
    ctx.sync()
    assert np.array_equal(dev.cpu().numpy(), buf)


def test_other_block_widths_give_the_same_bytes(png, ctx):
    """The width-given entry of the timing tool at T = 64 and 256, on shapes around those widths."""
    rs = np.random.RandomState(5)
    for width in (64, 256):
        shapes = [(129, p) for p in (1, 63, width - 63, width - 1, width, width + 1, 2 * width + 1)] + [(64, 65), (1, width)]
        buf, want, table = packed(png, rs, shapes, 3, "mix")
        dev = torch.from_numpy(buf).cuda()
        table_dev = torch.from_numpy(table.view(np.uint8)).cuda()
        rc = ctx.lib.radnet_png_unfilter_tiles_width_u8(ctx.h, dev.data_ptr(), buf.size, table.ctypes.data, table_dev.data_ptr(), len(table), 3, width)
        assert rc == 0
        ctx.sync()
        assert np.array_equal(dev.cpu().numpy(), want), width


# ---- the decoders ---------------------------------------------------------------------------------------------------------------------
def rle_file(data, idat_sizes=()):
    """The PNG file `data` with its IDAT stream compressed again as a run-length stream (level 1, Z_RLE: what inflate="device" takes),
    cut into IDAT chunks of idat_sizes and the rest."""
    pos, parts, idat = 8, [K.SIGNATURE], b""
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + length]
        elif kind == b"IEND":
            c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
            z = c.compress(zlib.decompress(idat)) + c.flush()
            for size in idat_sizes:
                parts.append(K.chunk(b"IDAT", z[:size]))
                z = z[size:]
            parts += [K.chunk(b"IDAT", z), K.chunk(b"IEND")]
        else:
            parts.append(data[pos:pos + 12 + length])
        pos += 12 + length
    return b"".join(parts)


def file_cases(png):
    """(what, samples, colour type, depth, palette, encode arguments): every legal colour type and depth, Adam7 at (1, 1), (9, 9),
    (33, 17) and with a pass of more than 64 rows, several IDAT chunks."""
    T = png.TILE_PIXELS
    rs = np.random.RandomState(2025)
    out = []

    def add(what, h, w, color_type, depth, filters, **kw):
        pal = rs.randint(0, 256, (1 << depth, 3)).astype(np.uint8) if color_type == 3 else None
        out.append((what, K.draw(rs, h, w, color_type, depth), color_type, depth, pal, dict(filters=filters, **kw)))

    for k, (color_type, depth) in enumerate(K.LEGAL):
        add("format %d/%d" % (color_type, depth), 65 + k, (1, 2, 97, T + 5)[k % 4], color_type, depth, 4 if k % 3 == 0 else np.random.RandomState(k) if k % 3 == 1 else "adaptive")
    for h, w in ((1, 1), (9, 9), (33, 17), (200, 97)):                    # 200 rows: the last pass has 100
        add("Adam7 %d x %d" % (h, w), h, w, 2, 8, np.random.RandomState(h), interlace=True)
    add("Adam7 150 x 70 grey 16", 150, 70, 0, 16, 4, interlace=True)
    add("IDAT chunks", 130, 2 * T + 1, 2, 8, "adaptive", idat_sizes=(1, 2, 300, 4000))
    add("Paeth 200 rows", 200, 2 * T + 70, 6, 8, 4)
    return out


@pytest.fixture(scope="module")
def files(png):
    """The cases encoded once: (what, the file, the file as a run-length stream, the expected image, its passes as (rows, rowbytes, bpp))."""
    out = []
    for what, s, ct, d, pal, kw in file_cases(png):
        enc = K.encode(s, ct, d, palette=pal, **kw)
        bpp = max(1, K.CHANNELS[ct] * d // 8)
        out.append((what, enc.data, rle_file(enc.data, idat_sizes=kw.get("idat_sizes", ())), K.expand(s, ct, d, pal), [(p[5], p[6], bpp) for p in enc.passes]))
    return out


def test_decode_device_by_tiles_on_the_host_inflate_path(png, files):
    assert png.TILE_ROWS == 64 and png.TILE_PIXELS % 32 == 0
    for what, data, _, want, passes in files:
        report = {}
        got = png.decode_device(data, unfilter="tiles", report=report)
        assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), what
        assert report["path"] == "host" and report["reconstruction"] == "tiles", (what, report)
        assert report["sweeps"] == max(png.plan_tiles(*p).sweeps for p in passes), (what, report)
        assert set(report) == {"path", "reason", "candidates", "false_candidates", "units", "blocks", "reconstruction", "sweeps"}
    band = {}
    png.decode_device(files[0][1], report=band)
    assert set(band) == {"path", "reason", "candidates", "false_candidates", "units", "blocks", "reconstruction"} and band["reconstruction"] is None


@pytest.mark.parametrize("inflate", ["device", "device-lz"])
def test_decode_device_by_tiles_on_the_device_inflate_paths(png, files, inflate):
    ways, on_device = set(), 0
    for what, data, rle, want, passes in files:
        data = rle if inflate == "device" else data
        report = {}
        got = png.decode_device(data, inflate=inflate, unfilter="tiles", report=report)
        assert np.array_equal(got.cpu().numpy(), want), what
        if report["path"] == "host":                                       # a stream the device inflate leaves to the host: tiled there
            assert report["reason"] and report["reconstruction"] == "tiles", (what, report)
            continue
        on_device += 1
        # the segments of the report's planner: those above 64 rows went to the tiles entry
        img = png.parse(data)
        table = png.plan_segments(img)
        long = table[table["rows"] > 64]
        assert report["reconstruction"] == ("tiles" if len(long) == len(table) else "segments+tiles"), (what, report)
        assert report["sweeps"] == max([png.plan_tiles(int(t["rows"]), int(t["rowbytes"]), img.bpp).sweeps for t in long], default=0), (what, report)
        ways.add((report["reconstruction"], report["sweeps"] > 0))
        default = {}
        png.decode_device(data, inflate=inflate, report=default)
        assert "sweeps" not in default and default["reconstruction"] in ("segments", "unfilter")
    assert on_device >= len(files) - 2, on_device
    assert ways == {("tiles", True), ("segments+tiles", True), ("segments+tiles", False)}, ways


def test_a_file_the_device_cannot_inflate_falls_back_and_is_still_tiled(png):
    T = png.TILE_PIXELS
    s = K.draw(np.random.RandomState(6), 130, 2 * T + 1, 2, 8, "low")     # few values, level 6: matches at other distances than 1
    data = K.encode(s, 2, 8, filters=4).data
    report = {}
    got = png.decode_device(data, inflate="device", unfilter="tiles", report=report)
    assert np.array_equal(got.cpu().numpy(), K.expand(s, 2, 8))
    assert report["path"] == "host" and report["reason"] and report["reconstruction"] == "tiles", report
    assert report["sweeps"] == png.plan_tiles(130, 3 * (2 * T + 1), 3).sweeps


def test_decode_device_many_by_tiles(png, files):
    """A mixed list: every bpp, all-Paeth files above 64 rows, files with None / Sub rows (cut into segments), Adam7."""
    datas = [f[1] for f in files]
    imgs = [png.parse(d) for d in datas]
    tables = [png.plan_segments(im) for im in imgs]
    rows = np.concatenate([t["rows"] for t in tables])
    assert {im.bpp for im in imgs} == {1, 2, 3, 4, 6, 8} and (rows > 64).any() and (rows <= 64).any()
    assert any(len(t) > len(im.passes) for t, im in zip(tables, imgs)) and any(len(t) == 1 and t["rows"][0] > 64 for t in tables)
    many = png.decode_device_many(datas, unfilter="tiles")
    assert len(many) == len(files)
    for (what, _, _, want, _), got in zip(files, many):
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), what
    (one,) = png.decode_device_many([datas[-1]], unfilter="tiles")
    assert np.array_equal(one.cpu().numpy(), files[-1][3])


def test_get_image_the_loader_and_predict_from_path_by_tiles(png, tmp_path, monkeypatch):
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
    assert rnet.png_unfilter == "band" and RADNet.png_unfilter == "band"
    img = np.random.RandomState(41).randint(0, 256, (420, 460, 3)).astype(np.uint8)
    os.makedirs(tmp_path / "blended_grey")
    (tmp_path / "blended_grey" / "scan.png").write_bytes(K.encode(img[:, :, ::-1], 2, 8, filters="adaptive").data)
    monkeypatch.chdir(tmp_path.parent)
    rel = tmp_path.name + "/scan.png"
    seen, decode = [], png.decode_device

    def watched(data, ctx=None, inflate="host", report=None, **kw):
        report = {} if report is None else report
        seen.append((kw.get("unfilter"), report))
        return decode(data, ctx, inflate, report, **kw)
    monkeypatch.setattr(png, "decode_device", watched)
    assert np.array_equal(utils_io.get_image(rel, Cc.img_types), img)                                 # the default, as before
    assert np.array_equal(utils_io.get_image(rel, Cc.img_types, unfilter="tiles"), img)
    on_device = utils_io.get_image(rel, Cc.img_types, to_host=False, unfilter="tiles", inflate="device-lz")
    assert on_device.is_cuda and np.array_equal(on_device.cpu().numpy(), img)
    assert [(u, r["reconstruction"]) for u, r in seen[:2]] == [(None, None), ("tiles", "tiles")]
    assert len(seen) == 3 and seen[2][0] == "tiles" and seen[2][1]["reconstruction"] in ("tiles", "segments+tiles") and seen[2][1]["path"] == "device"
    del seen[:]
    want = rnet.predict_from_path(rel)
    assert len(want) > 0 and [(u, r["reconstruction"]) for u, r in seen] == [(None, None)]
    rnet.png_unfilter = "tiles"
    got = rnet.predict_from_path(rel)
    assert [(u, r["reconstruction"]) for u, r in seen[1:]] == [("tiles", "tiles")]
    assert len(got) == len(want)
    for x, y in zip(got, want):
        assert list(x) == list(y) and all(type(x[k]) is type(y[k]) and np.array_equal(x[k], y[k]) for k in x), (x, y)
    del seen[:]
    d = {"filepath": rel}
    loader = utils_io.DeviceImageLoader(cache_bytes=1 << 24, unfilter="tiles")
    assert np.array_equal(loader(d, "blended_grey").cpu().numpy(), img) and [u for u, _ in seen] == ["tiles"]
    fresh = utils_io.DeviceImageLoader(cache_bytes=1 << 24, unfilter="tiles")
    assert fresh.prefetch([(d, "blended_grey")]) == 1 and np.array_equal(fresh(d, "blended_grey").cpu().numpy(), img) and fresh.hits == 1
