"""png.decode_device_many with a device inflate, through the public API: byte for byte decode_device per file and the NumPy statement
of tests/png_cases.py, in every combination of the modes; the per-file report (a file the device refuses goes to the host path
alone, with decode_device's reason); paths against arrays; the launch list of a batch the device takes whole, written out here
from the documented rules with a recording context (the Recorder idea of tests/test_gpu_png_launch_order.py); corrupt files, which
raise what the host-inflate entry raises; and the two callers, DeviceImageLoader(prefetch_modes=True) and RADNet.png_many."""
import copy
import itertools
import os
import zlib

import numpy as np
import pytest

import png_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEGMENTS, TILES, EXPAND = "radnet_png_unfilter_segments_u8", "radnet_png_unfilter_tiles_u8", "radnet_png_expand_bgr_u8"
CRC, JOIN = "radnet_crc32_segments", "radnet_png_join_u8"
CHECKED = ["radnet_deflate_rle_scan_u8", "radnet_png_gather_column_u8"]      # the Adler-32 parts, the filter-type column: a pair per file
ONE_STREAM = {"radnet_inflate_find_blocks", "radnet_inflate_rle_measure", "radnet_inflate_rle_emit", "radnet_inflate_lz_measure", "radnet_inflate_lz_emit"}
FIND, LZ_RESOLVE, LZ_GATHER = "radnet_inflate_find_blocks_many", "radnet_inflate_lz_resolve", "radnet_inflate_lz_gather"
MANY = {"device": [FIND, "radnet_inflate_rle_measure_many", "radnet_inflate_rle_emit_many"],
        "device-lz": [FIND, "radnet_inflate_lz_measure_many", "radnet_inflate_lz_emit_many"]}
NOT_RLE = "chain: a unit that did not decode (not run-length)"


class Recorder:
    """A context as decode_device_many takes one: call() notes the entry's name and forwards to the real context."""

    def __init__(self, ctx):
        self.ctx, self.names = ctx, []

    def call(self, name, *args):
        self.names.append(name)
        return self.ctx.call(name, *args)


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


File = type("File", (), {})


def _file(name, data, samples, color=2, depth=8, palette=None):
    f = File()
    f.name, f.data, f.want = name, data, K.expand(samples, color, depth, palette)
    return f


@pytest.fixture(scope="module")
def batch(png):
    """The eight files, in this order: P 100 x 40 Paeth; I 33 x 33 Adam7; S2 200 x 40 run-length with segments of both kinds; Z level 6
    with far matches; G 1-bit grey; PAL a palette file; ONE 1 x 1; CUT one stream in IDAT chunks of 1 to 7 bytes."""
    rs = np.random.RandomState(61)
    out = []
    samples = K.draw(rs, 100, 40, 2, 8)
    out.append(_file("P", K.encode(samples, 2, 8, filters=4, level=1).data, samples))
    samples = K.draw(rs, 33, 33, 2, 8)
    out.append(_file("I", K.encode(samples, 2, 8, filters="adaptive", interlace=True).data, samples))
    samples = K.draw(rs, 200, 40, 2, 8)
    lines, _ = K.filter_rows(samples.reshape(200, 120).astype(np.uint8), 3, np.where(np.isin(np.arange(200), (0, 30, 130)), 0, 2))
    out.append(_file("S2", png.assemble(lines.tobytes(), 40, 200, 2), samples))
    samples = np.tile(K.draw(rs, 8, 8, 2, 8), (8, 8, 1))
    out.append(_file("Z", K.encode(samples, 2, 8, filters=0, level=6).data, samples))
    samples = K.draw(rs, 70, 45, 0, 1)
    out.append(_file("G", K.encode(samples, 0, 1, filters=2).data, samples, 0, 1))
    samples, palette = K.draw(rs, 21, 19, 3, 4), rs.randint(0, 256, (16, 3))
    out.append(_file("PAL", K.encode(samples, 3, 4, filters=rs, palette=palette).data, samples, 3, 4, palette))
    samples = K.draw(rs, 1, 1, 2, 8)
    out.append(_file("ONE", K.encode(samples, 2, 8).data, samples))
    samples = K.draw(rs, 12, 20, 2, 8)
    z_len = len(zlib.compress(K.encode(samples, 2, 8, filters=1).stream, 6))
    sizes = list(itertools.islice(itertools.cycle(range(1, 8)), 2 * z_len))
    sizes = sizes[:int(np.searchsorted(np.cumsum(sizes), z_len))]      # the leading chunks; what is left, 1 to 7 bytes too, is the last
    out.append(_file("CUT", K.encode(samples, 2, 8, filters=1, idat_sizes=sizes).data, samples))
    return out


def test_the_files_are_what_the_cases_need(png, batch):
    by_name = {f.name: f for f in batch}
    rows = lambda f: png.plan_segments(png.parse(f.data))["rows"].tolist()      # noqa: E731
    assert rows(by_name["P"]) == [100] and rows(by_name["S2"]) == [30, 100, 70] and len(png.parse(by_name["I"].data).passes) == 7
    assert png.parse(by_name["ONE"].data).header[:2] == (1, 1) and png.parse(by_name["PAL"].data).header.color_type == 3
    pieces = [e - s for kind, s, e in png._chunks(memoryview(by_name["CUT"].data)) if kind == b"IDAT"]
    assert len(pieces) > 20 and set(pieces) <= set(range(1, 8))
    # which of them the run-length inflate takes, by decode_device itself
    took = {}
    for f in batch:
        report = {}
        assert np.array_equal(png.decode_device(f.data, inflate="device", report=report).cpu().numpy(), f.want)
        took[f.name] = (report["path"], report["reason"])
    assert took["Z"] == ("host", NOT_RLE) and took["P"] == took["S2"] == ("device", None), took


MODES = [dict(inflate=i, unfilter=u, crc=c, join=j) for i in ("device", "device-lz") for u in ("band", "tiles") for c in ("host", "device")
         for j in ("host", "device")]


@pytest.mark.parametrize("modes", MODES, ids=lambda m: "-".join(m.values()))
def test_many_equals_decode_device_file_by_file(png, ctx, batch, modes):
    report = {}
    got = png.decode_device_many([f.data for f in batch], report=report, **modes)
    assert len(got) == len(batch) and report["batches"] == 1 and report["overflow"] == 0
    for f, g, r in zip(batch, got, report["files"]):
        one = {}
        want = png.decode_device(f.data, report=one, **modes)
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), want.cpu().numpy()) and np.array_equal(g.cpu().numpy(), f.want), (f.name, modes)
        assert (r["path"], r["reason"]) == (one["path"], one["reason"]), (f.name, modes, r, one)
        for key in ("crc", "join", "units", "blocks", "candidates", "false_candidates", "far_units"):
            assert r.get(key) == one.get(key), (f.name, key, r, one)
        assert set(r) == set(one), (f.name, set(r) ^ set(one))
    paths = {f.name: r["path"] for f, r in zip(batch, report["files"])}
    if modes["inflate"] == "device":
        assert paths["Z"] == "host" and report["files"][3]["reason"] == NOT_RLE      # its neighbours keep the device
        assert paths["P"] == paths["S2"] == paths["ONE"] == "device", paths
    else:
        assert set(paths.values()) == {"device"}, report["files"]


def test_paths_are_read_like_arrays(png, batch, tmp_path):
    paths = []
    for f in batch:
        paths.append(str(tmp_path / (f.name + ".png")))
        with open(paths[-1], "wb") as out:
            out.write(f.data)
    mixed = [p if k % 2 else np.fromfile(p, np.uint8) for k, p in enumerate(paths)]
    for modes in (dict(), dict(inflate="device-lz"), dict(inflate="device-lz", join="device", crc="device"), dict(inflate="device", join="device")):
        for items in (paths, [tmp_path / (f.name + ".png") for f in batch], mixed):
            report = {}
            got = png.decode_device_many(items, report=report, **modes)
            for f, g in zip(batch, got):
                assert np.array_equal(g.cpu().numpy(), f.want), (f.name, modes)
            if modes.get("inflate") == "device-lz":
                assert {r["path"] for r in report["files"]} == {"device"}


@pytest.mark.parametrize("inflate", ["device", "device-lz"])
def test_the_launch_list_of_a_batch_the_device_takes_whole(png, ctx, batch, inflate):
    files = [f for f in batch if inflate == "device-lz" or f.name != "Z"]      # under "device" without the file that leaves for the host
    imgs = [png.parse(f.data) for f in files]
    for unfilter, crc, join in (("band", "host", "host"), ("tiles", "device", "device")):
        rec, report = Recorder(ctx), {}
        got = png.decode_device_many([f.data for f in files], ctx=rec, unfilter=unfilter, inflate=inflate, crc=crc, join=join, report=report)
        for f, g in zip(files, got):
            assert np.array_equal(g.cpu().numpy(), f.want)
        assert {r["path"] for r in report["files"]} == {"device"}
        names = rec.names
        for entry in MANY[inflate]:
            assert names.count(entry) == 1, (entry, names)
        assert not ONE_STREAM & set(names), names
        want = [JOIN] * len(files) * (join == "device") + [CRC] * (crc == "device") + MANY[inflate]
        if inflate == "device-lz":
            rounds = report["files"][0]["rounds"]
            assert all(r["rounds"] == rounds for r in report["files"])
            bound = (sum(len(im.stream) for im in imgs) - 1).bit_length()
            groups = min(-(-(rounds + 1) // 4), -(-bound // 4))          # once for the batch: up to the group with the first idle round
            want += [LZ_RESOLVE] * groups + [LZ_GATHER]
        want += CHECKED * len(files)
        for bpp in sorted({im.bpp for im in imgs}):                       # ONE table: grouped by bpp, short segments first
            rows = np.concatenate([png.plan_segments(im)["rows"] for im in imgs if im.bpp == bpp])
            if unfilter == "band":
                want.append(SEGMENTS)
            else:
                want += [SEGMENTS] * bool((rows <= 64).any()) + [TILES] * bool((rows > 64).any())
        want += [EXPAND] * sum(len(im.passes) for im in imgs)
        assert names == want, (unfilter, crc, join)


@pytest.mark.parametrize("unfilter", ["band", "tiles"])
def test_with_a_host_inflate_the_list_is_what_it_was(png, ctx, batch, unfilter):
    files = [batch[0], batch[4], batch[1]]
    imgs = [png.parse(f.data) for f in files]
    want = []
    for bpp in sorted({im.bpp for im in imgs}):
        rows = np.concatenate([png.plan_segments(im)["rows"] for im in imgs if im.bpp == bpp])
        want += [SEGMENTS] if unfilter == "band" else [SEGMENTS] * bool((rows <= 64).any()) + [TILES] * bool((rows > 64).any())
    want += [EXPAND] * sum(len(im.passes) for im in imgs)
    rec = Recorder(ctx)
    got = png.decode_device_many([f.data for f in files], ctx=rec, unfilter=unfilter, inflate="host", crc="host", join="host")
    assert rec.names == want
    for f, g in zip(files, got):
        assert np.array_equal(g.cpu().numpy(), f.want)


def outcome(fn):
    try:
        return "ok", [g.cpu().numpy() for g in fn()]
    except Exception as e:      # noqa: BLE001  (the type and the message are what is compared)
        return type(e).__name__, str(e)


def test_corrupt_files_raise_what_the_host_entry_raises(png, batch):
    good = [batch[0].data, batch[2].data, batch[5].data]
    data = bytearray(good[1])
    idat = [(s, e) for kind, s, e in png._chunks(memoryview(bytes(data))) if kind == b"IDAT"]
    bad_crc = bytearray(data)
    bad_crc[idat[0][1]] ^= 0x40                                            # the CRC field of file 1's first IDAT chunk
    flipped = bytearray(data)
    flipped[(idat[0][0] + idat[0][1]) // 2] ^= 0x08                        # a bit inside file 1's stream; the chunk's CRC is made to fit
    s, e = idat[0]
    flipped[e:e + 4] = zlib.crc32(bytes(flipped[s - 4:e])).to_bytes(4, "big")
    truncated = data[:len(data) - 30]
    modes = [dict(inflate=i, crc=c, join=j) for i in ("device", "device-lz") for c in ("host", "device") for j in ("host", "device")]
    for what, broken in (("bad CRC", bad_crc), ("flipped bit", flipped), ("truncated", truncated)):
        files = [good[0], bytes(broken), good[2]]
        want = outcome(lambda: png.decode_device_many(files))
        assert want[0] == "ValueError" and want[1].startswith("file 1: "), (what, want)
        for m in modes:
            assert outcome(lambda: png.decode_device_many(files, **m)) == want, (what, m)
        # a neighbour's error never hides a lower index: file 2 broken too, and in another way
        both = [good[0], bytes(broken), bytes(truncated if what != "truncated" else bad_crc)]
        assert outcome(lambda: png.decode_device_many(both))[1] == want[1]
        for m in modes[::3]:
            assert outcome(lambda: png.decode_device_many(both, **m)) == want, (what, m)


def test_prefetch_with_the_modes_fills_the_cache_with_the_same_images(png, batch, tmp_path, monkeypatch):
    from faster_rcnn import utils_io
    monkeypatch.chdir(tmp_path)
    data = []
    for f in batch:
        d = {"filepath": "maps/%s.png" % f.name}
        path = utils_io.image_path(d["filepath"], "rgb")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as out:
            out.write(f.data)
        data.append(d)
    pairs = [(d, "rgb") for d in data]
    calls, many = [], png.decode_device_many

    def watched(files, **kw):
        calls.append(([isinstance(f, str) for f in files], kw))
        return many(files, **kw)
    monkeypatch.setattr(png, "decode_device_many", watched)
    plain = utils_io.DeviceImageLoader(cache_bytes=64 << 20)
    assert plain.prefetch(pairs) == len(batch)
    loader = utils_io.DeviceImageLoader(cache_bytes=64 << 20, inflate="device-lz", join="device", prefetch_modes=True)
    assert loader.prefetch(pairs) == len(batch)
    assert calls == [([False] * len(batch), {}), ([True] * len(batch), dict(unfilter="band", inflate="device-lz", crc="host", join="device"))]
    for (d, t), f in zip(pairs, batch):
        got, want = loader(d, t), plain(d, t)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want.cpu().numpy()) and np.array_equal(got.cpu().numpy(), f.want)
    assert (loader.hits, loader.misses) == (len(batch), 0) == (plain.hits, plain.misses)


def test_predict_from_path_reads_the_types_in_one_pass(png, tmp_path, monkeypatch):
    from faster_rcnn import models as M
    from faster_rcnn.base_models import resnet50 as base
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    from oracle import dense
    Cc = Config()
    Cc.img_size = 300
    ms = M.build_models(Cc, weights=copy.deepcopy(dense.init_params(seed=3)), workload="predict")
    rnet = RADNet(Cc, ms[3], ms[4], base.preprocess)
    Cc.tile_size, Cc.tile_overlap, Cc.include_full_img, Cc.use_img_type = 400, 250, True, True
    Cc.img_types = ["blended_grey", "topo"]
    rnet.bbox_threshold, rnet.device_tail, rnet.device_resident = 0.0, True, True
    y, x = np.mgrid[0:420, 0:460]
    for k, kind in enumerate(Cc.img_types):
        img = np.stack([(x // (9 + k) + y // 7 * 3 + c * 40) & 255 for c in range(3)], axis=2).astype(np.uint8)
        os.makedirs(tmp_path / kind)
        (tmp_path / kind / "scan.png").write_bytes(K.encode(img[:, :, ::-1], 2, 8, filters="adaptive").data)
    monkeypatch.chdir(tmp_path.parent)
    rel = tmp_path.name + "/scan.png"
    reports, many = [], png.decode_device_many

    def watched(files, **kw):
        reports.append({})
        return many(files, report=reports[-1], **kw)
    monkeypatch.setattr(png, "decode_device_many", watched)
    rnet.png_inflate, rnet.png_join = "device-lz", "device"
    want = rnet.predict_from_path(rel)
    assert not reports and len(want) > 0
    rnet.png_many = True
    got = rnet.predict_from_path(rel)
    assert len(reports) == 1 and [r["path"] for r in reports[0]["files"]] == ["device", "device"]
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert list(a) == list(b) and all(type(a[k]) is type(b[k]) and np.array_equal(a[k], b[k]) for k in a), (a, b)
