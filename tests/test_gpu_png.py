"""PNG files decoded on the device (faster_rcnn/png.py over csrc/png.hip: scanline reconstruction and expansion to BGR) against
tests/png_cases.py: expected = the expansion rules applied to the source samples, product = decode of the encoded file.  Every
comparison is byte equality.  Then the decoder on a BackgroundFeed worker thread and TileFeed(device_augment=True) reading files
through utils_io.DeviceImageLoader."""
import os
import threading

import numpy as np
import pytest

import png_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BPP_FORMATS = [(0, 8), (4, 8), (2, 8), (6, 8), (2, 16), (6, 16)]      # bpp 1, 2, 3, 4, 6, 8
BPP_IDS = ["grey8", "greyalpha8", "rgb8", "rgba8", "rgb16", "rgba16"]


@pytest.fixture(scope="module")
def png():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    from faster_rcnn import png
    return png


def palette(n, seed=1):
    return np.random.RandomState(seed).randint(0, 256, size=(n, 3)).astype(np.uint8)


def check(png, samples, color_type, depth, pal=None, what=None, **kw):
    enc = K.encode(samples, color_type, depth, palette=pal, **kw)
    got = png.imdecode_color(enc.data)
    want = K.expand(samples, color_type, depth, pal)
    assert got.dtype == np.uint8 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, np.argwhere((got != want).any(axis=2))[:4].tolist())
    return enc


@pytest.mark.parametrize("fmt", BPP_FORMATS, ids=BPP_IDS)
def test_each_filter_type_on_every_row_and_mixed(png, fmt):
    color_type, depth = fmt
    rs = np.random.RandomState(10 * color_type + depth)
    for kind in ("low", "high", "full"):
        s = K.draw(rs, 29, 37, color_type, depth, kind)
        for f in range(5):
            check(png, s, color_type, depth, filters=f, what=(kind, f))
        check(png, s, color_type, depth, filters=np.random.RandomState(7), what=(kind, "mixed"))
        check(png, s, color_type, depth, filters="adaptive", what=(kind, "adaptive"))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 70), (70, 1), (2, 2), (3, 5)])
def test_degenerate_sizes(png, w, h):
    rs = np.random.RandomState(w * 100 + h)
    for color_type, depth in BPP_FORMATS + [(0, 1), (0, 16)]:
        s = K.draw(rs, h, w, color_type, depth)
        for f in (0, 1, 2, 3, 4, np.random.RandomState(1)):
            check(png, s, color_type, depth, filters=f, what=(color_type, depth, f if isinstance(f, int) else "mixed"))


def test_band_and_chunk_constants(png):
    from radnet_hip import lib as L
    assert png.UNFILTER_BAND_ROWS == L.header_constant("RADNET_PNG_UNFILTER_BAND_ROWS") and png.UNFILTER_BAND_ROWS % 64 == 0
    assert png.UNFILTER_CHUNK_BYTES == L.header_constant("RADNET_PNG_UNFILTER_CHUNK_BYTES") and png.UNFILTER_CHUNK_BYTES % 24 == 0


def seam_rows(png):
    B = png.UNFILTER_BAND_ROWS
    return sorted({63, 64, 65, B - 1, B, B + 1})


@pytest.mark.parametrize("which", range(6))
def test_wave_and_band_seams_in_the_row_count(png, which):
    """Paeth on every row: each row needs the row above, across the lane 63 -> lane 0 hand-over of two waves and across two bands."""
    rows = seam_rows(png)[which]
    rs = np.random.RandomState(rows)
    for (color_type, depth), w in (((0, 8), 70), ((2, 8), 5), ((6, 16), 9), ((4, 8), 33)):
        check(png, K.draw(rs, rows, w, color_type, depth, "low" if w == 5 else "full"), color_type, depth, filters=4, what=(rows, color_type, depth))
    check(png, K.draw(rs, rows, 37, 2, 8), 2, 8, filters=np.random.RandomState(2), what=(rows, "mixed"))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_chunk_seams_in_the_row_bytes(png, delta):
    """Row byte counts around one and two staging chunks (grey8: one byte per pixel), and the whole-pixel counts at the chunk for the
    wider pixels; Paeth on every row, 5 to 70 rows; then the band seam and the chunk seam together."""
    CB = png.UNFILTER_CHUNK_BYTES
    rs = np.random.RandomState(40 + delta)
    for n in (CB + delta, 2 * CB + delta):
        for rows in (5, 66, 70):
            check(png, K.draw(rs, rows, n, 0, 8), 0, 8, filters=4, what=(n, rows))
            check(png, K.draw(rs, rows, n, 0, 8, "low"), 0, 8, filters=3, what=(n, rows, "average"))
    for (color_type, depth), bpp in zip(BPP_FORMATS, (1, 2, 3, 4, 6, 8)):
        w = CB // bpp + delta                      # rowbytes = CB + delta * bpp
        check(png, K.draw(rs, 67, w, color_type, depth), color_type, depth, filters=4, what=(color_type, depth, w))
    B = png.UNFILTER_BAND_ROWS
    check(png, K.draw(rs, B + 1, CB + delta, 0, 8), 0, 8, filters=4, what=("band and chunk", delta))
    check(png, K.draw(rs, B + 1, CB + delta, 0, 8), 0, 8, filters=np.random.RandomState(3), what=("band and chunk, mixed", delta))


@pytest.mark.parametrize("w", [1, 7, 8, 9, 13])
def test_sub_byte_depths(png, w):
    rs = np.random.RandomState(w)
    for depth in (1, 2, 4):
        s = K.draw(rs, 11, w, 0, depth)
        for f in (0, 2, 4, np.random.RandomState(w)):
            check(png, s, 0, depth, filters=f, what=("grey", depth))
    for depth in (1, 2, 4, 8):
        n = 1 << depth
        s = K.draw(rs, 11, w, 3, depth)
        s[0, 0, 0] = n - 1
        for f in (0, 1, 3, np.random.RandomState(w)):
            check(png, s, 3, depth, pal=palette(n, depth), filters=f, what=("palette", depth))
        if n > 2:
            short = palette(n // 2 + 1, depth)     # shorter than the largest index used: those pixels are 0
            enc = check(png, s, 3, depth, pal=short, filters=4, what=("short palette", depth))
            got = png.imdecode_color(enc.data)
            assert not got[s[:, :, 0] >= len(short)].any() and (s[:, :, 0] >= len(short)).any()


def test_sixteen_bit_grey_and_grey_alpha(png):
    rs = np.random.RandomState(16)
    for color_type in (0, 4):
        for kind in ("low", "high", "full"):
            s = K.draw(rs, 23, 31, color_type, 16, kind)
            for f in (0, 1, 2, 3, 4, np.random.RandomState(5)):
                check(png, s, color_type, 16, filters=f, what=(color_type, kind))


def test_trns_is_ignored(png):
    rs = np.random.RandomState(3)
    g = K.draw(rs, 9, 12, 0, 8)
    check(png, g, 0, 8, filters=4, trns=b"\x00" + bytes([int(g[0, 0, 0])]), what="grey")
    rgb = K.draw(rs, 9, 12, 2, 8)
    check(png, rgb, 2, 8, filters=4, trns=b"".join(b"\x00" + bytes([int(v)]) for v in rgb[0, 0]), what="rgb")
    idx = K.draw(rs, 9, 12, 3, 4)
    check(png, idx, 3, 4, pal=palette(16), filters=4, trns=bytes(range(0, 160, 10)), what="palette")


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (8, 8), (9, 9), (33, 17)])
def test_adam7(png, w, h):
    rs = np.random.RandomState(w + h)
    for color_type, depth, pal in ((2, 8, None), (3, 4, palette(16)), (0, 16, None)):
        s = K.draw(rs, h, w, color_type, depth)
        enc = check(png, s, color_type, depth, pal=pal, filters=np.random.RandomState(w), interlace=True, what=(color_type, depth))
        assert len(enc.passes) == len(K.pass_list(w, h, True))
        check(png, s, color_type, depth, pal=pal, filters=4, interlace=True, what=(color_type, depth, "paeth"))


def test_multiple_idat_chunks(png):
    rs = np.random.RandomState(9)
    s = K.draw(rs, 40, 50, 2, 8)
    one = check(png, s, 2, 8, filters="adaptive")
    for sizes in ([1], [1, 1, 0, 3], [2, 100, 1000], [7] * 40):      # [1]: split inside the two-byte zlib header
        enc = check(png, s, 2, 8, filters="adaptive", idat_sizes=sizes, what=sizes)
        assert enc.data.count(b"IDAT") == len(sizes) + 1 and len(enc.data) == len(one.data) + 12 * len(sizes)


def test_decode_device_on_a_background_feed_worker_thread(png):
    """BackgroundFeed's worker decodes on its own context and stream (runtime.default_context per thread): same bytes."""
    from faster_rcnn import data_feed as F
    rs = np.random.RandomState(21)
    files = [K.encode(K.draw(rs, 150, 130, 2, 8), 2, 8, filters="adaptive").data,
             K.encode(K.draw(rs, 90, 77, 0, 16), 0, 16, filters=np.random.RandomState(1), interlace=True).data,
             K.encode(K.draw(rs, 600, 100, 6, 8), 6, 8, filters=4).data]
    main = [png.decode_device(f) for f in files]
    assert all(t.is_cuda and t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3 and t.is_contiguous() for t in main)

    class Feed:
        rng = np.random.RandomState(0)

        def __iter__(self):
            for f in files * 3:
                assert threading.current_thread() is not threading.main_thread()
                yield png.decode_device(f)

    bg = F.BackgroundFeed(Feed(), depth=2)
    try:
        got = [t.cpu().numpy() for t in bg]
    finally:
        bg.close()
    assert len(got) == 9
    for k, g in enumerate(got):
        assert np.array_equal(g, main[k % 3].cpu().numpy()), k


def test_tile_feed_with_device_image_loader(png, tmp_path, monkeypatch):
    """TileFeed(device_augment=True) over files read by DeviceImageLoader against the same feed given the same pixels as NumPy
    arrays: same image bytes, same boxes, same rng position; the second pass over the data comes out of the cache."""
    from faster_rcnn import data_feed as F
    from faster_rcnn import utils_io
    from faster_rcnn.config import Config
    from test_data_feed import CLASSES, dataset
    C = Config()
    C.use_noise = False
    C.img_types = ["rgb", "topo"]
    C.use_img_type = True
    C.img_size, C.tile_size, C.tile_overlap, C.balanced_classes, C.max_n_tiles_train = 200, 200, 100, False, 2
    data, base = dataset(3, [(420, 310), (200, 260)])
    pixels = {}
    rs = np.random.RandomState(77)
    for d in data:
        for k, t in enumerate(C.img_types):
            img = base[d["filepath"]] if k == 0 else rs.randint(0, 256, base[d["filepath"]].shape).astype(np.uint8)
            path = utils_io.image_path(d["filepath"], t)
            os.makedirs(tmp_path / os.path.dirname(path), exist_ok=True)
            (tmp_path / path).write_bytes(K.encode(img[:, :, ::-1], 2, 8, filters="adaptive").data)      # the file holds R, G, B
            pixels[(d["filepath"], t)] = img
    monkeypatch.chdir(tmp_path)
    assert utils_io.image_size(utils_io.image_path(data[0]["filepath"], "rgb")) == (420, 310)
    assert np.array_equal(utils_io.load_image(data[0], "topo"), pixels[(data[0]["filepath"], "topo")])
    cc = {c: 1 for c in CLASSES}
    rng_ref, rng_dev = np.random.RandomState(5), np.random.RandomState(5)
    loader = utils_io.DeviceImageLoader(cache_bytes=64 << 20)
    ref = F.TileFeed([dict(d) for d in data], C, cc, lambda d, t: pixels[(d["filepath"], t)], rng=rng_ref, device_augment=True)
    dev = F.TileFeed([dict(d) for d in data], C, cc, loader, rng=rng_dev, device_augment=True)
    n = 16                                         # two images, up to two tiles and the full image each: several passes over the data
    for k, (a, b) in enumerate(zip(ref, dev)):
        assert (a["filepath"], a["width"], a["height"], a["bboxes"]) == (b["filepath"], b["width"], b["height"], b["bboxes"]), k
        assert b["img"].is_cuda and np.array_equal(a["img"].cpu().numpy(), b["img"].cpu().numpy()), k
        if k + 1 == n:
            break
    sa, sb = rng_ref.get_state(), rng_dev.get_state()
    assert np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    assert loader.misses <= 4 and loader.hits > 0 and loader.hits + loader.misses >= n
    off = utils_io.DeviceImageLoader(cache_bytes=0)
    one = off(data[0], "rgb")
    assert off(data[0], "rgb") is not one and (off.hits, off.misses) == (0, 2)
    assert np.array_equal(one.cpu().numpy(), pixels[(data[0]["filepath"], "rgb")])
