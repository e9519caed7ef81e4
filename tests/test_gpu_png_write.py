"""The writer's device half and the rectangle painter: radnet_png_filter_rows_u8 against tests/png_cases.filter_rows (bytes and
types), png.encode_device read back by png.decode_device and by the tests' own decoder, radnet_draw_rects_u8 against the NumPy
painter of tests/png_write_cases.py on the whole buffer (pitch padding included), RADNet.draw_detections and
RADNet.write_predictions.  Every comparison is byte equality."""
import json
import os

import numpy as np
import pytest

import png_cases as K
import png_write_cases as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import draw_gpu_helpers as G  # noqa: E402  (needs torch)
from draw_gpu_helpers import ERR_ARG, SENTINEL, canvas  # noqa: E402


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


@pytest.fixture(scope="module")
def R(png):
    from faster_rcnn import RADNet
    return RADNet


# ---- the filter kernel ---------------------------------------------------------------------------------------------------------------
def filter_call(ctx, img_dev, h, w, channels, pitch, mode, stream_dev, handle=True):
    rc = ctx.lib.radnet_png_filter_rows_u8(ctx.h if handle else None, img_dev.data_ptr() if img_dev is not None else None, h, w, channels, pitch, mode,
                                           stream_dev.data_ptr() if stream_dev is not None else None)
    msg = ctx.lib.radnet_last_error(ctx.h)
    return rc, (msg.decode() if msg else "")


def device_stream(ctx, img, mode, pad=0, guard=0):
    """The kernel's stream for a [h][w] or [h][w][3] array as [h][1 + w * channels]; `pad` bytes of sentinels behind every image
    row, `guard` sentinel bytes behind the stream: both are checked to be unchanged."""
    h, w = img.shape[:2]
    channels = 1 if img.ndim == 2 else 3
    n = w * channels
    rows = np.full((h, n + pad), SENTINEL, np.uint8)
    rows[:, :n] = img.reshape(h, n)
    img_dev = torch.from_numpy(rows).cuda()
    out = torch.full((h * (1 + n) + guard,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc, msg = filter_call(ctx, img_dev, h, w, channels, n + pad, mode, out)
    assert rc == 0, msg
    got = out.cpu().numpy()
    assert (got[h * (1 + n):] == SENTINEL).all(), "bytes behind the stream were written"
    assert np.array_equal(img_dev.cpu().numpy(), rows), "the image was written"
    return got[:h * (1 + n)].reshape(h, 1 + n)


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("size", W.FILTER_SIZES, ids=["%dx%d" % s for s in W.FILTER_SIZES])
def test_filter_rows_against_the_reference_filter(ctx, size, channels):
    h, w = size
    for kind in W.FILTER_INPUTS:
        img = W.filter_input(kind, h, w, channels)
        raw = W.stream_rows(img)
        for mode in W.FILTER_MODES:
            want, types = K.filter_rows(raw, channels, "adaptive" if mode == 5 else mode)
            got = device_stream(ctx, img if channels == 3 else img[:, :, 0], mode)
            assert np.array_equal(got[:, 0], types), (kind, mode, got[:, 0].tolist(), types.tolist())
            assert np.array_equal(got, want), (kind, mode, np.argwhere(got != want)[:4].tolist())


def test_adaptive_choices_cover_the_types_and_the_ties(ctx):
    """What the inputs are meant to exercise does occur: the ramp makes Sub, Up and Paeth win somewhere; zeros tie everywhere and
    take type 0; a flat image ties Up with Paeth below row 0 and takes Up."""
    ramp = device_stream(ctx, W.filter_input("ramp", 67, 342, 3), 5)[:, 0]
    want = K.filter_rows(W.stream_rows(W.filter_input("ramp", 67, 342, 3)), 3, "adaptive")[1]
    assert np.array_equal(ramp, want) and {1, 2, 4} <= set(ramp.tolist())
    assert (device_stream(ctx, W.filter_input("constant", 67, 342, 3), 5)[:, 0] == 0).all()
    flat = device_stream(ctx, W.filter_input("flat", 5, 86, 3), 5)[:, 0]
    assert flat.tolist() == [1, 2, 2, 2, 2]
    half = np.full((3, 300), 128, np.uint8)                                # residuals of exactly 128 count 128 either way
    got = device_stream(ctx, half, 5)
    assert np.array_equal(got, K.filter_rows(half, 1, "adaptive")[0])


@pytest.mark.parametrize("channels", [3, 1])
def test_filter_rows_with_a_pitch_and_with_guard_bytes(ctx, channels):
    for h, w in ((3, 2), (2, 86), (67, 342)):
        img = W.filter_input("noise", h, w, channels, seed=7)
        img = img if channels == 3 else img[:, :, 0]
        for mode in (4, 5):
            want, _ = K.filter_rows(W.stream_rows(img), channels, "adaptive" if mode == 5 else mode)
            assert np.array_equal(device_stream(ctx, img, mode, pad=5), want), (h, w, mode, "pitch")
            assert np.array_equal(device_stream(ctx, img, mode, guard=64), want), (h, w, mode, "guard")


def test_filter_rows_argument_errors(ctx):
    img = torch.zeros(4 * 15, dtype=torch.uint8, device="cuda")
    out = torch.full((4 * 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    for what, args in (("null image", (None, 4, 5, 3, 15, 5, out)), ("null stream", (img, 4, 5, 3, 15, 5, None)), ("no rows", (img, 0, 5, 3, 15, 5, out)),
                       ("no columns", (img, 4, 0, 3, 15, 5, out)), ("two channels", (img, 4, 5, 2, 15, 5, out)), ("four channels", (img, 4, 3, 4, 15, 5, out)),
                       ("mode 6", (img, 4, 5, 3, 15, 6, out)), ("mode -1", (img, 4, 5, 3, 15, -1, out)), ("short pitch", (img, 4, 5, 3, 14, 5, out)),
                       ("a row above 2^24 bytes", (img, 1, (1 << 24) // 3 + 1, 3, 1 << 25, 0, out))):
        rc, msg = filter_call(ctx, *args)
        assert rc != 0 and msg, what
    assert filter_call(ctx, img, 4, 5, 3, 15, 5, out, handle=False)[0] == ERR_ARG
    ctx.sync()
    assert (out.cpu().numpy() == SENTINEL).all()


# ---- encode_device -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pictures():
    """{name: array}: an RGB image with more than one deflate piece at chunk_bytes=7 and rows beyond one sweep, a tiny one, a grey one."""
    return {"rgb": W.filter_input("ramp", 37, 101, 3), "noise": W.filter_input("noise", 5, 3, 3), "one": W.filter_input("noise", 1, 1, 3),
            "grey": W.filter_input("ramp", 23, 51, 1)[:, :, 0]}


def test_encode_device_round_trips(png, pictures):
    for name, img in pictures.items():
        dev = torch.from_numpy(img).cuda()
        data = png.encode_device(dev)
        assert isinstance(data, bytes)
        want = img if img.ndim == 3 else np.repeat(img[:, :, None], 3, axis=2)               # grey replicated to three channels
        back = png.decode_device(data)
        assert back.is_cuda and torch.equal(back, torch.from_numpy(want).cuda()), name
        assert np.array_equal(W.decode_bgr(data), want), name
        d = W.decode(data)
        assert d.color_type == (2 if img.ndim == 3 else 0) and d.kinds == [b"IHDR", b"IDAT", b"IEND"]
        lines, _ = K.filter_rows(W.stream_rows(img), 3 if img.ndim == 3 else 1, "adaptive")
        assert d.stream == lines.tobytes(), name                                               # the adaptive stream of the reference filter
        assert torch.equal(dev.cpu(), torch.from_numpy(img)), "the input was written"


def test_encode_device_arguments_do_not_change_the_image(png, pictures):
    img = pictures["rgb"]
    dev = torch.from_numpy(img).cuda()
    default = png.encode_device(dev)
    small = png.encode_device(dev, chunk_bytes=7, workers=3)
    assert small != default and W.decode(small).stream == W.decode(default).stream
    assert png.encode_device(dev, workers=1) == default == png.encode_device(dev)              # deterministic, whatever the threads
    assert png.encode_device(img) == default                                                  # a NumPy input: the bytes of the cuda input
    assert png.encode_device(pictures["grey"]) == png.encode_device(torch.from_numpy(pictures["grey"]).cuda())
    for f, mode in (("none", 0), ("sub", 1), ("up", 2), ("average", 3), ("paeth", 4), (3, 3)):
        d = W.decode(png.encode_device(dev, filter=f, level=6, strategy="default"))
        assert d.stream == K.filter_rows(W.stream_rows(img), 3, mode)[0].tobytes(), f
        assert np.array_equal(d.samples[:, :, ::-1], img)
    with pytest.raises(ValueError, match="contiguous"):
        png.encode_device(dev[:, ::2])
    with pytest.raises(TypeError, match="cuda"):
        png.encode_device(torch.from_numpy(img))


def test_imwrite_writes_encode_device(png, pictures, tmp_path):
    from faster_rcnn import utils_io
    dev = torch.from_numpy(pictures["rgb"]).cuda()
    path = tmp_path / "map.png"
    assert utils_io.imwrite(path, dev, chunk_bytes=100) is True
    assert path.read_bytes() == png.encode_device(dev, chunk_bytes=100)
    assert torch.equal(png.decode_device(np.fromfile(path, np.uint8)), dev)


# ---- the draw kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (70, 130)], ids=["64x64", "70x130"])
def test_draw_rects_against_the_painter(ctx, R, size):
    h, w = size
    for pad in (0, 7):
        buf = canvas(h, w, pad, seed=h + pad)
        for name, rects in W.rect_lists(h, w).items():
            rc, msg, got = G.rects_call(ctx, R, buf, h, w, 3 * w + pad, rects)
            assert rc == 0, (name, msg)
            want = G.expected(W.paint, buf, h, w, rects)
            assert np.array_equal(got, want), (name, pad, np.argwhere(got != want)[:4].tolist())
            if name in ("wholly outside", "outline wider than the image"):
                assert np.array_equal(got, buf), name
            elif not name.startswith("huge"):
                assert not np.array_equal(got, buf), name


def test_draw_rects_overlap_order_matters(ctx, R):
    lists = W.rect_lists(64, 64)
    buf = canvas(64, 64, 0)
    a = G.rects_call(ctx, R, buf, 64, 64, 192, lists["overlap a then b"])[2]
    b = G.rects_call(ctx, R, buf, 64, 64, 192, lists["overlap b then a"])[2]
    assert not np.array_equal(a, b)


def test_draw_rects_more_than_one_batch(ctx, R):
    """RADNET_DRAW_RECT_BATCH + 1 one-pixel rectangles on the 64x64 image: every tile walks two batches; the entry of the second
    batch lands on a pixel the first batch painted, and wins."""
    from radnet_hip import lib as L
    batch = L.header_constant("RADNET_DRAW_RECT_BATCH")
    rs = np.random.RandomState(12)
    xs, ys = rs.randint(0, 64, batch + 1), rs.randint(0, 64, batch + 1)
    xs[batch], ys[batch] = xs[3], ys[3]
    rects = [(int(x), int(y), int(x), int(y), 1 if k % 2 else W.FILLED, k % 256, (7 * k) % 256, 255 - k % 256) for k, (x, y) in enumerate(zip(xs, ys))]
    buf = canvas(64, 64, 3, seed=5)
    rc, msg, got = G.rects_call(ctx, R, buf, 64, 64, 195, rects)
    assert rc == 0, msg
    want = G.expected(W.paint, buf, 64, 64, rects)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert tuple(got[ys[3], 3 * xs[3]:3 * xs[3] + 3]) == rects[batch][5:]
    big = [(k % 60, (k * 7) % 60, k % 60 + 9, (k * 7) % 60 + 5, (1, 8, W.FILLED)[k % 3], k % 256, 3, 200) for k in range(2 * batch + 5)]
    rc, msg, got = G.rects_call(ctx, R, buf, 64, 64, 195, big)                                    # three batches of overlapping rectangles
    assert rc == 0 and np.array_equal(got, G.expected(W.paint, buf, 64, 64, big)), msg


def test_draw_rects_count_zero_and_refusals(ctx, R):
    h, w = 20, 30
    buf = canvas(h, w, 4)
    good = [(2, 2, 9, 9, 8, 1, 2, 3), (4, 4, 12, 12, W.FILLED, 255, 0, 255), (1, 1, 5, 5, 1, 0, 0, 0)]
    rc, msg, got = G.rects_call(ctx, R, buf, h, w, 3 * w + 4, [])
    assert rc == 0 and np.array_equal(got, buf)
    rc, msg, got = G.rects_call(ctx, R, buf, h, w, 3 * w + 4, good, count=0, host=False, dev=False)
    assert rc == 0 and np.array_equal(got, buf)

    def with_entry(i, **fields):
        t = [list(r) for r in good]
        for k, v in fields.items():
            t[i][R.RECT.names.index(k)] = v
        return t

    for what, rects, mention in (("thickness 0", with_entry(1, thickness=0), "rectangle 1"), ("blue 256", with_entry(2, b=256), "rectangle 2"),
                                 ("green -1", with_entry(0, g=-1), "rectangle 0"), ("red 1000", with_entry(2, r=1000), "rectangle 2")):
        rc, msg, got = G.rects_call(ctx, R, buf, h, w, 3 * w + 4, rects)
        assert rc == ERR_ARG and mention in msg, (what, msg)
        assert np.array_equal(got, buf), what                                                 # not even the entries in front of the bad one
    for what, kw in (("short pitch", dict(pitch=3 * w - 1)), ("negative count", dict(count=-1)), ("null host table", dict(host=False)),
                     ("null device table", dict(dev=False)), ("no context", dict(handle=False))):
        pitch = kw.pop("pitch", 3 * w + 4)
        rc, msg, got = G.rects_call(ctx, R, buf, h, w, pitch, good, **kw)
        assert rc == ERR_ARG and np.array_equal(got, buf), what
    rc, msg, got = G.rects_call(ctx, R, buf, 0, w, 3 * w + 4, good)
    assert rc == ERR_ARG and np.array_equal(got, buf)


# ---- RADNet.draw_detections and write_predictions -----------------------------------------------------------------------------------
class _Config:
    class_mapping = {"boat": 0, "human": 1, "animal": 2, "bg": 3}


DETS = [{'class': 'boat', 'prob': np.float32(0.91), 'x1': np.int64(10), 'y1': np.int64(20), 'x2': np.int64(70), 'y2': np.int64(60)},
        {'class': 'human', 'prob': 0.75, 'x1': 50, 'y1': 40, 'x2': 100, 'y2': 90},
        {'class': 'animal', 'prob': 0.25, 'x1': 90, 'y1': 5, 'x2': 126, 'y2': 45},
        {'class': 'wheel', 'prob': 1.0, 'x1': -4, 'y1': 70, 'x2': 30, 'y2': 99}]


def det_rects(dets, color, thickness=8):
    return [(int(d['x1']), int(d['y1']), int(d['x2']), int(d['y2']), thickness) + tuple(color) for d in dets]


def test_draw_detections(R):
    net = R.RADNet(_Config(), None, None, None)
    img = np.random.RandomState(1).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    out = net.draw_detections(dev, DETS)
    assert out.is_cuda and out.data_ptr() != dev.data_ptr() and torch.equal(dev.cpu(), torch.from_numpy(img))      # inplace=False: the input stays
    assert np.array_equal(out.cpu().numpy(), W.paint(img.copy(), det_rects(DETS, (255, 255, 255))))
    out = net.draw_detections(dev, DETS, color=(1, 2, 3), thickness=1, classes=("human", "wheel"))
    assert np.array_equal(out.cpu().numpy(), W.paint(img.copy(), det_rects(DETS[1::2], (1, 2, 3), 1)))
    out = net.draw_detections(dev, DETS, color=(9, 8, 7), thickness=-1, classes=lambda name: name != "human")
    assert np.array_equal(out.cpu().numpy(), W.paint(img.copy(), det_rects(DETS[:1] + DETS[2:], (9, 8, 7), -1)))
    assert torch.equal(net.draw_detections(dev, DETS, classes=()), dev) and torch.equal(net.draw_detections(dev, []), dev)
    same = net.draw_detections(dev, DETS, inplace=True)
    assert same.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy(), W.paint(img.copy(), det_rects(DETS, (255, 255, 255))))
    from_host = net.draw_detections(img, DETS)                                                # a NumPy image is uploaded, the array stays
    assert from_host.is_cuda and torch.equal(from_host, dev)


def test_write_predictions(R, png, tmp_path):
    net = R.RADNet(_Config(), None, None, None)
    img = np.random.RandomState(2).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    dev = torch.from_numpy(img).cuda()
    paths = net.write_predictions(DETS, dev, str(tmp_path / "out"))
    assert [os.path.basename(p) for p in paths] == ["all_predictions.png", "boat_predictions.png", "human_predictions.png", "other_predictions.png",
                                                    "predictions.json"]
    assert torch.equal(dev.cpu(), torch.from_numpy(img))
    for path, color, dets in zip(paths, ((255, 255, 255), (28, 26, 228), (184, 126, 55), (0, 127, 255)), (DETS, DETS[:1], DETS[1:2], DETS[2:])):
        want = W.paint(img.copy(), det_rects(dets, color))
        data = open(path, "rb").read()
        assert np.array_equal(W.decode_bgr(data), want), path
        assert np.array_equal(png.decode_device(data).cpu().numpy(), want), path
    with open(paths[-1]) as f:
        text = f.read()
    assert json.loads(text) == [{"label": d['class'], "confidence": float(d['prob']), "x1": int(d['x1']), "y1": int(d['y1']), "x2": int(d['x2']),
                                 "y2": int(d['y2'])} for d in DETS]
    assert text.startswith('[\n    {\n        "label": "boat",')                                # indent=4
    again = net.write_predictions(DETS, img, str(tmp_path / "again"))                          # a NumPy map: the same files
    for a, b in zip(paths, again):
        assert open(a, "rb").read() == open(b, "rb").read()
