"""RADNet.predict on an image that is already on the device (a uint8 [H][W][3] cuda tensor): every tile is a description
(RADNet.ImageWindow) that becomes one radnet_resize_bicubic_window_u8 launch, nothing image-sized goes back to the host.  The same
kernels see the same bytes, so predict([cuda_tensor]) must return exactly what predict([host_array]) returns: the same keys in the
same order, the same classes, np.array_equal values, the same Python and NumPy types -- the last block of
test_gpu_detect_tail._end_to_end, over device_tail, include_full_img, the download fallback, image sizes, predict_from_path and an
image made on another stream."""
import copy
import os

import numpy as np
import pytest

import png_cases as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _models():
    """As tests/test_gpu_detect_tail.py:_models."""
    from faster_rcnn import models as M
    from faster_rcnn.base_models import resnet50 as base
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    from oracle import dense
    Cc = Config()
    Cc.img_size = 300
    ms = M.build_models(Cc, weights=copy.deepcopy(dense.init_params(seed=3)), workload="predict")
    return Cc, ms, RADNet(Cc, ms[3], ms[4], base.preprocess)


def _noise(seed, shape):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    Cc, ms, rnet = _models()
    Cc.tile_size, Cc.tile_overlap = 400, 250           # 700 x 900: 3 x 3 tiles, last row and column clipped to the far edge
    assert Cc.max_n_tiles_train > 0
    Cc.include_full_img = True
    rnet.bbox_threshold = 0.0
    img = _noise(41, (700, 900, 3))
    rnet.device_tail, rnet.device_resident = True, True
    want = rnet.predict([img])                          # the reference of most tests: computed once, never changed
    assert len(want) > 0
    return Cc, ms, rnet, img, want


@pytest.fixture()
def net(setup):
    """The shared net with its switches at their defaults for this module, whatever the previous test left."""
    Cc, ms, rnet, img, want = setup
    Cc.include_full_img, Cc.use_img_type = True, False
    rnet.device_tail, rnet.device_resident = True, True
    rnet.bbox_threshold = 0.0
    return setup


def same_dets(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for key in x:
            assert type(x[key]) is type(y[key]), (key, type(x[key]), type(y[key]))
            assert np.array_equal(x[key], y[key]), (key, x[key], y[key])


def test_tiling_of_the_test_image(net):
    from faster_rcnn.RADNet import _spans
    assert _spans(700, 400, 250) == [(0, 400), (250, 650), (300, 700)]
    assert _spans(900, 400, 250) == [(0, 400), (250, 650), (500, 900)]


@pytest.mark.parametrize("device_tail", [True, False])
@pytest.mark.parametrize("full", [True, False])
def test_device_image_equals_host_image(net, device_tail, full):
    Cc, ms, rnet, img, want = net
    rnet.device_tail = device_tail
    Cc.include_full_img = full
    ref = want if (device_tail and full) else rnet.predict([img])
    assert len(ref) > 0
    same_dets(rnet.predict([torch.from_numpy(img).cuda()]), ref)


def test_download_fallback_without_device_resident(net):
    Cc, ms, rnet, img, want = net
    rnet.device_resident = False
    ref = rnet.predict([img])
    assert len(ref) > 0
    same_dets(rnet.predict([torch.from_numpy(img).cuda()]), ref)
    same_dets(ref, want)                                # and the NumPy-facing path gives the device-resident path's detections


@pytest.mark.parametrize("shape", [(400, 400, 3), (233, 310, 3)], ids=["exactly_one_tile", "smaller_than_a_tile"])
def test_single_tile_images(net, shape):
    Cc, ms, rnet, img, want = net
    small = _noise(43, shape)
    for tail in (True, False):
        rnet.device_tail = tail
        ref = rnet.predict([small])
        assert len(ref) > 0
        same_dets(rnet.predict([torch.from_numpy(small).cuda()]), ref)


def test_image_at_network_size_is_handed_on(net, monkeypatch):
    """300 x 300 at img_size 300 and a tile that covers it: contiguous and at the target size, no resize launch at all."""
    import faster_rcnn.RADNet as R
    Cc, ms, rnet, img, want = net
    small = _noise(44, (300, 300, 3))
    ref = rnet.predict([small])
    assert len(ref) > 0
    calls = []
    real = R.resize_cubic_window
    monkeypatch.setattr(R, "resize_cubic_window", lambda *a, **kw: calls.append(a[1:7]) or real(*a, **kw))
    same_dets(rnet.predict([torch.from_numpy(small).cuda()]), ref)
    assert calls == []


@pytest.mark.parametrize("device_tail", [True, False])
def test_no_host_round_trip_and_one_launch_per_window(net, monkeypatch, device_tail):
    import faster_rcnn.RADNet as R
    Cc, ms, rnet, img, want = net
    rnet.device_tail = device_tail
    ref = want if device_tail else rnet.predict([img])

    def refuse(*a, **kw):
        raise AssertionError("resize_cubic (host tile upload) called on the device-image path")

    calls = []
    real = R.resize_cubic_window

    def counted(img_dev, x0, y0, ww, wh, new_w, new_h, ctx=None):
        calls.append((x0, y0, ww, wh, new_w, new_h))
        assert ctx is not None                          # every window is resized on an engine lane
        return real(img_dev, x0, y0, ww, wh, new_w, new_h, ctx=ctx)

    monkeypatch.setattr(R, "resize_cubic", refuse)
    monkeypatch.setattr(R, "resize_cubic_window", counted)
    dev = torch.from_numpy(img).cuda()
    got = rnet.predict([dev])
    monkeypatch.undo()
    same_dets(got, ref)
    assert len(calls) == 9 + 1
    assert calls[:9] == [(x0, y0, 400, 400, 300, 300) for y0 in (0, 250, 300) for x0 in (0, 250, 500)]
    assert calls[9] == (0, 0, 900, 700, 385, 300)       # the full image: 700 x 900 -> 300 x 385


def _write_png(tmp_path, img, img_type):
    os.makedirs(tmp_path / img_type)
    enc = K.encode(img[:, :, ::-1], 2, 8, filters="adaptive")          # samples are R, G, B; the decoder returns B, G, R
    (tmp_path / img_type / "scan.png").write_bytes(enc.data)


def test_predict_from_path_stays_on_the_device(net, tmp_path, monkeypatch):
    import faster_rcnn.RADNet as R
    from faster_rcnn import png, utils_io
    Cc, ms, rnet, img, want = net
    Cc.img_types = ["blended_grey"]
    _write_png(tmp_path, img, "blended_grey")
    monkeypatch.chdir(tmp_path.parent)
    rel = tmp_path.name + "/scan.png"                                   # the type becomes path component 1
    assert np.array_equal(utils_io.get_image(rel, Cc.img_types), img)
    same_dets(rnet.predict_from_path(rel), want)
    monkeypatch.setattr(R, "resize_cubic", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("resize_cubic called")))
    monkeypatch.setattr(png, "imdecode_color", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("image decoded to the host")))
    same_dets(rnet.predict_from_path(rel), want)
    monkeypatch.undo()
    monkeypatch.chdir(tmp_path.parent)
    rnet.device_resident = False                                        # as before: host arrays
    same_dets(rnet.predict_from_path(rel), want)


def test_image_made_on_another_stream(net):
    Cc, ms, rnet, img, want = net
    pinned = torch.from_numpy(img).pin_memory()
    with torch.cuda.stream(torch.cuda.Stream()):
        dev = pinned.to("cuda", non_blocking=True)                      # in flight on this stream when predict starts
        got = rnet.predict([dev])
    same_dets(got, want)


def test_refused_device_images_raise_before_any_launch(net, monkeypatch):
    import faster_rcnn.RADNet as R
    Cc, ms, rnet, img, want = net
    good = torch.from_numpy(img).cuda()
    bad = {
        "uint8": good.float(),
        "rank": good[:, :, 0].contiguous(),
        "channels": torch.zeros((64, 64, 4), dtype=torch.uint8, device="cuda"),
        "contiguous": good[:, ::2, :],
    }
    assert not bad["contiguous"].is_contiguous()

    def no_work(*a, **kw):
        raise AssertionError("device work started before the images were checked")

    monkeypatch.setattr(R, "resize_cubic_window", no_work)
    monkeypatch.setattr(R, "resize_cubic", no_work)
    monkeypatch.setattr(rnet, "_detect_sharded", no_work)
    for word, t in bad.items():
        with pytest.raises((TypeError, ValueError), match=word):
            rnet.predict([t])
        with pytest.raises((TypeError, ValueError), match=word):
            rnet.predict([good, t])                     # a good image first: still nothing starts
