"""The device-resident augmentation (csrc/augment.hip through the C ABI, faster_rcnn/augmentation_device.py, TileFeed(device_augment=True),
TrainStep on device samples) against the host path it mirrors (faster_rcnn/augmentation.py, byte for byte outside the noise modes)
and, for the noise modes, against the NumPy restatement of the Philox field definition in tests/aug_device_cases.py."""
import copy

import numpy as np
import pytest

import aug_device_cases as K

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED = 0x5eed0123456789ab
SIZE_IDS = ["%dx%d" % s for s in K.SIZES]


@pytest.fixture(scope="module")
def ctx():
    from radnet_hip import runtime as rt
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return rt.default_context()


@pytest.fixture(scope="module")
def AD():
    from faster_rcnn import augmentation_device
    return augmentation_device


def dev(img):
    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def host(t):
    return t.cpu().numpy()


def variants(h, w):
    return [K.image(h, w, 10 * h + w, "border"), K.image(h, w, 10 * h + w + 1, "full")]


# ---- kernels ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
def test_gather_all_transforms_and_windows(ctx, AD, size):
    h, w = size
    img = K.image(h, w, 1, "full")
    d = dev(img)
    for window in K.windows(h, w):
        for t in range(8):
            got = host(AD.gather(ctx, d, t, window))
            assert np.array_equal(got, K.dihedral(img, window, t)), (window, t)


def test_gather_names_match_the_host_functions(ctx, AD):
    from faster_rcnn import augmentation as A
    img = K.image(37, 53, 2)
    d = dev(img)
    assert np.array_equal(host(AD.gather(ctx, d, AD.FLIP_COLS)), A.flip_u8(img, 1))
    assert np.array_equal(host(AD.gather(ctx, d, AD.FLIP_ROWS)), A.flip_u8(img, 0))
    assert np.array_equal(host(AD.gather(ctx, d, AD.FLIP_BOTH)), A.flip_u8(img, -1))
    assert np.array_equal(host(AD.gather(ctx, d, AD.ROT90)), A.flip_u8(np.transpose(img, (1, 0, 2)), 1))
    assert np.array_equal(host(AD.gather(ctx, d, AD.ROT270)), A.flip_u8(np.transpose(img, (1, 0, 2)), 0))
    with pytest.raises(Exception):                                       # a window outside the image is refused, not read
        AD.gather(ctx, d, 0, (30, 0, 8, 53))


@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
def test_extent_equals_strap_img(ctx, AD, size):
    from faster_rcnn import augmentation as A
    h, w = size
    for img in variants(h, w):
        if not img[:, :, 1].any():
            img[h // 2, w // 2, 1] = 9
        assert AD.extent(ctx, dev(img)) == tuple(int(v) for v in A.strap_img(img))
    one = np.zeros((h, w, 3), np.uint8)
    one[h - 1, w // 2, 1] = 1                                            # a single non-zero pixel
    assert AD.extent(ctx, dev(one)) == (h - 1, h - 1, w // 2, w // 2)
    one[:, :, 1] = 0
    one[0, 0, 0] = one[0, 0, 2] = 200                                    # other channels do not count
    with pytest.raises(ValueError) as dev_err:
        AD.extent(ctx, dev(one))
    with pytest.raises(ValueError) as host_err:
        A.strap_img(one)
    assert str(dev_err.value) == str(host_err.value)


@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
def test_histogram_equals_bincount(ctx, AD, size):
    for img in variants(*size):
        d = dev(img)
        assert np.array_equal(AD.histogram(ctx, d, False), np.bincount(img[:, :, 0].ravel(), minlength=256))
        assert np.array_equal(AD.histogram(ctx, d, True), np.bincount(img.ravel(), minlength=256))


def brightness_ref(img, delta, darker):
    f = img.astype("float32")
    if darker:
        f -= np.float32(delta)
    else:
        f += np.float32(delta)
    out = np.clip(f, 0, 255).astype("uint8")
    out[img == 0] = 0
    return out


@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
def test_brightness_both_directions_and_saturation(ctx, AD, size):
    from radnet_hip.lib import AUG_BRIGHTNESS
    for img in variants(*size):
        d = dev(img)
        for delta, darker in ((17.31, True), (52.9, False), (300.0, True), (254.5, False), (0.0, True)):
            got = host(AD.pointwise(ctx, d, AUG_BRIGHTNESS, float(np.float32(delta)), 1.0 if darker else 0.0))
            assert np.array_equal(got, brightness_ref(img, delta, darker)), (delta, darker)


@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
def test_contrast_equals_rescale_intensity(ctx, AD, size):
    from faster_rcnn import augmentation as A
    from radnet_hip.lib import AUG_CONTRAST
    for img in variants(*size):
        d = dev(img)
        for lo, hi in ((31.7, 201.3), (0.0, 255.0), (74.99, 180.0), (0.5, 0.5), (1.0, 1.0)):
            got = host(AD.pointwise(ctx, d, AUG_CONTRAST, lo, hi))
            assert np.array_equal(got, A.rescale_intensity(img, (lo, hi))), (lo, hi)


@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("grey", [True, False], ids=["grey", "per_channel"])
def test_salt_and_pepper_equals_restatement(ctx, AD, size, grey):
    from radnet_hip.lib import AUG_SALT_PEPPER
    for img in variants(*size):
        d = dev(img)
        for amount in (0.01, 0.3):
            for field_id in (0, 7):
                got = host(AD.pointwise(ctx, d, AUG_SALT_PEPPER, amount, 0.4, grey, SEED, field_id))
                assert np.array_equal(got, K.noise(img, "s&p", grey, amount, 0.4, SEED, field_id)), (amount, field_id)
    big = K.image(64, 61, 5, "full")
    a = host(AD.pointwise(ctx, dev(big), AUG_SALT_PEPPER, 0.3, 0.4, grey, SEED, 0))
    b = host(AD.pointwise(ctx, dev(big), AUG_SALT_PEPPER, 0.3, 0.4, grey, SEED, 7))
    assert not np.array_equal(a, b)                                      # the field id does select another field


def one_level_on_few_pixels(got, ref, what):
    """Zero differing pixels is expected.  The device's log / cos / exp are within 1 ulp of NumPy's but not the same code: a case
    may differ by one grey level on at most 1 pixel in 10^4, and by nothing larger."""
    diff = np.abs(got.astype(np.int16) - ref.astype(np.int16))
    n_pix = int((diff.max(axis=2) > 0).sum())
    print("%s: %d of %d pixels differ, largest difference %d" % (what, n_pix, diff.shape[0] * diff.shape[1], int(diff.max()) if diff.size else 0))
    assert diff.size == 0 or diff.max() <= 1, what
    assert n_pix * 10 ** 4 <= diff.shape[0] * diff.shape[1], what


@pytest.mark.parametrize("size", K.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("grey", [True, False], ids=["grey", "per_channel"])
def test_gaussian_and_poisson_equal_restatement(ctx, AD, size, grey):
    from radnet_hip.lib import AUG_GAUSSIAN, AUG_POISSON
    for i, img in enumerate(variants(*size)):
        d = dev(img)
        for mean, var, field_id in ((0.0312, 0.0071, 0), (-0.05, 0.001, 7)):
            sigma = float(np.sqrt(var))
            got = host(AD.pointwise(ctx, d, AUG_GAUSSIAN, mean, sigma, grey, SEED, field_id))
            one_level_on_few_pixels(got, K.noise(img, "gaussian", grey, mean, sigma, SEED, field_id), "gaussian %s %d" % (size, i))
        for v, field_id in ((K.poisson_v(img, grey), 0), (16.0, 7)):
            got = host(AD.pointwise(ctx, d, AUG_POISSON, v, 0.0, grey, SEED, field_id))
            one_level_on_few_pixels(got, K.noise(img, "poisson", grey, v, 0.0, SEED, field_id), "poisson %s %d v=%g" % (size, i, v))


def test_reductions_beyond_their_grid_cap(ctx, AD):
    """The extent and the histogram run on a capped grid (1024 workgroups of 256 threads) and stride over the rest; the gather and
    the pointwise kernel launch one thread per pixel, uncapped.  1500 x 1500 pixels: every thread of the capped grids loops."""
    from radnet_hip.lib import AUG_BRIGHTNESS
    h, w = K.LARGE
    rs = np.random.RandomState(77)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[:11] = 0
    img[-3:] = 0
    img[:, :7] = 0
    img[:, -20:] = 0
    d = dev(img)
    assert AD.extent(ctx, d) == (11, h - 4, 7, w - 21)
    assert np.array_equal(AD.histogram(ctx, d, False), np.bincount(img[:, :, 0].ravel(), minlength=256))
    assert np.array_equal(AD.histogram(ctx, d, True), np.bincount(img.ravel(), minlength=256))
    assert np.array_equal(host(AD.gather(ctx, d, AD.ROT90, (11, 7, h - 14, w - 27))), K.dihedral(img, (11, 7, h - 14, w - 27), AD.ROT90))
    assert np.array_equal(host(AD.pointwise(ctx, d, AUG_BRIGHTNESS, 40.0, 1.0)), brightness_ref(img, 40.0, True))


# ---- the chain -------------------------------------------------------------------------------------------------------------------

def config(noise, grey=True):
    from faster_rcnn.config import Config
    C = Config()
    C.use_noise = noise
    C.img_types = ["enhanced_topo_grey", "topo_grey"] if grey else ["rgb", "topo"]
    return C


def chain_case(seed):
    h, w = K.CHAIN_SIZES[seed % len(K.CHAIN_SIZES)]
    img = K.image(h, w, 500 + seed, "full" if seed % 5 == 4 else "border")
    data = {"filepath": "t%d.png" % seed, "bboxes": K.boxes(h, w, seed), "width": w, "height": h}
    return img, data


def test_chain_without_noise_equals_host(AD):
    from faster_rcnn import augmentation as A
    C = config(False)
    applied = 0
    for seed in range(40):
        img, data = chain_case(seed)
        rng_h, rng_d = np.random.RandomState(seed), np.random.RandomState(seed)
        want, want_img = A.augment(copy.deepcopy(data), img, C, rng=rng_h)
        got, got_img = AD.augment_device(copy.deepcopy(data), dev(img), C, rng=rng_d)
        assert got == want, seed
        assert got_img.is_cuda and got_img.dtype == torch.uint8
        assert np.array_equal(host(got_img), want_img), seed
        assert (got["width"], got["height"]) == (got_img.shape[1], got_img.shape[0])
        sh, sd = rng_h.get_state(), rng_d.get_state()
        assert np.array_equal(sh[1], sd[1]) and sh[2:] == sd[2:], seed
        applied += int(want_img.shape != img.shape or not np.array_equal(want_img, img))
    assert applied >= 30                                                 # the seeds do exercise the chain


def test_chain_with_noise_draws_as_host_and_fields_as_defined(AD):
    from faster_rcnn import augmentation as A
    modes = set()
    for seed in range(16):
        grey = seed % 2 == 0
        C, C0 = config(True, grey), config(False, grey)
        img, data = chain_case(100 + seed)
        rng_h, rng_d, rng_p = (np.random.RandomState(seed) for _ in range(3))
        want, want_img = A.augment(copy.deepcopy(data), img, C, rng=rng_h, noise_rng=np.random.default_rng(seed))
        got, got_img = AD.augment_device(copy.deepcopy(data), dev(img), C, rng=rng_d, noise_seed=SEED, field_id=seed)
        assert got == want and tuple(got_img.shape) == want_img.shape, seed
        sh, sd = rng_h.get_state(), rng_d.get_state()
        assert np.array_equal(sh[1], sd[1]) and sh[2:] == sd[2:], seed
        # the image just before the noise step: the same chain with the noise switch off, then the noise draws replayed
        _, pre = AD.augment_device(copy.deepcopy(data), dev(img), C0, rng=rng_p)
        pre = host(pre)
        ref = pre
        if rng_p.random() < 0.5:
            which = rng_p.randint(0, 4)
            modes.add(int(which))
            if which == 0:
                amount = (0.3 - 0.01) * rng_p.random() + 0.01
                svp = A.get_truncated_normal(mean=0.5, sd=0.1, low=0, upp=1).rvs(size=1, random_state=rng_p)[0]
                ref = K.noise(pre, "s&p", grey, amount, svp, SEED, seed)
            elif which == 1:
                mean = (0.05 + 0.05) * rng_p.random() - 0.05
                var = (0.01 - 0.001) * rng_p.random() + 0.001
                ref = K.noise(pre, "gaussian", grey, mean, float(np.sqrt(var)), SEED, seed)
            elif which == 2:
                ref = K.noise(pre, "poisson", grey, K.poisson_v(pre, grey), 0.0, SEED, seed)
            else:
                lo = 75 * rng_p.random()
                ref = A.rescale_intensity(pre, (lo, (255 - 180) * rng_p.random() + 180))
        sp = rng_p.get_state()
        assert np.array_equal(sp[1], sd[1]) and sp[2:] == sd[2:], seed
        one_level_on_few_pixels(host(got_img), ref, "chain seed %d" % seed)
    assert modes == {0, 1, 2, 3}


# ---- the feed and the step -------------------------------------------------------------------------------------------------------

def feed_pair(background):
    from faster_rcnn import data_feed as F
    from test_data_feed import CLASSES, dataset
    C = config(False, grey=False)
    C.img_size, C.tile_size, C.tile_overlap, C.balanced_classes = 300, 300, 150, False
    C.max_n_tiles_train = 2
    data, imgs = dataset(3, [(640, 480), (300, 300), (500, 620)])
    cc = {c: 1 for c in CLASSES}
    load = lambda d, t: imgs[d["filepath"]]
    mk = lambda **kw: F.TileFeed([dict(d) for d in data], C, cc, load, rng=np.random.RandomState(5), **kw)
    feeds = [mk(), mk(device_augment=True)]
    return [F.BackgroundFeed(f, depth=3) for f in feeds] if background else feeds


def take(feed, n, device):
    out = []
    for s in feed:
        if device:
            assert isinstance(s["img"], torch.Tensor) and s["img"].is_cuda and s["img"].dtype == torch.uint8
        img = host(s["img"]) if device else s["img"]
        out.append((s["filepath"], s["width"], s["height"], [tuple(sorted(b.items())) for b in s["bboxes"]], img))
        if len(out) == n:
            break
    return out


@pytest.mark.parametrize("background", [False, True], ids=["direct", "background_feed"])
def test_tile_feed_device_path_yields_the_host_path_samples(background):
    ref_feed, dev_feed = feed_pair(background)
    try:
        ref, got = take(ref_feed, 12, False), take(dev_feed, 12, True)
    finally:
        if background:
            ref_feed.close()
            dev_feed.close()
    assert len(ref) == len(got) == 12
    for k, (a, b) in enumerate(zip(ref, got)):
        assert a[:4] == b[:4], k
        assert a[4].shape == b[4].shape and np.array_equal(a[4], b[4]), k
    assert len({a[4].shape for a in ref}) >= 1 and any(a[4].shape[:2] != (300, 300) for a in ref)      # rotation / shear changed sizes


def test_validation_feed_device_path_crops_and_resizes_only():
    from faster_rcnn import data_feed as F
    from test_data_feed import CLASSES, dataset
    C = config(True, grey=False)
    C.img_size, C.tile_size, C.tile_overlap, C.balanced_classes, C.max_n_tiles_val = 200, 300, 150, False, 3
    data, imgs = dataset(3, [(640, 480), (500, 620)])
    cc = {c: 1 for c in CLASSES}
    load = lambda d, t: imgs[d["filepath"]]
    mk = lambda **kw: F.TileFeed([dict(d) for d in data], C, cc, load, train_mode=False, rng=np.random.RandomState(5), **kw)
    ref, got = take(mk(), 100, False), take(mk(device_augment=True, noise_seed=1), 100, True)
    assert len(ref) == len(got) > 0
    for a, b in zip(ref, got):
        assert a[:4] == b[:4] and np.array_equal(a[4], b[4]) and a[4].shape[:2] == (200, 200)


def test_train_step_on_a_device_sample_is_bit_identical():
    """TrainStep.step on a sample whose image is already on the device (a device-to-device copy into the plan's raw panel) against the
    same sample downloaded to the host (pinned staging): the same losses, bit for bit.  The cont_train trainer and NativeTrainStep
    refuse device samples with a TypeError."""
    import tempfile
    from faster_rcnn.config import Config
    from radnet_hip import synth
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.native import NativeTrainStep
    from radnet_hip.trainer import TrainStep
    C = Config()
    C.img_size = 300
    W = synth.synthetic_weights(seed=3)
    img = synth.synthetic_panel(1, 300, 500)
    meta = synth.synthetic_gt(2, n=6, src_w=1000, src_h=600, smin=60, smax=300)
    on_device = dev(img)
    tune = tempfile.mktemp(suffix=".txt")
    losses = []
    for k, panel in enumerate((np.ascontiguousarray(host(on_device)), on_device)):
        eng = FasterRCNNEngine(C)
        if k:
            eng.load_tuning(tune)                  # same launch shapes -> same summation order
        eng.set_weights(W)
        np.random.seed(64)
        ts = TrainStep(eng)
        ts.step([dict(img=panel, bboxes=copy.deepcopy(meta["bboxes"]), width=1000, height=600)])
        losses.append(ts.losses())
        ts.flush()
        if not k:
            eng.save_tuning(tune)
    assert losses[0] == losses[1], losses
    assert losses[0]["rpn_cls"] > 0
    with pytest.raises(TypeError):
        NativeTrainStep(eng).step(dict(img=on_device, bboxes=meta["bboxes"], width=1000, height=600))
