"""Host-side checks of the device-resident augmentation (faster_rcnn/augmentation_device.py, csrc/augment.hip): the known
answers of the tests' own Philox restatement (tests/aug_device_cases.py), its distributions, the C ABI surface and TileFeed's
opt-in arguments.  No GPU; the kernels themselves are tested in test_gpu_augment_device.py."""
import numpy as np
import pytest

import aug_device_cases as K

AUG_SYMBOLS = ("radnet_aug_gather_u8", "radnet_aug_extent_u8", "radnet_aug_histogram_u8", "radnet_aug_pointwise_u8")
N = 10 ** 5


def test_philox_known_answers():
    for counter, key, want in K.PHILOX_KAT:
        got = K.philox4x32([np.array([c], dtype=np.uint64) for c in counter], key)
        assert tuple(int(g[0]) for g in got) == want
    # vectorised over the counter: element i of a field is its own block
    idx = np.array([0, 1, 2 ** 32 - 1], dtype=np.uint64)
    zero = np.zeros(3, dtype=np.uint64)
    many = K.philox4x32((idx, zero, zero + np.uint64(7), zero), (5, 9))
    for i in range(3):
        one = K.philox4x32([np.array([c], dtype=np.uint64) for c in (int(idx[i]), 0, 7, 0)], (5, 9))
        assert [int(m[i]) for m in many] == [int(o[0]) for o in one]


def test_uniforms_are_inside_the_unit_interval_and_keyed():
    ua, ub = K.uniforms(N, 0x0123456789abcdef, 3)
    assert ua.min() > 0.0 and ua.max() < 1.0 and ub.min() > 0.0 and ub.max() < 1.0
    assert not np.array_equal(ua, ub)
    assert not np.array_equal(ua, K.uniforms(N, 0x0123456789abcdef, 4)[0])          # another field
    assert not np.array_equal(ua, K.uniforms(N, 0x0123456789abcdee, 3)[0])          # another seed
    assert np.array_equal(ua, K.uniforms(N, 0x0123456789abcdef, 3)[0])
    for u in (ua, ub):                                                                # uniform: mean 1/2, variance 1/12
        assert abs(u.mean() - 0.5) < 5 * np.sqrt(1.0 / 12 / N)


@pytest.mark.parametrize("amount,svp", [(0.01, 0.5), (0.3, 0.35)])
def test_salt_and_pepper_rates(amount, svp):
    img = np.full((N // 100, 100, 3), 100, dtype=np.uint8)
    out = K.noise(img, "s&p", True, amount, svp, 11, 0)[:, :, 0]
    hit = out != 100
    assert abs(hit.mean() - amount) < 5 * np.sqrt(amount * (1 - amount) / N)
    n_hit = int(hit.sum())
    assert abs((out[hit] == 255).mean() - svp) < 5 * np.sqrt(svp * (1 - svp) / n_hit)
    assert set(np.unique(out)) <= {0, 100, 255}


def test_gaussian_moments():
    z = K.normal(*K.uniforms(N, 12, 1))
    assert abs(z.mean()) < 5 * np.sqrt(1.0 / N)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / (N - 1))
    # through the mode: mid-grey + N(mean, var), far from the clip, back in grey levels
    mean, var = 0.03, 0.004
    img = np.full((N // 100, 100, 3), 128, dtype=np.uint8)
    out = K.noise(img, "gaussian", True, mean, np.sqrt(var), 12, 1)[:, :, 0].astype(np.float64) / 255.0
    step = (1.0 / 255.0) ** 2 / 12.0                                                  # variance the rounding to grey levels adds
    assert abs(out.mean() - (128 / 255.0 + mean)) < 5 * np.sqrt((var + step) / N)
    assert abs(out.var() - (var + step)) < 5 * (var + step) * np.sqrt(2.0 / (N - 1))


@pytest.mark.parametrize("lam", [0.5, 32.0, 200.0])
def test_poisson_mean_and_variance(lam):
    ua, _ = K.uniforms(N, 13, 2)
    k = K.poisson_counts(np.full(N, lam), ua)
    assert abs(k.mean() - lam) < 5 * np.sqrt(lam / N)
    assert abs(k.var() - lam) < 5 * np.sqrt((lam + 2 * lam * lam) / N)               # Var(s^2) of a Poisson: (lam + 2 lam^2) / n
    assert k.min() >= 0 and k.max() < 1023


def test_noise_background_and_grey_handling():
    img = K.image(37, 53, 3)
    for mode, p0, p1 in (("s&p", 0.3, 0.5), ("gaussian", 0.0, 0.1), ("poisson", K.poisson_v(img, False), 0.0)):
        out = K.noise(img, mode, False, p0, p1, 5, 0)
        assert out.shape == img.shape and (out[img == 0] == 0).all() and not np.array_equal(out, img)
    out = K.noise(img, "gaussian", True, 0.0, 0.1, 5, 0)
    assert np.array_equal(out[:, :, 0], out[:, :, 1]) and np.array_equal(out[:, :, 0], out[:, :, 2])
    assert (out[img[:, :, 0] == 0] == 0).all()


def test_entry_points_declared_and_bound():
    import inspect
    from radnet_hip import lib as L
    declared = L.declared_symbols()
    table = inspect.getsource(L.load_library)
    for name in AUG_SYMBOLS:
        assert name in declared, name
        assert '"%s"' % name in table, name
    header = open(L.HEADER_PATH).read()
    for mode, value in (("BRIGHTNESS", L.AUG_BRIGHTNESS), ("CONTRAST", L.AUG_CONTRAST), ("SALT_PEPPER", L.AUG_SALT_PEPPER),
                        ("GAUSSIAN", L.AUG_GAUSSIAN), ("POISSON", L.AUG_POISSON)):
        assert "#define RADNET_AUG_%s %d\n" % (mode, value) in header


def test_tile_feed_device_arguments():
    import inspect
    from faster_rcnn import data_feed as F
    from faster_rcnn.config import Config
    sig = inspect.signature(F.TileFeed.__init__)
    assert sig.parameters["device_augment"].default is False and sig.parameters["noise_seed"].default is None
    C = Config()
    assert C.use_noise
    feed = F.TileFeed([], C, {"boat": 1}, None, resize=lambda im, w, h: im)
    assert feed.device_augment is False and feed.warp is None
    with pytest.raises(ValueError):
        F.TileFeed([], C, {"boat": 1}, None, device_augment=True, noise_seed=1, resize=lambda im, w, h: im)
    with pytest.raises(ValueError):
        F.TileFeed([], C, {"boat": 1}, None, device_augment=True)                    # C.use_noise without a noise_seed
    assert F.TileFeed([], C, {"boat": 1}, None, device_augment=True, noise_seed=0).warp is None
    C.use_noise = False
    assert F.TileFeed([], C, {"boat": 1}, None, device_augment=True).device_augment is True


def test_extracted_box_helpers_are_what_the_host_functions_run():
    """The box arithmetic the device path shares with the host path: any_degree_rotation / shear go through the same helpers."""
    from faster_rcnn import augmentation as A
    img = K.image(61, 64, 8)
    bx = K.boxes(61, 64, 8)
    seen = {}

    def warp(im, mat, dsize):
        seen["mat"], seen["dsize"] = np.array(mat), tuple(dsize)
        return A.warp_affine_u8(im, mat, dsize)

    out, got = A.any_degree_rotation(img, [dict(b) for b in bx], rng=np.random.RandomState(2), warp=warp)
    angle = np.random.RandomState(2).uniform(-3.0, 3.0)
    mat, dsize = A._rotation_plan(61, 64, angle)
    assert np.array_equal(mat, seen["mat"]) and dsize == seen["dsize"]
    ext = A.strap_img(A.warp_affine_u8(img, mat, dsize))
    assert got == A._strapped_rotation_boxes([dict(b) for b in bx], A._rotated_hulls(A._boxes_array(bx), mat), ext)
