"""csrc/resize.hip, radnet_resize_bicubic_window_u8 through the C ABI: the tile cut and the resize in one launch.  The contract is
that dst holds exactly the bytes radnet_resize_bicubic_u8 writes for a contiguous copy of the window, so every comparison is BIT FOR
BIT against oracle.resize.resize_bicubic_u8(np.ascontiguousarray(img[y0:y0+wh, x0:x0+ww]), dw, dh).  The source is noise: a tap
that reads a pixel beyond the window (a clamp to the image's extent instead of the window's) changes the output."""
import numpy as np
import pytest

from oracle import resize as OR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SH, SW = 97, 131
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from radnet_hip import lib as L
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    c = L.Context(0)
    yield c
    c.close()


def noise(ch, seed=5):
    return np.random.RandomState(seed + ch).randint(0, 256, (SH, SW, ch)).astype(np.uint8)


def window_call(ctx, src, sh, sw, y0, x0, wh, ww, dst, dh, dw, ch):
    ctx.call("radnet_resize_bicubic_window_u8", src, sh, sw, y0, x0, wh, ww, dst, dh, dw, ch)


def gpu_window(ctx, img, y0, x0, wh, ww, dw, dh):
    src = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    dst = torch.full((dh, dw, img.shape[2]), SENTINEL, dtype=torch.uint8, device="cuda")
    window_call(ctx, src, img.shape[0], img.shape[1], y0, x0, wh, ww, dst, dh, dw, img.shape[2])
    ctx.sync()
    return dst.cpu().numpy()


def want(img, y0, x0, wh, ww, dw, dh):
    return OR.resize_bicubic_u8(np.ascontiguousarray(img[y0:y0 + wh, x0:x0 + ww]), dw, dh)


CASES = [  # (y0, x0, wh, ww, dh, dw, channels, what)
    (17, 23, 61, 83, 23, 31, 3, "interior_down"),            # real pixels on all four sides of the window
    (17, 23, 61, 83, 140, 197, 3, "interior_up_noninteger"),
    (17, 23, 61, 83, 61, 83, 3, "interior_identity"),
    (0, 0, 40, 50, 71, 93, 3, "corner_top_left"),
    (0, SW - 50, 40, 50, 71, 93, 3, "corner_top_right"),
    (SH - 40, 0, 40, 50, 71, 93, 3, "corner_bottom_left"),
    (SH - 40, SW - 50, 40, 50, 17, 29, 3, "corner_bottom_right"),
    (40, 60, 1, 1, 5, 7, 3, "one_pixel"),                     # every tap clamps inside the window
    (30, 60, 33, 1, 50, 6, 3, "one_pixel_wide"),
    (40, 20, 1, 45, 4, 77, 3, "one_pixel_high"),
    (11, 37, 30, 41, 47, 59, 1, "odd_x0_c1"),                 # the window's first byte is not 4-byte aligned
    (11, 37, 30, 41, 47, 59, 3, "odd_x0_c3"),
    (20, 30, 37, 29, 19, 53, 1, "c1"),
    (20, 30, 37, 29, 19, 53, 4, "c4"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[-1] for c in CASES])
def test_window_bit_exact_vs_oracle_on_the_copied_window(ctx, case):
    y0, x0, wh, ww, dh, dw, ch, what = case
    img = noise(ch)
    if what.startswith("odd_x0"):
        assert ((y0 * SW + x0) * ch) % 4 != 0
    got = gpu_window(ctx, img, y0, x0, wh, ww, dw, dh)
    ref = want(img, y0, x0, wh, ww, dw, dh)
    assert got.shape == ref.shape and got.dtype == np.uint8
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, "%d differing bytes, first at %s: gpu %d oracle %d" % (len(bad), bad[0], got[tuple(bad[0])], ref[tuple(bad[0])])
    if (wh, ww) == (dh, dw):
        assert np.array_equal(got, img[y0:y0 + wh, x0:x0 + ww])        # identity: the window's bytes


def test_pixels_outside_the_window_do_not_matter(ctx):
    """Everything outside the window redrawn: the output is the same bytes (up-scaled, so the border taps do leave the window)."""
    img = noise(3)
    y0, x0, wh, ww = 17, 23, 61, 83
    other = noise(3, seed=77)
    other[y0:y0 + wh, x0:x0 + ww] = img[y0:y0 + wh, x0:x0 + ww]
    assert not np.array_equal(other, img)
    a = gpu_window(ctx, img, y0, x0, wh, ww, 197, 140)
    assert np.array_equal(a, gpu_window(ctx, other, y0, x0, wh, ww, 197, 140))
    assert np.array_equal(a, want(img, y0, x0, wh, ww, 197, 140))


@pytest.mark.parametrize("dh,dw", [(SH, SW), (41, 59), (150, 211)])
def test_whole_image_window_equals_the_plain_resize(ctx, dh, dw):
    img = noise(3)
    src = torch.from_numpy(img).cuda()
    plain = torch.zeros((dh, dw, 3), dtype=torch.uint8, device="cuda")
    ctx.call("radnet_resize_bicubic_u8", src, SH, SW, plain, dh, dw, 3)
    win = torch.zeros((dh, dw, 3), dtype=torch.uint8, device="cuda")
    window_call(ctx, src, SH, SW, 0, 0, SH, SW, win, dh, dw, 3)
    ctx.sync()
    assert torch.equal(plain, win)
    assert np.array_equal(win.cpu().numpy(), OR.resize_bicubic_u8(img, dw, dh))


def test_window_borders_replicate_the_window_not_the_image(ctx):
    """Modelled on test_gpu_resize.test_borders_replicate: a constant window with a ring of another value just outside it.  Up-scaled,
    the window stays constant only if the out-of-range taps replicate the WINDOW's edge."""
    img = np.full((SH, SW, 3), 90, np.uint8)
    y0, x0, wh, ww = 30, 40, 25, 35
    img[y0 - 1:y0 + wh + 1, x0 - 1:x0 + ww + 1] = 200
    img[y0:y0 + wh, x0:x0 + ww] = 17
    got = gpu_window(ctx, img, y0, x0, wh, ww, 121, 83)
    assert np.array_equal(got, want(img, y0, x0, wh, ww, 121, 83))
    assert (got == 17).all()


REFUSED = [  # (y0, x0, wh, ww, dh, dw, what)
    (-1, 10, 20, 20, 9, 9, "negative_y0"),
    (10, -1, 20, 20, 9, 9, "negative_x0"),
    (-5, 10, 20, 20, 9, 9, "leaves_top"),
    (10, -5, 20, 20, 9, 9, "leaves_left"),
    (SH - 19, 10, 20, 20, 9, 9, "leaves_bottom"),
    (10, SW - 19, 20, 20, 9, 9, "leaves_right"),
    (10, 10, 0, 20, 9, 9, "zero_wh"),
    (10, 10, 20, 0, 9, 9, "zero_ww"),
    (10, 10, 20, 20, 0, 9, "zero_dh"),
    (10, 10, 20, 20, 9, 0, "zero_dw"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[-1] for c in REFUSED])
def test_refused_arguments_launch_nothing(ctx, case):
    """Argument checks return before any launch: the binding raises and a dst full of a sentinel is untouched."""
    from radnet_hip.lib import RadnetError
    y0, x0, wh, ww, dh, dw, what = case
    src = torch.from_numpy(noise(3)).cuda()
    dst = torch.full((16, 16, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    with pytest.raises(RadnetError):
        window_call(ctx, src, SH, SW, y0, x0, wh, ww, dst, dh, dw, 3)
    ctx.sync()
    assert (dst == SENTINEL).all()


def test_refused_null_pointers_extents_and_channels(ctx):
    from radnet_hip.lib import RadnetError
    src = torch.from_numpy(noise(3)).cuda()
    dst = torch.full((16, 16, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    for args in ((None, SH, SW, 1, 1, 8, 8, dst, 9, 9, 3), (src, SH, SW, 1, 1, 8, 8, None, 9, 9, 3),
                 (src, 0, SW, 0, 0, 1, 1, dst, 9, 9, 3), (src, SH, 0, 0, 0, 1, 1, dst, 9, 9, 3), (src, SH, SW, 1, 1, 8, 8, dst, 9, 9, 0)):
        with pytest.raises(RadnetError):
            window_call(ctx, *args)
    assert ctx.lib.radnet_resize_bicubic_window_u8(None, src.data_ptr(), SH, SW, 1, 1, 8, 8, dst.data_ptr(), 9, 9, 3) != 0
    ctx.sync()
    assert (dst == SENTINEL).all()
