"""augmentation.augment (augmentation.py:481-533) for a tile that is already on the device: the same coins in the same order
from `rng`, the same thresholds, the same box arithmetic -- the host module's own box code is called, not restated -- and every
image operation one launch of csrc/augment.hip (index gather, strap extent, histogram, pointwise modes), of
radnet_warp_affine_u8 (the +-3 degree rotation, the shear) or of radnet_resize_bicubic_u8 (the feed's final resize).  The image
crosses PCIe once, upward; what comes back is what a decision needs: four ints after each warp (the strap), one kilobyte of
histogram before brightness (its mean decides whether and what it draws) and before the poisson mode (its `v`).

What "same as the host path" means:
  every switch but the three noise modes   equal to augmentation.augment on the same inputs and `rng`: image bytes, boxes,
                                           width / height, the position of `rng` afterwards.
  brightness                               the foreground mean is np.float32(sum) / np.float32(count) from the EXACT integer sum
      and count of the non-zero elements, i.e. the correctly rounded mean.  NumPy's float32 pairwise mean is exact while the sum
      of the elements stays below 2^24; on larger tiles it is not (2000 x 2000 x 3 noise: NumPy 127.965996, exact 127.96607), so
      outputs can then differ from the host's by one grey level at isolated pixels.  NumPy's summation order is not emulated.
  salt-and-pepper / gaussian / poisson     same draws from `rng`, same boxes, same background restore and grey-mode handling; the
      pixel values come from the device's own reproducible field, Philox4x32-10 keyed by `noise_seed` with the element index and
      `field_id` (the sample's ordinal in the feed) as counter -- defined in include/radnet_hip.h.  scikit-image draws the
      reference's field from a generator the reference never seeds: only the distribution is specified (augmentation.py header).
"""
import contextlib
import copy
import ctypes

import numpy as np

from radnet_hip.lib import AUG_BRIGHTNESS, AUG_CONTRAST, AUG_GAUSSIAN, AUG_POISSON, AUG_SALT_PEPPER

from . import augmentation as A

IDENTITY, FLIP_ROWS, FLIP_COLS, FLIP_BOTH, TRANSPOSE, ROT270, ROT90, ANTI_TRANSPOSE = range(8)      # radnet_aug_gather_u8 transforms
_ROT = {90: ROT90, 180: FLIP_BOTH, 270: ROT270}


@contextlib.contextmanager
def feed_stream(ctx=None):
    """(context, side stream) for device work of the feed: the calling thread's default context, and -- on a BackgroundFeed worker
    thread -- that thread's own stream made current, as RADNet.resize_cubic does.  hand_over() passes a result to the consumer."""
    import torch
    from radnet_hip import runtime as rt
    own = ctx is None
    ctx = rt.default_context() if own else ctx
    side = rt.thread_stream() if own else None
    with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        yield ctx, side


def hand_over(t, side):
    """A device result made on the worker's stream: its consumer's stream waits, and the caching allocator is told that the memory
    is in use there too (see RADNet.resize_cubic)."""
    import torch
    if side is not None:
        torch.cuda.current_stream().wait_stream(side)
        t.record_stream(torch.cuda.current_stream())
    return t


def _empty(h, w):
    import torch
    return torch.empty((int(h), int(w), 3), dtype=torch.uint8, device="cuda")


def _check(img):
    import torch
    if not (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
            and img.is_contiguous()):
        raise TypeError("device augmentation takes a contiguous uint8 HWC cuda tensor with 3 channels")
    return img


def gather(ctx, img, transform=IDENTITY, window=None):
    """radnet_aug_gather_u8: the window (y0, x0, height, width; default: the whole image) of `img` under a dihedral transform."""
    sh, sw = img.shape[:2]
    y0, x0, wh, ww = (0, 0, sh, sw) if window is None else (int(v) for v in window)
    out = _empty(ww, wh) if transform & 4 else _empty(wh, ww)
    if out.numel():
        ctx.call("radnet_aug_gather_u8", img, sh, sw, y0, x0, wh, ww, int(transform), out)
    return out


def extent(ctx, img):
    """strap_img on the device: (row_min, row_max, col_min, col_max) of the pixels whose channel 1 is non-zero; four ints come back."""
    import torch
    out = torch.empty(4, dtype=torch.int32, device="cuda")
    ctx.call("radnet_aug_extent_u8", img, img.shape[0], img.shape[1], out)
    r0, r1, c0, c1 = (int(v) for v in out.cpu().numpy())
    if r1 < 0:
        raise ValueError("zero-size array to reduction operation minimum which has no identity")      # strap_img's, of r.min()
    return r0, r1, c0, c1


def histogram(ctx, img, all_channels):
    """256 bins (int64 on the host) over channel 0 or over all three channels; one kilobyte comes back."""
    import torch
    bins = torch.empty(256, dtype=torch.int32, device="cuda")
    ctx.call("radnet_aug_histogram_u8", img, img.shape[0], img.shape[1], 1 if all_channels else 0, bins)
    return bins.cpu().numpy().view(np.uint32).astype(np.int64)


def pointwise(ctx, img, mode, p0=0.0, p1=0.0, grey=False, noise_seed=0, field_id=0):
    """radnet_aug_pointwise_u8 into a new image."""
    out = _empty(img.shape[0], img.shape[1])
    if out.numel():
        ctx.call("radnet_aug_pointwise_u8", img, out, img.shape[0], img.shape[1], int(mode), 1 if grey else 0, ctypes.c_double(p0), ctypes.c_double(p1),
                 ctypes.c_uint64(int(noise_seed) & (2 ** 64 - 1)), ctypes.c_uint32(int(field_id) & 0xffffffff))
    return out


def warp(ctx, img, mat, dsize):
    """radnet_warp_affine_u8 with device input and output (RADNet.warp_affine_device's arithmetic; the image does not move)."""
    import torch
    dw, dh = int(dsize[0]), int(dsize[1])
    adelta, bdelta, x0, y0 = A.warp_tables(mat, dsize)
    col = torch.from_numpy(np.concatenate([adelta, bdelta]).astype(np.int32)).cuda()
    row = torch.from_numpy(np.concatenate([x0, y0]).astype(np.int32)).cuda()
    out = _empty(dh, dw)
    ctx.call("radnet_warp_affine_u8", img, img.shape[0], img.shape[1], 3, out, dh, dw, col, row)
    return out


def resize(ctx, img, new_w, new_h):
    """radnet_resize_bicubic_u8 with device input and output."""
    if (int(new_h), int(new_w)) == tuple(img.shape[:2]):
        return img
    out = _empty(new_h, new_w)
    ctx.call("radnet_resize_bicubic_u8", img, img.shape[0], img.shape[1], out, int(new_h), int(new_w), 3)
    return out


def _boxes_only(fn, img, boxes, **kw):
    """Run a host flip / rotation for its box arithmetic alone: on an image of the same extents with zero channels (the extents
    are all that arithmetic reads; reversing or transposing zero bytes costs nothing)."""
    return fn(np.empty((int(img.shape[0]), int(img.shape[1]), 0), dtype=np.uint8), boxes, **kw)[1]


class _LastChoice:
    """Passes `rng` through and remembers what choice() returned (ninety_degree_rotation draws its angle itself)."""

    def __init__(self, rng):
        self.rng, self.last = rng, None

    def choice(self, *a, **kw):
        self.last = self.rng.choice(*a, **kw)
        return self.last


def strap(ctx, img):
    """strap_img and the callers' [row_min:row_max, col_min:col_max] slice: (the strapped image, the extent)."""
    row_min, row_max, col_min, col_max = ext = extent(ctx, img)
    return gather(ctx, img, IDENTITY, (row_min, col_min, row_max - row_min, col_max - col_min)), ext


def horizontal_flip(ctx, img, boxes):
    return gather(ctx, img, FLIP_COLS), _boxes_only(A.horizontal_flip, img, boxes)


def vertical_flip(ctx, img, boxes):
    return gather(ctx, img, FLIP_ROWS), _boxes_only(A.vertical_flip, img, boxes)


def ninety_degree_rotation(ctx, img, boxes, rng):
    tap = _LastChoice(rng)
    boxes = _boxes_only(A.ninety_degree_rotation, img, boxes, rng=tap)
    return gather(ctx, img, _ROT[int(tap.last[0])]), boxes


def any_degree_rotation(ctx, img, boxes, rng):
    arr = A._boxes_array(boxes)
    h, w = (int(v) for v in img.shape[:2])
    angle = rng.uniform(-3.0, 3.0)
    mat, dsize = A._rotation_plan(h, w, angle)
    img = warp(ctx, img, mat, dsize)
    arr = A._rotated_hulls(arr, mat)
    img, ext = strap(ctx, img)
    return img, A._strapped_rotation_boxes(boxes, arr, ext)


def shear(ctx, img, boxes, rng):
    f = rng.uniform(-0.3, 0.3)
    if f < 0.0:
        img, boxes = horizontal_flip(ctx, img, boxes)
    h, w = (int(v) for v in img.shape[:2])
    arr = A._sheared_boxes(boxes, f)
    mat, dsize = A._shear_plan(h, w, f)
    img, (row_min, _, col_min, _) = strap(ctx, warp(ctx, img, mat, dsize))
    if arr.ndim == 2:
        A._write_back(boxes, arr, col_min, row_min)
    if f < 0.0:
        img, boxes = horizontal_flip(ctx, img, boxes)
    return img, boxes


def brightness(ctx, img, boxes, rng):
    """augmentation.brightness: the mean of the non-zero elements from the histogram (exact sum and count), its draws, one launch."""
    bins = histogram(ctx, img, True)
    lo, hi = 75, 180
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.float32(int((bins * np.arange(256)).sum())) / np.float32(int(bins[1:].sum()))
    if avg <= lo or avg >= hi:
        return img, boxes
    if rng.random() < (avg - lo) / (hi - lo):
        delta, darker = rng.random() * (avg - lo), 1.0
    else:
        delta, darker = rng.random() * (hi - avg), 0.0
    return pointwise(ctx, img, AUG_BRIGHTNESS, float(np.float32(delta)), darker), boxes


def contrast(ctx, img, boxes, rng):
    lo = 75 * rng.random()
    hi = (255 - 180) * rng.random() + 180
    return pointwise(ctx, img, AUG_CONTRAST, lo, hi), boxes


def salt_and_pepper_noise(ctx, img, boxes, img_type, rng, noise_seed, field_id):
    amount = (0.3 - 0.01) * rng.random() + 0.01
    svp = A.get_truncated_normal(mean=0.5, sd=0.1, low=0, upp=1).rvs(size=1, random_state=None if rng is np.random else rng)[0]
    return pointwise(ctx, img, AUG_SALT_PEPPER, amount, svp, "grey" in img_type, noise_seed, field_id), boxes


def gaussian_noise(ctx, img, boxes, img_type, rng, noise_seed, field_id):
    mean = (0.05 + 0.05) * rng.random() - 0.05
    var = (0.01 - 0.001) * rng.random() + 0.001
    return pointwise(ctx, img, AUG_GAUSSIAN, mean, float(np.sqrt(var)), "grey" in img_type, noise_seed, field_id), boxes


def poisson_noise(ctx, img, boxes, img_type, rng, noise_seed, field_id):
    grey = "grey" in img_type
    distinct = int(np.count_nonzero(histogram(ctx, img, not grey)))           # len(np.unique(f)) of random_noise
    v = 2.0 ** np.ceil(np.log2(distinct))
    return pointwise(ctx, img, AUG_POISSON, float(v), 0.0, grey, noise_seed, field_id), boxes


def augment_device(img_data, img_dev, C, rng=np.random, noise_seed=0, field_id=0, ctx=None):
    """augmentation.augment for a uint8 HWC cuda tensor: (a deep copy of img_data with the boxes / width / height of the augmented
    image, the augmented image as a uint8 HWC cuda tensor).  See the module docstring for what equals the host path.  ctx: a
    radnet context (its stream must be torch's current one); None = the calling thread's default context, on a BackgroundFeed
    worker thread on that thread's own stream."""
    for k in ("filepath", "bboxes", "width", "height"):
        assert k in img_data
    out = copy.deepcopy(img_data)
    img, boxes = _check(img_dev), out["bboxes"]
    with feed_stream(ctx) as (ctx, side):
        if C.use_horizontal_flips and rng.random() < 0.5:
            img, boxes = horizontal_flip(ctx, img, boxes)
        if C.use_vertical_flips and rng.random() < 0.5:
            img, boxes = vertical_flip(ctx, img, boxes)
        if C.use_90_rotations and rng.random() < 0.5:
            img, boxes = ninety_degree_rotation(ctx, img, boxes, rng)
        if C.use_rotations and rng.random() < 0.5:
            img, boxes = any_degree_rotation(ctx, img, boxes, rng)
        if C.use_shear and rng.random() < 0.25:
            img, boxes = shear(ctx, img, boxes, rng)
        if C.use_brightness and rng.random() < 0.5:
            img, boxes = brightness(ctx, img, boxes, rng)
        if C.use_noise and rng.random() < 0.5:
            which = rng.randint(0, 4)
            kind = C.img_types[0]
            if which == 0:
                img, boxes = salt_and_pepper_noise(ctx, img, boxes, kind, rng, noise_seed, field_id)
            elif which == 1:
                img, boxes = gaussian_noise(ctx, img, boxes, kind, rng, noise_seed, field_id)
            elif which == 2:
                img, boxes = poisson_noise(ctx, img, boxes, kind, rng, noise_seed, field_id)
            else:
                img, boxes = contrast(ctx, img, boxes, rng)
    out["bboxes"] = boxes
    out["width"], out["height"] = int(img.shape[1]), int(img.shape[0])
    return out, hand_over(img, side)
