"""Cases and reference arithmetic of the device-resident augmentation tests (test_augment_device_host.py on the CPU,
test_gpu_augment_device.py on the device).  Not a test.  The noise part is a NumPy restatement of the field definition in
include/radnet_hip.h -- Philox4x32-10, the two uniforms, the three modes, img_as_ubyte, background / grey handling -- written
from that definition and the published Philox one; it imports nothing of the product."""
import numpy as np

SIZES = [(1, 1), (2, 3), (37, 53), (64, 61), (61, 64)]            # H x W
CHAIN_SIZES = [(37, 53), (64, 61), (61, 64)]                      # sizes at which every step of the chain has an image left to work on
LARGE = (1500, 1500)                                              # more pixels than the capped grids of the two reductions have threads

# Philox4x32-10 known answers: (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

_M0, _M1, _W0, _W1, _MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xffffffff)
_S32 = np.uint64(32)


def image(h, w, seed, kind="border"):
    """Random uint8 HWC content.  'border': a zero border (several pixels wide where the image has room, one pixel on the smaller
    ones) plus zeros planted at random elements and whole zero pixels -- the strap and the background restore have work to do;
    'full': no zero anywhere."""
    rs = np.random.RandomState(seed)
    if kind == "full":
        return rs.randint(1, 256, (h, w, 3)).astype(np.uint8)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    img[rs.random_sample((h, w, 3)) < 0.05] = 0
    img[rs.random_sample((h, w)) < 0.05] = 0
    b = 5 if min(h, w) >= 30 else (1 if min(h, w) >= 3 else 0)
    if b:
        img[:b] = 0
        img[-b:] = 0
        img[:, :b - 1 if b > 1 else 1] = 0            # unequal margins: a transposed or mirrored strap would show
        img[:, -b:] = 0
        img[b, b if b > 1 else 1, 1] = 255            # the strap's corners are real pixels
        img[h - b - 1, w - b - 1, 1] = 255
    return img


def philox4x32(counter, key, rounds=10):
    """counter: four uint64 arrays (values below 2^32) of one shape, key: two ints.  Returns the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2                                  # 32 x 32 -> 64 bit products
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniforms(n, noise_seed, field_id):
    """u_a, u_b of the elements 0 .. n-1 of field `field_id` under the 64-bit `noise_seed`."""
    idx = np.arange(n, dtype=np.uint64)
    zero = np.zeros(n, dtype=np.uint64)
    seed = int(noise_seed) & (2 ** 64 - 1)
    x0, x1, x2, x3 = philox4x32((idx & _MASK, idx >> _S32, zero + np.uint64(field_id), zero), (seed & 0xffffffff, seed >> 32))
    eleven = np.uint64(11)
    ua = ((((x0 << _S32) | x1) >> eleven).astype(np.float64) + 0.5) * 2.0 ** -53
    ub = ((((x2 << _S32) | x3) >> eleven).astype(np.float64) + 0.5) * 2.0 ** -53
    return ua, ub


def normal(ua, ub):
    return np.sqrt(-2.0 * np.log(ua)) * np.cos(6.283185307179586 * ub)


def poisson_counts(lam, ua):
    """Inversion by walking the CDF in float64: p = s = exp(-lam), k = 0; while u > s: k += 1, p *= lam / k, s += p; capped at 1023."""
    lam = np.asarray(lam, dtype=np.float64)
    p = np.exp(-lam)
    s = p.copy()
    k = np.zeros(lam.shape, dtype=np.int64)
    for step in range(1, 1024):
        live = ua > s
        if not live.any():
            break
        k[live] = step
        p[live] = p[live] * (lam[live] / float(step))
        s[live] = s[live] + p[live]
    return k


def noise(img, mode, grey, p0, p1, noise_seed, field_id):
    """The device's noise modes on a uint8 HWC image.  mode 's&p' (p0 = amount, p1 = salt_vs_pepper), 'gaussian' (p0 = mean,
    p1 = sigma) or 'poisson' (p0 = v).  grey: one plane from channel 0 to all three channels.  Zeros of the input stay zero."""
    plane = img[:, :, 0] if grey else img
    ua, ub = (u.reshape(plane.shape) for u in uniforms(plane.size, noise_seed, field_id))
    f = plane.astype(np.float64) / 255.0
    if mode == "s&p":
        x = f.copy()
        hit, salt = ua <= p0, ub <= p1
        x[hit & salt] = 1.0
        x[hit & ~salt] = 0.0
    elif mode == "gaussian":
        x = f + (p0 + p1 * normal(ua, ub))
    else:
        x = poisson_counts(f * p0, ua) / float(p0)
    x = np.clip(x, 0.0, 1.0)
    out = np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8)              # img_as_ubyte
    out[plane == 0] = 0
    return np.repeat(out[:, :, None], 3, axis=2) if grey else out


def poisson_v(img, grey):
    """random_noise's v: the number of distinct values rounded up to a power of two."""
    return float(2.0 ** np.ceil(np.log2(len(np.unique(img[:, :, 0] if grey else img)))))


def dihedral(img, window, transform):
    """NumPy indexing form of the gather: window (y0, x0, h, w), then bit 2 transposes, bit 0 reverses rows, bit 1 columns."""
    y0, x0, h, w = window
    out = img[y0:y0 + h, x0:x0 + w]
    if transform & 4:
        out = out.transpose(1, 0, 2)
    if transform & 1:
        out = out[::-1]
    if transform & 2:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def windows(h, w):
    """Full image, an interior window, a 1-pixel window."""
    out = [(0, 0, h, w), (h - 1, w - 1, 1, 1)]
    if h >= 3 and w >= 3:
        out.append((1, 2 if w > 3 else 1, h - 2, w - (3 if w > 3 else 2)))
    return out


def boxes(h, w, seed):
    rs = np.random.RandomState(1000 + seed)
    out = []
    for _ in range(4):
        x1, y1 = int(rs.randint(0, w - 8)), int(rs.randint(0, h - 8))
        out.append({"class": "boat", "x1": x1, "y1": y1, "x2": int(rs.randint(x1 + 4, w)), "y2": int(rs.randint(y1 + 4, h))})
    return out
