"""Case tables for radnet_score_levels_u8 and radnet_heat_paint_u8, and a NumPy model of both written from the contracts in
include/radnet_hip.h, not from the kernels.  Shared by tests/test_heat_host.py (CPU) and tests/test_gpu_heat.py.

levels(pred, ld, M, first, count): per row the maximum of the columns [first, first + count), NaNs skipped; the level is
clamp(floor(s * 255 + 0.5), 0, 255) with the product and the sum each rounded to float32; a row of NaNs gives 0.

paint(img, pool, places, lut, tau, min_level): a placement (x0, y0, w, h, mw, mh, offset) covers [x0, x0 + w) x [y0, y0 + h); pixel
(X, Y) reads its map at row ((Y - y0) * mh) // h, column ((X - x0) * mw) // w; the pixel's level is the maximum over the placements
that hold it; not held or below min_level: untouched; else every channel is (c * (255 - tau) + d * tau + 127) // 255."""
import numpy as np

PITCH = 128
SENTINEL = 0xA5
SIZES = [(21, 37), (8, 32), (9, 33)]                     # (h, w): several tiles with ragged edges, exactly one tile, one pixel more
TAUS = (0, 102, 255)
MIN_LEVELS = (0, 1, 128, 255)
MUTANTS = ("round", "min", "last", "inclusive", "le")


# ---- the level rule -----------------------------------------------------------------------------------------------------------------
def levels(pred, ld, M, first, count):
    rows = np.asarray(pred, np.float32).reshape(-1)[:M * ld].reshape(M, ld)[:, first:first + count]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.fmax.reduce(rows, axis=1)                 # fmax skips NaNs; NaN only when the whole row is
        t = (s * np.float32(255.0)).astype(np.float32)
        t = np.floor((t + np.float32(0.5)).astype(np.float32))
    out = np.zeros(M, np.uint8)
    ok = ~np.isnan(t)
    out[ok] = np.clip(t[ok], 0, 255).astype(np.uint8)
    return out


LEVEL_MS = (1, 63, 64, 65, 1000)
LEVEL_RANGES = ((0, 9), (3, 1), (6, 3), (0, 12))
LEVEL_LD = 64


def level_case(M, first, count, outside):
    """[M][64] float32 scores: the columns [first, first + count) hold values around and exactly at the level boundaries, some
    infinities and NaNs, and (M > 1) one row of NaNs only; every other column holds `outside` (+inf or NaN), so reading it shows."""
    rs = np.random.RandomState(1000 * M + 10 * first + count)
    pred = np.full((M, LEVEL_LD), outside, np.float32)
    win = rs.uniform(-0.05, 1.05, (M, count)).astype(np.float32)
    k = rs.randint(0, 256, M)
    special = [np.float32(k / 255.0), (np.float32(k) / np.float32(255.0)), np.float32((k + 0.5) / 255.0), np.float32((k - 0.5) / 255.0),
               np.zeros(M, np.float32), np.ones(M, np.float32), np.full(M, -1e-3, np.float32), np.full(M, 1.0 + 1e-3, np.float32),
               np.full(M, np.inf, np.float32), np.full(M, -np.inf, np.float32)]
    kind = rs.randint(0, len(special) + 2, M)            # the last two: the row stays random
    for m in range(M):
        if kind[m] < len(special):
            v = special[kind[m]][m]
            if kind[m] < 8:                              # the special value is the row's maximum: the others lie below it or are NaN
                win[m] = np.minimum(win[m], v) - np.float32(0.25) * (rs.random_sample(count) < 0.5)
            win[m, rs.randint(count)] = v
        if count > 1 and rs.random_sample() < 0.4:
            win[m, rs.randint(count)] = np.nan           # skipped; may hit the special value, then the rest decides
    if M > 1:
        win[M // 2] = np.nan
        win[M - 1] = -np.inf
    pred[:, first:first + count] = win
    return pred


def level_cases():
    return [(M, first, count, name) for M in LEVEL_MS for (first, count) in LEVEL_RANGES for name in ("inf", "nan")]


# ---- the painter ----------------------------------------------------------------------------------------------------------------------
def paint(img, pool, places, lut, tau, min_level, mutant=None):
    """Paints into img ([h][w][3] uint8) in place and returns it.  `mutant` breaks one rule (MUTANTS), for the tests of the cases."""
    h, w = img.shape[:2]
    pool = np.asarray(pool, np.uint8).reshape(-1)
    lut = np.asarray(lut, np.uint8).reshape(256, 3)
    level = np.full((h, w), -1, np.int64)
    edge = 1 if mutant == "inclusive" else 0
    for (x0, y0, pw, ph, mw, mh, off) in places:
        xa, xb, ya, yb = max(x0, 0), min(x0 + pw + edge, w), max(y0, 0), min(y0 + ph + edge, h)
        if xa >= xb or ya >= yb:
            continue
        X, Y = np.arange(xa, xb, dtype=np.int64), np.arange(ya, yb, dtype=np.int64)
        if mutant == "round":
            cols, rows = (2 * (X - x0) * mw + pw) // (2 * pw), (2 * (Y - y0) * mh + ph) // (2 * ph)
        else:
            cols, rows = ((X - x0) * mw) // pw, ((Y - y0) * mh) // ph
        cols, rows = np.minimum(cols, mw - 1), np.minimum(rows, mh - 1)          # only the mutants ever reach past the map
        cells = pool[off:off + mw * mh].reshape(mh, mw).astype(np.int64)[rows][:, cols]
        old = level[ya:yb, xa:xb]
        if mutant == "last":
            new = cells
        elif mutant == "min":
            new = np.where(old < 0, cells, np.minimum(old, cells))
        else:
            new = np.maximum(old, cells)
        level[ya:yb, xa:xb] = new
    on = (level >= 0) & ((level > min_level) if mutant == "le" else (level >= min_level))
    c = lut[level[on]].astype(np.int64)
    d = img[on].astype(np.int64)
    img[on] = (c if tau == 0 else (c * (255 - tau) + d * tau + 127) // 255).astype(np.uint8)
    return img


def canvas(h, w, seed=0):
    """A noise image in a buffer of h rows of PITCH bytes, sentinels in the padding."""
    buf = np.full((h, PITCH), SENTINEL, np.uint8)
    buf[:, :3 * w] = np.random.RandomState(seed).randint(0, 256, (h, 3 * w))
    return buf


def expected(buf, h, w, pool, places, lut, tau, min_level, mutant=None):
    want = buf.copy()
    img = want[:, :3 * w].reshape(h, w, 3).copy()
    paint(img, pool, places, lut, tau, min_level, mutant)
    want[:, :3 * w] = img.reshape(h, 3 * w)
    return want


def luts():
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    return {"grey": grey, "random": np.random.RandomState(77).randint(0, 256, (256, 3)).astype(np.uint8)}


class _Pool:
    """Maps appended to one byte pool; levels at and around the thresholds of MIN_LEVELS are frequent."""

    def __init__(self, seed):
        self.rs, self.parts, self.n = np.random.RandomState(seed), [np.full(5, 0xEE, np.uint8)], 5      # five bytes no map refers to

    def add(self, mh, mw, values=None):
        if values is None:
            values = np.where(self.rs.random_sample((mh, mw)) < 0.5, self.rs.choice([0, 1, 2, 127, 128, 129, 254, 255], (mh, mw)),
                              self.rs.randint(0, 256, (mh, mw)))
        values = np.asarray(values, np.uint8).reshape(mh, mw)
        off = self.n
        self.parts.append(values.reshape(-1))
        self.n += mh * mw
        return (mw, mh, off)

    def bytes(self):
        return np.concatenate(self.parts)


def paint_tables():
    """{name: places} and the pool they share.  The coordinates are laid out for the 37 x 21 image; on the two small images the
    same tables overhang more."""
    p = _Pool(5)
    one, m32, m54, wide = p.add(1, 1, [[200]]), p.add(2, 3), p.add(4, 5), p.add(1, 2047)
    a = np.where((np.add.outer(np.arange(4), np.arange(4)) % 2) == 0, 210, 20)
    b = np.where((np.add.outer(np.arange(4), np.arange(4)) % 2) == 0, 30, 190)
    ma, mb = p.add(4, 4, a), p.add(4, 4, b)
    t = {}
    t["none"] = []
    t["one 1x1"] = [(3, 2, 9, 5) + one]
    t["one 3x2 much larger than its map"] = [(2, 3, 30, 15) + m32]
    t["two: 5x4 and 1x1"] = [(1, 1, 20, 10) + m54, (25, 12, 8, 6) + one]
    extras = [(i % 37, (i * 7) % 21, 1 + i % 3, 1 + i % 2) + p.add(1, 1) for i in range(255)]
    t["257: two batches"] = [(2, 3, 30, 15) + m32, (1, 1, 20, 10) + m54] + extras
    t["2047x1 into 37 columns"] = [(0, 5, 37, 3) + wide]
    t["2047x1 overhanging both sides"] = [(-900, 1, 2047, 4) + wide]
    t["destination smaller than its map"] = [(10, 4, 2, 3) + m54]
    t["overhang left"] = [(-7, 4, 15, 9) + m54]
    t["overhang top"] = [(5, -3, 12, 9) + m54]
    t["overhang right"] = [(30, 2, 20, 9) + m54]
    t["overhang bottom"] = [(6, 15, 14, 20) + m32]
    t["overhang on all four sides"] = [(-5, -4, 60, 40) + m54]
    t["wholly outside"] = [(40, 3, 5, 5) + m54, (-10, -10, 5, 5) + m32, (3, 21, 5, 5) + m32, (3, -5, 5, 5) + one]
    t["two overlapping, the maximum alternates"] = [(5, 3, 16, 8) + ma, (5, 3, 16, 8) + mb]
    t["two overlapping, shifted"] = [(3, 2, 20, 12) + mb, (9, 5, 20, 12) + ma, (0, 0, 6, 6) + m32]
    return t, p.bytes()


def paint_cases():
    """[(size, table name, tau, min_level, lut name)]: every table under every tau, min_level and colour table on the 37 x 21 image,
    and under two of those combinations on the image of exactly one tile and the one a pixel larger."""
    tables, _ = paint_tables()
    out = []
    for size in SIZES:
        combos = [(tau, ml, lut) for tau in TAUS for ml in MIN_LEVELS for lut in ("grey", "random")]
        if size != SIZES[0]:
            combos = [(0, 0, "grey"), (102, 1, "random"), (255, 128, "random")]
        out += [(size, name, tau, ml, lut) for name in tables for (tau, ml, lut) in combos]
    return out


# ---- tables radnet_heat_check refuses: (what, places, pool_len, h, w, the bad entry, the field its message names) ---------------------------
def refused_tables():
    good = [(1, 1, 20, 10, 5, 4, 0), (25, 12, 8, 6, 1, 1, 20), (0, 0, 1048576, 1048576, 2047, 2047, 21)]
    pool_len = 21 + 2047 * 2047
    M = 16777216

    def with_(entry, field, value):
        t = [list(r) for r in good]
        t[entry][field] = value
        return [tuple(r) for r in t]

    cases = [("w = 0", with_(0, 2, 0), "w"), ("w too large", with_(2, 2, 1048577), "w"), ("w negative", with_(1, 2, -3), "w"),
             ("h = 0", with_(1, 3, 0), "h"), ("h too large", with_(0, 3, 1048577), "h"),
             ("mw = 0", with_(0, 4, 0), "mw"), ("mw = 2048", with_(1, 4, 2048), "mw"),
             ("mh = 0", with_(2, 5, 0), "mh"), ("mh = 2048", with_(0, 5, 2048), "mh"),
             ("x0 beyond", with_(1, 0, M + 1), "x0"), ("x0 beyond, negative", with_(0, 0, -M - 1), "x0"),
             ("y0 beyond", with_(2, 1, M + 1), "y0"), ("y0 at the end of int32", with_(0, 1, -2 ** 31), "y0"),
             ("offset negative", with_(1, 6, -1), "offset"), ("offset past the pool", with_(1, 6, pool_len), "offset"),
             ("the last map one byte too long", with_(2, 6, 22), "offset"), ("offset at the end of int64", with_(0, 6, 2 ** 63 - 1), "offset")]
    out = [(what, places, pool_len, 21, 37, [i for i, (a, b) in enumerate(zip(places, good)) if a != b][0], field) for what, places, field in cases]
    return good, pool_len, out
