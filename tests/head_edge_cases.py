"""Shared case tables, float64 references, per-element bounds and input builders of the edge tests of the pooling, RoI crop, classifier
head and loss kernels: csrc/elementwise.hip (maxpool, roi_resize fwd / bwd, avgpool fwd / bwd_relu, dense_heads fwd / bwd, rpn_loss,
det_loss) and csrc/head_tail.hip (head_tail_fwd).  Device-free check of the tables, the references and their teeth:
tests/test_head_edge_cases_reference.py; the kernels: tests/test_gpu_head_edges.py.  NumPy only: no torch, no library.

The operations, every reference written out below in float64 on the fp32 input values:

  maxpool          y[b][oy][ox][c] = max over i, j < k of x[b][oy*s + i][ox*s + j][c], oh = (h - k) / s + 1 ('valid') ........... bit-exact
  roi_resize fwd   per RoI (x, y, w, h): truncate to int, clamp the slice to the map, crop; TF1 legacy bilinear resize to ps x ps:
                   s = fl32(oy * fl32(ch / ps)), lo = floor(s), hi = min(lo + 1, ch - 1), l = fl32(s - lo) -- the kernel's own fp32
                   coordinate arithmetic, repeated here in np.float32 --, out = top + (bot - top) * ly, top = a + (b - a) * lx.
                   An empty crop gives a row of +0.0.
  roi_resize bwd   dfmap[y0 + yy][x0 + xx] += dy[r][oy][ox] * wy * wx for the four taps of every output pixel, wy in (1 - ly, ly).
  avgpool fwd      feat[r][c] = (sum_p x[r][p][c]) / hw
  avgpool bwd_relu dx[r][p][c] = act[r][p][c] > 0 ? fl32(g[r][c] / hw) : +0.0 ...................................................... bit-exact
  dense_heads fwd  z = feat @ w[:, :nout] + b[:nout];  out_cls = softmax(z[:nc]) with max-subtraction, out_regr = z[nc:nout]
  dense_heads bwd  dw[k][n] (+)= sum_r feat[r][k] dz[r][n], db[n] (+)= sum_r dz[r][n], dfeat[r][k] = sum_{n < nout} dz[r][n] w[k][n];
                   columns nout .. ldw-1 of dw / db receive (+)= 0
  rpn_loss         losses.py:16-66: [cls, regr] and dz [m][ld_dz]: columns [0, a) the class term through the sigmoid, [a, 5a) smooth-L1,
                   [5a, ld_dz) +0.0; normalisers 1e-4 * m * a + sum valid and 1e-4 * m * 4a + sum mask
  det_loss         losses.py:69-95: [cls, regr, accuracy] and dz [r][nc + nreg]: categorical cross-entropy on the re-normalised, clipped
                   q through the softmax, smooth-L1 over 1e-4 * r * nreg + sum mask; argmax takes the FIRST maximum
  head_tail fwd    avgpool -> dense heads -> softmax -> per GROUP of r / groups rows the detector losses with the group's own
                   normalisers, all in float64 from y5; an idle group has +0.0 gradient rows and untouched loss slots

The clip bounds are the kernels' fp32 constants (1e-7f and 1.0f - 1e-7f) as float64.

Bounds, U = 2^-24.  Where a kernel uses + - * / only, per element
  tol = (terms + roundings of the epilogue) * U * sum|terms| + 2 U |old|
counted from the association the kernel writes, every operation as one rounding:
  roi_resize fwd   a tap passes b - a, * lx, + a, bot - top, * ly, + top: 6.  sum|terms| is the same expression with every tap replaced
                   by its magnitude and every difference by a sum: T = |a| + (|a| + |b|) lx, mag = T + (T + B) ly.
                   The weights carry one rounding more than the first count had: the kernel writes sy = oy * hs; ly = sy - ylo, and
                   the compiler contracts the two into one FMA, which does NOT round the product, while the reference (and
                   TensorFlow) round it; the two weights differ by up to U sy, a rounding at the magnitude of the source
                   coordinate, not of the weight.  The first run on the device measured 1.65 of 6 U mag at ps = 14 on the (5, 7, 4)
                   map where ly = 0.07 and lx = 0; the count was corrected, not scaled:
                   tol = 6 U mag + U sx |d out / d lx| + U sy |d out / d ly|, the derivatives with magnitudes for taps:
                   (|a| + |b|)(1 - ly) + (|d| + |e|) ly and T + B
  roi_resize bwd   n taps land on a pixel.  A product is 1 - ly, 1 - lx, v * wy, * wx: 4 roundings; n - 1 additions; the addition to the
                   old value: (n + 4) U sum|v wy wx| + 2 U |old| in the ordered form, plus the weights' U sy, U sx of the forward:
                   U sum|v| (sy wx + sx wy).  The atomic form adds every tap to the running value, which holds the old one: the old
                   value passes n additions, n U |old| there (2 U |old| for n < 2).  A pixel no tap lands on keeps its old bits.
  avgpool fwd      hw terms, one division: (hw + 1) U sum|x| / hw -- in any order of the additions (elementwise sums the positions in
                   order, head_tail in four groups of positions)
  dense logits     k products, k - 1 additions in any tree, the bias: (k + 1) U (sum|f w| + |b|)
  dw, db, dfeat    r (dw, db) or nout (dfeat) terms: terms U sum|terms|, with accumulate one addition more and 2 U |old|
  head_tail feat   as avgpool fwd; its regression outputs read the device's own feat, so their bound is the dense one at k = c plus
                   the feat bound carried through |w|: tol_feat @ |w|
Where a kernel calls expf / logf a rounding count bounds nothing; the tolerances are the ones tests/test_gpu_kernels.py states for these
kernels, each applied to its own block (class / regression columns of dz, columns [0, a) / [a, 5a) of the RPN's dz, each group's rows
in the head tail): RPN losses 2e-5 |ref| + 1e-7, detector losses 1e-5 |ref| + 1e-7, accuracy 1e-6, RPN dz 2e-5 of the block's max,
detector class dz 1e-4 and regression dz 1e-5 of the block's max, softmax 1e-5 of the block's max.  None of them had to be replaced
by the fp32-emulation procedure.

Inputs.  Nothing but RoI coordinates is restricted to integers.  RoI coordinates and sizes are non-negative.  Pad columns of w, b
(>= nout) and of pred ([5a, ld_pred)) hold 1e30: by the kernels' indexing they reach no output.  No decision that the device takes in
fp32 and the reference in float64 is borderline: smooth-L1 differences are exactly 0 or at least 1e-3 away from |x| = 1, activations
are 0.0, -0.0 or of magnitude >= 1e-3, clipped probabilities are exactly 0, exactly 1 or inside [1e-4, 1 - 1e-4], the two largest
entries of an argmax row are equal (both sides take the first) or 1e-4 apart.  `borderline_*` count the violations; the CPU test
asserts zero for every case, so a GPU test skips no element.

Every function that describes an output returns the FULL buffer: dict(buf, inside, tol, zero, shape[, old]) -- the float64 reference of
every element of the tensor the kernel writes into followed by TAIL floats, NaN where nothing may be written (the element keeps the
SENTINEL bits it was prefilled with), `inside` the elements that must be written, `tol` their bound, `zero` the elements that must be
exactly +0.0, `old` the fp32 values the buffer holds before an accumulating launch."""
import collections
import functools

import numpy as np

U = 2.0 ** -24
SENTINEL = np.uint32(0x7FC5A5A5)          # the project's quiet NaN no kernel produces (winograd_edge_cases.py): prefill of every output element
TAIL = 64                                 # floats behind every output that must keep the sentinel
PAD = np.float32(1e30)                    # what pad columns of w, b and pred hold
F = np.float32
LO, HI = float(F(1e-7)), float(F(1.0) - F(1e-7))          # the kernels' clip bounds
LOSS_EPS = 1e-4
MARGIN = 1e-3                             # smooth-L1 and ReLU decisions
PMARGIN = 1e-4                            # clip and argmax decisions
L1_GAP = 0.05                             # how far the builders keep a non-zero smooth-L1 difference from |x| = 1

MUTANTS = ("pool_init_zero", "pool_drop_last", "roi_round", "roi_no_clamp", "roi_hi_unclamped", "roi_dedup", "avg_div49", "tail_drop_64",
           "no_bias", "softmax_no_max", "acc_ignored", "pad_read", "rpn_no_eps", "l1_threshold", "det_batch_norm", "idle_live", "acc_last_max")


def _out(ref, tol=None, zero=None, old=None):
    """The full buffer of one output: ref float64 (NaN: must keep the sentinel), TAIL floats behind it."""
    ref = np.asarray(ref, np.float64)
    inside = ~np.isnan(ref)
    tol = np.zeros(ref.shape) if tol is None else np.where(inside, np.broadcast_to(tol, ref.shape), 0.0)
    zero = np.zeros(ref.shape, bool) if zero is None else np.broadcast_to(zero, ref.shape)
    cat = lambda a, fill, ty: np.concatenate([np.asarray(a, ty).ravel(), np.full(TAIL, fill, ty)])
    res = dict(buf=cat(ref, np.nan, np.float64), inside=cat(inside, False, bool), tol=cat(tol, 0.0, np.float64), zero=cat(zero, False, bool),
               shape=ref.shape)
    if old is not None:
        res["old"] = np.ascontiguousarray(old, F)
        assert res["old"].shape == ref.shape
    return res


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _frozen(v)
    return d


def _normal(rs, *shape):
    return rs.standard_normal(shape).astype(F)


def activations(rs, shape, relu=False):
    """fp32 values that are 0.0, -0.0 or of magnitude >= MARGIN (the ReLU decision `> 0` is the same in every precision)."""
    x = _normal(rs, *shape)
    if relu:
        x = np.maximum(x, F(0))
    x[np.abs(x) < MARGIN] = F(0)
    flat = x.reshape(-1)
    flat[rs.randint(0, flat.size, max(1, flat.size // 16))] = F(-0.0)
    flat[rs.randint(0, flat.size, max(1, flat.size // 16))] = F(0.0)
    return x


def l1_offsets(rs, shape):
    """Differences on both smooth-L1 branches, at least L1_GAP away from |x| = 1, and exact zeros."""
    d = rs.choice([-1.0, 1.0], shape) * np.where(rs.uniform(size=shape) < 0.5, rs.uniform(L1_GAP, 1 - L1_GAP, shape), rs.uniform(1 + L1_GAP, 3.0, shape))
    d[rs.uniform(size=shape) < 0.1] = 0.0
    return d.astype(F)


def targets_for(pred, d):
    """fp32 targets with fl32(tgt - pred) == 0 where d == 0 and within 2^-21 of d elsewhere (|pred| < 8)."""
    return np.where(d == 0, pred, (pred.astype(F) + d.astype(F)).astype(F)).astype(F)


def borderline_l1(tgt, pred, mask=None):
    """Elements whose smooth-L1 branch could differ between fp32 and float64: |x| within MARGIN of 1 (x == 0 is the exact zero)."""
    x32 = np.abs((tgt.astype(F) - pred.astype(F)).astype(np.float64))
    x64 = np.abs(tgt.astype(np.float64) - pred.astype(np.float64))
    bad = (np.abs(x32 - 1.0) < MARGIN) | (np.abs(x64 - 1.0) < MARGIN) | ((x32 == 0) != (x64 == 0))
    return int((bad if mask is None else bad & (mask != 0)).sum())


def borderline_act(x):
    return int(((x != 0) & (np.abs(x) < MARGIN)).sum())


def borderline_prob(p):
    """Clip decisions against [1e-7, 1 - 1e-7]: exactly 0, exactly 1 or inside [PMARGIN, 1 - PMARGIN]."""
    p = np.asarray(p, np.float64)
    return int((~((p == 0) | (p == 1) | ((p >= PMARGIN) & (p <= 1 - PMARGIN)))).sum())


def borderline_argmax(q):
    """Rows whose two largest entries are neither equal nor PMARGIN apart."""
    q = np.asarray(q, np.float64)
    if q.shape[-1] < 2:
        return 0
    top = np.sort(q, -1)[..., -2:]
    gap = top[..., 1] - top[..., 0]
    return int(((gap != 0) & (gap < PMARGIN)).sum())


def first_argmax(a):
    """The kernels' loop `if (a[i] > a[am]) am = i`: the first maximum (np.argmax's rule as well)."""
    return np.argmax(a, -1)


# ================================================================================================================ maxpool
# radnet_maxpool_fwd(x, y, nb, h, w, c, k, s).  Contract (entry checks + maxpool_kernel's indexing): c % 4 == 0, nb, k, s >= 1,
# h, w >= k (a non-empty 'valid' output), fewer than 2^31 float4 work items.  The window starts from src[0], its own first element.
MAXPOOL = [(1, 3, 3, 4, 3, 2),            # one output
           (1, 2, 3, 4, 1, 1),            # identity
           (2, 7, 9, 4, 3, 2),
           (1, 8, 10, 8, 3, 2),           # last row and column unused
           (3, 5, 6, 12, 2, 2),           # odd h
           (1, 21, 30, 68, 3, 2)]         # 17 float4 columns
MAXPOOL_NEGATIVE = (0, 2)                 # cases whose inputs are all negative: a window that starts from 0 fails


def maxpool_contract(nb, h, w, c, k, s):
    return min(nb, k, s) >= 1 and c >= 4 and c % 4 == 0 and h >= k and w >= k and nb * ((h - k) // s + 1) * ((w - k) // s + 1) * (c // 4) < 2 ** 31


@functools.lru_cache(maxsize=None)
def maxpool_inputs(i):
    nb, h, w, c, k, s = MAXPOOL[i]
    x = _normal(np.random.RandomState(100 + i), nb, h, w, c)
    if i in MAXPOOL_NEGATIVE:
        x = -np.abs(x) - F(0.5)
    return _frozen(dict(x=x))


def ref_maxpool(x, k, s, mut=None):
    nb, h, w, c = x.shape
    oh, ow = (h - k) // s + 1, (w - k) // s + 1
    out = np.full((nb, oh, ow, c), 0.0 if mut == "pool_init_zero" else -np.inf)
    kj = k - 1 if (mut == "pool_drop_last" and k > 1) else k
    for i in range(k):
        for j in range(kj):
            out = np.maximum(out, x[:, i:i + s * (oh - 1) + 1:s, j:j + s * (ow - 1) + 1:s, :].astype(np.float64))
    return dict(y=_out(out))


# ================================================================================================================ roi_resize
# radnet_roi_resize_fwd(fmap, h, w, c, rois, r, ps, y) / radnet_roi_resize_bwd(dy, h, w, c, rois, r, ps, dfmap).  Contract: c % 4 == 0,
# r, ps, h, w >= 1; RoI (x, y, w, h) non-negative floats (the proposals are clipped at 0).  roi_geom truncates and clamps to the map, so
# every tap lies inside it; the ordered backward keeps one bit per output column (ps <= 32), the entry takes the atomics kernel above.
ROI_MAPS = [(5, 7, 4), (6, 5, 12),
            (9, 11, 260),                 # 65 float4 columns: 128 threads, half of the last wave idle
            (4, 4, 1028)]                 # 257 columns: second pass of the stride loop
ROI_FWD_PS = (1, 2, 7, 14)


def roi_bwd_ps(mi):
    return (1, 2, 7) + ((32, 33) if ROI_MAPS[mi] == (5, 7, 4) else ())          # mask width, then the fallback to the atomics kernel


def roi_contract(H, W, C, rois, ps):
    return C % 4 == 0 and C >= 4 and min(H, W, ps, len(rois)) >= 1 and bool((rois >= 0).all()) and rois.dtype == F


def roi_list(H, W):
    """The RoIs (x, y, w, h) fitted to an H x W map."""
    return np.array([[0, 0, W, H],                                              # the whole map (larger than ps = 1, 2; than 7 on 9x11)
                     [0, 0, 1, 1], [W - 1, 0, 1, 1], [0, H - 1, 1, 1], [W - 1, H - 1, 1, 1],          # one pixel at each corner (smaller than ps)
                     [1, 1, 0, 2], [1, 1, 2, 0],                                # w = 0, h = 0: empty
                     [W - 2, H - 2, 5, 5],                                      # past the right and bottom edge: clamped to 2 x 2
                     [W, 0, 3, 3],                                              # starts at x = W: empty after clamping
                     [1.9, 0.7, 2.6, 3.9],                                      # truncation (1, 0, 2, 3), not rounding (2, 1, 3, 4)
                     [1, 1, 3, 3], [1, 1, 3, 3], [2, 2, 3, 2]], F)              # the same RoI twice and one overlapping it


@functools.lru_cache(maxsize=None)
def roi_inputs(mi, ps):
    H, W, C = ROI_MAPS[mi]
    rs = np.random.RandomState(200 + 10 * mi + ps)
    rois = roi_list(H, W)
    return _frozen(dict(fmap=_normal(rs, H, W, C), rois=rois, dy=_normal(rs, len(rois), ps, ps, C), old=_normal(rs, H, W, C)))


def _geom(roi, H, W, mut=None):
    conv = np.rint if mut == "roi_round" else np.trunc
    x, y, w, h = (int(conv(v)) for v in roi)
    if mut == "roi_no_clamp":
        return x, y, w, h
    y0, y1 = min(max(y, 0), H), min(max(y + h, 0), H)
    x0, x1 = min(max(x, 0), W), min(max(x + w, 0), W)
    return x0, y0, x1 - x0, y1 - y0


def _taps(n, ps, o, mut=None):
    """(lo, hi, l, s) of output index o along an axis of crop length n: the kernel's fp32 arithmetic."""
    s = F(o) * (F(n) / F(ps))
    lo = int(np.floor(s))
    return lo, (lo + 1 if mut == "roi_hi_unclamped" else min(lo + 1, n - 1)), float(F(s - F(lo))), float(s)


def _flat_map(fmap, dt):
    """[pixel][c] with NaN rows behind the map: what a tap index past the map reads (mutants only)."""
    H, W, C = fmap.shape
    return np.concatenate([fmap.reshape(H * W, C).astype(dt), np.full((64 * W + 64, C), np.nan, dt)])


def ref_roi_fwd(fmap, rois, ps, mut=None, dt=np.float64):
    H, W, C = fmap.shape
    flat = _flat_map(fmap, dt)
    R = len(rois)
    out, mag, empty = np.zeros((R, ps, ps, C), dt), np.zeros((R, ps, ps, C)), np.zeros(R, bool)
    for r in range(R):
        x0, y0, cw, ch = _geom(rois[r], H, W, mut)
        if cw <= 0 or ch <= 0:
            empty[r] = True
            continue
        for oy in range(ps):
            ylo, yhi, ly, sy = _taps(ch, ps, oy, mut)
            for ox in range(ps):
                xlo, xhi, lx, sx = _taps(cw, ps, ox, mut)
                a, b = flat[(y0 + ylo) * W + x0 + xlo], flat[(y0 + ylo) * W + x0 + xhi]
                d, e = flat[(y0 + yhi) * W + x0 + xlo], flat[(y0 + yhi) * W + x0 + xhi]
                top, bot = a + (b - a) * dt(lx), d + (e - d) * dt(lx)
                out[r, oy, ox] = top + (bot - top) * dt(ly)
                aa, ab, ad, ae = (np.abs(v.astype(np.float64)) for v in (a, b, d, e))
                T, B = aa + (aa + ab) * lx, ad + (ad + ae) * lx
                mag[r, oy, ox] = 6 * (T + (T + B) * ly) + sx * ((aa + ab) * (1 - ly) + (ad + ae) * ly) + sy * (T + B)
    zero = np.broadcast_to(empty[:, None, None, None], out.shape)
    return dict(y=_out(out, U * mag, zero))


def ref_roi_bwd(dy, H, W, rois, ps, old, ordered, mut=None, dt=np.float64):
    C = dy.shape[-1]
    n_pix = H * W + 64 * W + 64
    acc, mag, slack, n = np.zeros((n_pix, C), dt), np.zeros((n_pix, C)), np.zeros((n_pix, C)), np.zeros(n_pix, np.int64)
    seen = set()
    for r in range(len(rois)):
        if mut == "roi_dedup":
            if tuple(rois[r]) in seen:
                continue
            seen.add(tuple(rois[r]))
        x0, y0, cw, ch = _geom(rois[r], H, W, mut)
        if cw <= 0 or ch <= 0:
            continue
        for oy in range(ps):
            ylo, yhi, ly, sy = _taps(ch, ps, oy, mut)
            for ox in range(ps):
                xlo, xhi, lx, sx = _taps(cw, ps, ox, mut)
                v = dy[r, oy, ox].astype(dt)
                for yy, wy in ((ylo, dt(1) - dt(ly)), (yhi, dt(ly))):          # the scatter order: top-low, top-high, bottom-low, bottom-high
                    for xx, wx in ((xlo, dt(1) - dt(lx)), (xhi, dt(lx))):
                        at = (y0 + yy) * W + x0 + xx
                        acc[at] = acc[at] + (v * wy) * wx
                        mag[at] += np.abs(v.astype(np.float64)) * float(wy) * float(wx)
                        slack[at] += np.abs(v.astype(np.float64)) * (sy * float(wx) + sx * float(wy))
                        n[at] += 1
    spilled = bool(n[H * W:].any())                                              # a mutant that writes behind the map
    acc, mag, n = acc[:H * W].reshape(H, W, C), mag[:H * W].reshape(H, W, C), n[:H * W].reshape(H, W, 1)
    slack = slack[:H * W].reshape(H, W, C)
    o64 = old.astype(np.float64)
    out = acc.astype(np.float64) if mut == "acc_ignored" else (old.astype(dt) + acc).astype(np.float64)
    out = np.where(n > 0, out, o64)
    tol = np.where(n > 0, (n + 4) * U * mag + U * slack + (2 if ordered else np.maximum(n, 2)) * U * np.abs(o64), 0.0)
    res = _out(out, tol, old=old)
    res["spilled"] = spilled
    return dict(dfmap=res)


# ================================================================================================================ avgpool
# radnet_avgpool_fwd(x, r, hw, c, y) / radnet_avgpool_bwd_relu(dfeat, y_act, r, hw, c, dx).  Contract: c % 4 == 0, r, hw >= 1 (the
# kernels divide by hw), fewer than 2^31 float4 work items in the backward.
AVGPOOL = [(1, 1, 4), (1, 49, 4), (3, 2, 8), (5, 49, 260), (2, 64, 12), (2, 100, 36)]


def avgpool_contract(r, hw, c):
    return c % 4 == 0 and c >= 4 and r >= 1 and hw >= 1 and r * hw * (c // 4) < 2 ** 31


@functools.lru_cache(maxsize=None)
def avgpool_inputs(i):
    r, hw, c = AVGPOOL[i]
    rs = np.random.RandomState(300 + i)
    return _frozen(dict(x=activations(rs, (r, hw, c)), g=_normal(rs, r, c)))


def ref_avgpool_fwd(x, mut=None):
    hw = x.shape[1]
    x64 = x.astype(np.float64)
    return dict(y=_out(x64.sum(1) / (49 if mut == "avg_div49" else hw), (hw + 1) * U * np.abs(x64).sum(1) / hw))


def ref_avgpool_bwd(g, act, mut=None):
    """One fp32 division per element: bit-exact."""
    hw = act.shape[1]
    q = (g.astype(F) / F(49 if mut == "avg_div49" else hw)).astype(F)
    live = act > 0
    return dict(dx=_out(np.where(live, q[:, None, :], F(0)).astype(np.float64), None, ~live))


# ================================================================================================================ dense_heads fwd
# radnet_dense_heads_fwd(feat, r, k, w, ldw, b, nc, nreg, out_cls, out_regr).  Contract: ldw in (32, 64), 1 <= nc, 0 <= nreg,
# nc + nreg <= ldw, r, k >= 1; w is [k][ldw], b [ldw]; the kernel multiplies every column of w but reads red[][n], b[n] for n < nout only.
DENSE_FWD = [(1, 4, 32, 2, 4), (3, 100, 32, 7, 24),
             (2, 300, 32, 1, 4),           # one class: softmax is 1
             (5, 256, 64, 13, 48),
             (1, 257, 64, 16, 48),         # nout == ldw
             (2, 4096, 64, 21, 40)]
# class biases spread over +-80 (the max-subtraction matters, some q underflow to exactly 0 in fp32) and, to give the mutant without the
# subtraction an fp32 overflow (expf(z[i] - mx) of dense_heads_fwd_kernel: expf alone overflows above 88.72), over +-100
DENSE_FWD_SPREAD = {1: 80.0, 3: 100.0}


def dense_contract(r, k, ldw, nc, nreg):
    return ldw in (32, 64) and nc >= 1 and nreg >= 0 and nc + nreg <= ldw and r >= 1 and k >= 1


def padded_wb(rs, k, ldw, nout, scale):
    w, b = np.full((k, ldw), PAD, F), np.full(ldw, PAD, F)
    w[:, :nout] = _normal(rs, k, nout) * F(scale)
    b[:nout] = _normal(rs, nout) * F(0.1)
    return w, b


@functools.lru_cache(maxsize=None)
def dense_fwd_inputs(i):
    r, k, ldw, nc, nreg = DENSE_FWD[i]
    rs = np.random.RandomState(400 + i)
    w, b = padded_wb(rs, k, ldw, nc + nreg, 0.02)
    if i in DENSE_FWD_SPREAD:
        b[:nc] = np.linspace(-DENSE_FWD_SPREAD[i], DENSE_FWD_SPREAD[i], nc).astype(F)
    return _frozen(dict(feat=_normal(rs, r, k), w=w, b=b))


def softmax(z, subtract_max=True):
    e = np.exp(z - z.max(-1, keepdims=True)) if subtract_max else np.exp(z)
    return e / e.sum(-1, keepdims=True)


def dense_logits(feat, w, b, nout, mut=None):
    """(z, tol) of feat @ w[:, :nout] + b[:nout] in float64."""
    f64, w64, b64 = feat.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    if mut == "pad_read":                                                        # w read with pitch nout: pad columns taken for data
        w64 = np.concatenate([w64.ravel(), np.zeros(w64.size)])[:w64.shape[0] * nout].reshape(-1, nout)
    else:
        w64 = w64[:, :nout]
    z = f64 @ w64 + (0.0 if mut == "no_bias" else b64[:nout])
    return z, (feat.shape[1] + 1) * U * (np.abs(f64) @ np.abs(w64) + np.abs(b64[:nout]))


def ref_dense_fwd(feat, w, b, nc, nreg, mut=None):
    z, tz = dense_logits(feat, w, b, nc + nreg, mut)
    if mut == "softmax_no_max":                                                  # the mutant's arithmetic is the device's: fp32 exp overflows
        with np.errstate(over="ignore", invalid="ignore"):
            q = softmax(z[:, :nc].astype(F), False).astype(np.float64)
    else:
        q = softmax(z[:, :nc])
    return dict(out_cls=_out(q, 1e-5 * np.abs(softmax(dense_logits(feat, w, b, nc + nreg)[0][:, :nc])).max()), out_regr=_out(z[:, nc:], tz[:, nc:]))


# ================================================================================================================ dense_heads bwd
# radnet_dense_heads_bwd(feat, dz, r, k, w, ldw, nout, dw, db, dfeat, accumulate).  Contract: ldw in (32, 64), 1 <= nout <= ldw, r, k >= 1,
# r * ldw * 4 <= 64 KiB of dynamic LDS; dz is dense [r][nout], dw [k][ldw], db [ldw]; columns >= nout of dw / db get (+)= 0.
DENSE_BWD = [(1, 4, 32, 31, 0), (20, 9, 32, 32, 1), (33, 100, 64, 37, 1), (64, 2048, 64, 64, 0),
             (20, 2048, 32, 31, 1),       # the training step's own call: `dw[kk * np + n] += v` at the workload's shape
             (512, 8, 32, 31, 0)]         # exactly 64 KiB of dynamic LDS, which the entry accepts


def dense_bwd_contract(r, k, ldw, nout, acc):
    return ldw in (32, 64) and 1 <= nout <= ldw and r >= 1 and k >= 1 and r * ldw * 4 <= 64 * 1024 and acc in (0, 1)


@functools.lru_cache(maxsize=None)
def dense_bwd_inputs(i):
    r, k, ldw, nout, acc = DENSE_BWD[i]
    rs = np.random.RandomState(500 + i)
    w, _ = padded_wb(rs, k, ldw, nout, 0.02)
    dw0, db0 = np.zeros((k, ldw), F), np.zeros(ldw, F)                            # pad columns of the old values are +0.0, as the engine keeps them
    dw0[:, :nout], db0[:nout] = _normal(rs, k, nout), _normal(rs, nout)
    return _frozen(dict(feat=_normal(rs, r, k), dz=_normal(rs, r, nout) * F(0.1), w=w, dw0=dw0, db0=db0))


def ref_dense_bwd(feat, dz, w, ldw, nout, acc, dw0, db0, mut=None):
    r, k = feat.shape
    f64, z64, w64 = feat.astype(np.float64), dz.astype(np.float64), w.astype(np.float64)[:, :nout]
    keep = acc and mut != "acc_ignored"
    pad = np.arange(ldw) >= nout
    dw, db = np.zeros((k, ldw)), np.zeros(ldw)
    dw[:, :nout], db[:nout] = f64.T @ z64, z64.sum(0)
    tw, tb = np.zeros((k, ldw)), np.zeros(ldw)
    tw[:, :nout], tb[:nout] = (r + acc) * U * (np.abs(f64).T @ np.abs(z64)), (r + acc) * U * np.abs(z64).sum(0)
    if acc:
        tw, tb = tw + 2 * U * np.abs(dw0.astype(np.float64)), tb + 2 * U * np.abs(db0.astype(np.float64))
    if keep:
        dw, db = dw + dw0, db + db0
    return dict(dw=_out(dw, tw, np.broadcast_to(pad, dw.shape), dw0 if acc else None), db=_out(db, tb, pad, db0 if acc else None),
                dfeat=_out(z64 @ w64.T, nout * U * (np.abs(z64) @ np.abs(w64).T)))


# ================================================================================================================ smooth-L1, detector rows
def smooth_l1(x, mut=None):
    """(value, derivative w.r.t. x) of losses.py's smooth-L1; the mutant switches at 2."""
    ax, thr = np.abs(x), (2.0 if mut == "l1_threshold" else 1.0)
    return np.where(ax <= thr, 0.5 * x * x, ax - 0.5), np.where(ax <= thr, x, np.sign(x))


def det_rows(q, pregr, y1, y2, mut=None):
    """The detector losses of ONE group of rows in float64: (dz [rows][nc + nreg], [cls, regr, accuracy])."""
    q, pregr, t = q.astype(np.float64), pregr.astype(np.float64), y1.astype(np.float64)
    rows, nreg = q.shape[0], pregr.shape[1]
    mask, tgt = y2[:, :nreg].astype(np.float64), y2[:, nreg:].astype(np.float64)
    S = q.sum(-1, keepdims=True)
    o = q / S
    oc = np.clip(o, LO, HI)
    ce = -(t * np.log(oc)).sum(-1)
    am_q = q.shape[1] - 1 - np.argmax(q[:, ::-1], -1) if mut == "acc_last_max" else first_argmax(q)
    accuracy = (first_argmax(t) == am_q).mean()
    ak = np.where((o >= LO) & (o <= HI), -t / oc, 0.0)
    dq = (ak - (ak * o).sum(-1, keepdims=True)) / S / rows
    dcls = q * (dq - (dq * q).sum(-1, keepdims=True))
    val, d = smooth_l1(tgt - pregr, mut)
    den = LOSS_EPS * rows * nreg + mask.sum()
    return np.concatenate([dcls, -(mask * d) / den], 1), np.array([ce.mean(), (mask * val).sum() / den, accuracy])


def _block_tol(ref, rtol):
    return rtol * float(np.abs(ref).max()) if ref.size else 0.0


def det_outputs(dz, losses, nc):
    """Full buffers of dz (class and regression blocks under their own tolerance) and the three losses of one group."""
    tol = np.concatenate([np.full(dz[:, :nc].shape, _block_tol(dz[:, :nc], 1e-4)), np.full(dz[:, nc:].shape, _block_tol(dz[:, nc:], 1e-5))], 1)
    return tol, np.array([1e-5 * abs(losses[0]) + 1e-7, 1e-5 * abs(losses[1]) + 1e-7, 1e-6])


def class_targets(rs, rows, nc, nreg, background=False):
    """One-hot y1 and [mask || 0] y2 of losses.py: class nc - 1 is the background, a foreground class masks its own 4 columns."""
    cls = np.full(rows, nc - 1) if background else rs.randint(0, nc, rows)
    y1 = np.eye(nc, dtype=F)[cls]
    lab = np.zeros((rows, nreg), F)
    for i, c in enumerate(cls):
        if c != nc - 1 and 4 * c + 4 <= nreg:
            lab[i, 4 * c:4 * c + 4] = 1
    return cls, y1, lab


# ================================================================================================================ rpn_loss
# radnet_rpn_loss(pred, ld_pred, y_cls, y_regr, m, a, bce_mode, dz, ld_dz, losses, scratch8).  Contract: m, a >= 1, ld_pred, ld_dz >= 5a;
# pred [m][ld_pred] = [sigmoid outputs (a) || regressions (4a) || pad], y_cls [m][2a] = [valid || overlap], y_regr [m][8a] = [mask || target];
# dz [m][ld_dz] is written in full, columns >= 5a with +0.0.
RPN = [(1, 1, 5, 5), (3, 2, 10, 12), (7, 12, 64, 64), (50, 9, 45, 64), (300, 12, 64, 80)]
RPN_LAYOUTS = ("general", "none_valid", "all_valid", "no_positive")


def rpn_contract(m, a, ld_pred, ld_dz):
    return m >= 1 and a >= 1 and ld_pred >= 5 * a and ld_dz >= 5 * a


@functools.lru_cache(maxsize=None)
def rpn_inputs(i, layout):
    m, a, ld_pred, _ = RPN[i]
    rs = np.random.RandomState(600 + 10 * i + RPN_LAYOUTS.index(layout))
    valid = (rs.uniform(size=(m, a)) < 0.3).astype(F)
    valid[0, 0] = 1
    ov = ((rs.uniform(size=(m, a)) < 0.5) * valid).astype(F)
    if layout == "none_valid":
        valid, ov = np.zeros((m, a), F), np.zeros((m, a), F)
    elif layout == "all_valid":
        valid = np.ones((m, a), F)
        ov = (rs.uniform(size=(m, a)) < 0.5).astype(F)
    elif layout == "no_positive":
        ov = np.zeros((m, a), F)
    elif m * a >= 2:
        ov[0, 0] = 1                                                              # at least one positive anchor
    pred = np.full((m, ld_pred), PAD, F)
    p = np.clip(1.0 / (1.0 + np.exp(-3.0 * rs.standard_normal((m, a)))), 2 * PMARGIN, 1 - 2 * PMARGIN).astype(F)
    at = np.argwhere(valid > 0)
    if layout in ("general", "all_valid") and len(at) >= 3:                       # predictions exactly 0 and exactly 1 at valid anchors
        p[tuple(at[0])], p[tuple(at[-1])] = 0.0, 1.0
    reg = _normal(rs, m, 4 * a)
    pred[:, :a], pred[:, a:5 * a] = p, reg
    mask = np.repeat(ov, 4, -1)
    tgt = targets_for(reg, l1_offsets(rs, reg.shape))
    return _frozen(dict(pred=pred, y_cls=np.concatenate([valid, ov], 1), y_regr=np.concatenate([mask, tgt], 1)))


def ref_rpn(pred, y_cls, y_regr, m, a, ld_dz, mode, mut=None):
    P = pred.astype(np.float64)
    P = P.ravel()[:m * 5 * a].reshape(m, 5 * a) if mut == "pad_read" else P[:, :5 * a]          # mutant: pred read with pitch 5a
    p, reg = P[:, :a], P[:, a:]
    valid, t = y_cls[:, :a].astype(np.float64), y_cls[:, a:].astype(np.float64)
    mask, tgt = y_regr[:, :4 * a].astype(np.float64), y_regr[:, 4 * a:].astype(np.float64)
    with np.errstate(all="ignore"):
        if mode == 0:                                                             # Keras-2 argument order: the logit of the clipped LABEL
            o = np.clip(t, LO, HI)
            l = np.log(o / (1.0 - o))
            ce, dce = np.maximum(l, 0) - l * p + np.log1p(np.exp(-np.abs(l))), -l
        else:
            pc = np.clip(p, LO, HI)
            z = np.log(pc / (1.0 - pc))
            ce = np.maximum(z, 0) - z * t + np.log1p(np.exp(-np.abs(z)))
            dce = np.where((p >= LO) & (p <= HI), (pc - t) / (pc * (1.0 - pc)), 0.0)
        den_c = (0.0 if mut == "rpn_no_eps" else LOSS_EPS * m * a) + valid.sum()
        den_r = (0.0 if mut == "rpn_no_eps" else LOSS_EPS * m * 4 * a) + mask.sum()
        val, d = smooth_l1(tgt - reg, mut)
        losses = np.array([(valid * ce).sum() / den_c, (mask * val).sum() / den_r])
        dz = np.zeros((m, ld_dz))
        dz[:, :a] = valid * dce / den_c * p * (1.0 - p)
        dz[:, a:5 * a] = -(mask * d) / den_r
    return dz, losses


def rpn_outputs(pred, y_cls, y_regr, m, a, ld_dz, mode, mut=None):
    dz, losses = ref_rpn(pred, y_cls, y_regr, m, a, ld_dz, mode, mut)
    ref_dz, ref_l = (dz, losses) if mut is None else ref_rpn(pred, y_cls, y_regr, m, a, ld_dz, mode)
    tol = np.zeros((m, ld_dz))
    tol[:, :a], tol[:, a:5 * a] = _block_tol(ref_dz[:, :a], 2e-5), _block_tol(ref_dz[:, a:5 * a], 2e-5)
    return dict(dz=_out(dz, tol, np.broadcast_to(np.arange(ld_dz) >= 5 * a, dz.shape)), losses=_out(losses, 2e-5 * np.abs(ref_l) + 1e-7))


# ================================================================================================================ det_loss
# radnet_det_loss(p_cls, p_regr, y1, y2, r, nc, nreg, dz, losses).  Contract: r, nc >= 1, nreg >= 0; one workgroup strides the rows by 256.
DET = [(1, 2, 4), (3, 7, 24), (20, 7, 24), (64, 13, 48),
       (257, 7, 24)]                      # thread 0 owns rows 0 and 256
DET_LAYOUTS = ("general", "all_background")


def det_contract(r, nc, nreg):
    return r >= 1 and nc >= 1 and nreg >= 0


def spread_argmax(q):
    """Raise the largest entry of every row whose two largest are closer than 10 * PMARGIN and not equal."""
    srt = np.sort(q, -1)
    near = (srt[:, -1] - srt[:, -2] < 10 * PMARGIN) & (srt[:, -1] != srt[:, -2])
    q[near, np.argmax(q[near], -1)] += F(20 * PMARGIN)
    return q


@functools.lru_cache(maxsize=None)
def det_inputs(i, layout):
    r, nc, nreg = DET[i]
    rs = np.random.RandomState(700 + 10 * i + DET_LAYOUTS.index(layout))
    q = np.clip(softmax(2.0 * rs.standard_normal((r, nc))), 10 * PMARGIN, 1 - 10 * PMARGIN).astype(F)
    q = spread_argmax(q)
    cls, y1, lab = class_targets(rs, r, nc, nreg, layout == "all_background")
    if r >= 3 and layout == "general":
        q[0] = 0                                                                  # exact zeros: clipped at 1e-7, out of range in the gradient
        q[0, 0], q[0, 1] = 0.25, 0.75
        y1[0] = np.eye(nc, dtype=F)[nc - 1]                                       # the label on a zero entry: ce = -log(1e-7)
        q[1] *= F(0.5)                                                            # rows that do not sum to 1: the re-normalisation
        if r > 3:
            q[2] *= F(2.0)
        q[r - 1] = F(0.25 / max(nc - 2, 1))                                       # an exact tie of the two largest, the label on the SECOND
        q[r - 1, 0] = q[r - 1, 1] = 0.375 if nc > 2 else 0.5
        y1[r - 1] = np.eye(nc, dtype=F)[1]
    pregr = _normal(rs, r, nreg)
    y2 = np.concatenate([lab, targets_for(pregr, l1_offsets(rs, pregr.shape))], 1)
    return _frozen(dict(q=q, pregr=pregr, y1=y1, y2=y2))


def ref_det(q, pregr, y1, y2, mut=None):
    nc = q.shape[1]
    dz, losses = det_rows(q, pregr, y1, y2, mut)
    tol, tl = det_outputs(*det_rows(q, pregr, y1, y2), nc)
    return dict(dz=_out(dz, tol), losses=_out(losses, tl))


# ================================================================================================================ head_tail_fwd
# radnet_head_tail_fwd(y5, r, hw, c, w, ldw, b, nc, nreg, feat, p_cls, p_regr, y1, y2, dz, losses, groups, group_live, scratch).
# Contract: r, hw, nc >= 1, nreg >= 0, ldw in (32, 64), nc + nreg <= ldw, c % 32 == 0 and c / 32 <= 64 (eight channel slices of at most
# 64 float4 columns), 1 <= groups <= 256, r % groups == 0, y1 given -> y2, dz, losses given, scratch of radnet_head_tail_scratch_bytes(r)
# bytes, zero before the first launch.  The kernel hands off by last-arriver tickets and never waits.
HeadTail = collections.namedtuple("HeadTail", "R hw c ldw nc nreg groups idle")
HEAD_TAIL = [HeadTail(1, 1, 32, 32, 2, 4, 1, None),          # hw < 4: waves 1..3 have no position; one column per slice
             HeadTail(6, 3, 96, 32, 7, 24, 1, None),          # 3 columns per slice: col_ok false in 61 lanes
             HeadTail(6, 16, 32, 64, 13, 48, 2, 0),           # the <64> kernel, first group idle
             HeadTail(6, 49, 96, 64, 16, 48, 6, 5),           # nout == ldw, one row per group, last group idle
             HeadTail(6, 64, 32, 32, 7, 24, 2, None),         # the register window exactly full
             HeadTail(6, 65, 96, 32, 7, 24, 6, 0),            # the tail loop runs in wave 0 only
             HeadTail(40, 100, 32, 64, 21, 40, 2, 1),         # nine tail-loop passes, 20 rows per group
             HeadTail(6, 65, 2048, 32, 7, 24, 2, 1),          # the workload's channel count with a tail loop
             HeadTail(1, 100, 2048, 64, 13, 48, 1, None)]


def head_tail_contract(cs):
    return (min(cs.R, cs.hw, cs.nc) >= 1 and cs.nreg >= 0 and cs.ldw in (32, 64) and cs.nc + cs.nreg <= cs.ldw and cs.c % 32 == 0
            and cs.c // 32 <= 64 and 1 <= cs.groups <= 256 and cs.R % cs.groups == 0 and (cs.idle is None or 0 <= cs.idle < cs.groups))


def head_forward(y5, w, b, nc, nreg, mut=None):
    """(feat, tol_feat, z, tol_z, q) of the float64 chain average pool -> dense -> softmax."""
    hw = y5.shape[1]
    x64 = y5.astype(np.float64)
    pooled = x64[:, :64] if mut == "tail_drop_64" else x64
    feat = pooled.sum(1) / (49 if mut == "avg_div49" else hw)
    tf = (hw + 1) * U * np.abs(x64).sum(1) / hw
    nout = nc + nreg
    w64, b64 = w.astype(np.float64)[:, :nout], b.astype(np.float64)[:nout]
    z = feat @ w64 + (0.0 if mut == "no_bias" else b64)
    tz = (y5.shape[2] + 1) * U * (np.abs(feat) @ np.abs(w64) + np.abs(b64)) + tf @ np.abs(w64)
    return feat, tf, z, tz, softmax(z[:, :nc])


@functools.lru_cache(maxsize=None)
def head_tail_inputs(i):
    cs = HEAD_TAIL[i]
    rs = np.random.RandomState(800 + i)
    y5 = activations(rs, (cs.R, cs.hw, cs.c), relu=True)
    y5[y5 == 0] = F(0)                                                            # post-ReLU activations: no -0.0
    w, b = padded_wb(rs, cs.c, cs.ldw, cs.nc + cs.nreg, 2.0 / np.sqrt(cs.c))
    z = head_forward(y5, w, b, cs.nc, cs.nreg)[2]
    _, y1, lab = class_targets(rs, cs.R, cs.nc, cs.nreg)
    pregr = z[:, cs.nc:].astype(F)
    d = l1_offsets(rs, pregr.shape)
    d[d == 0] = F(0.5)                                                            # the device's own p_regr is subtracted: no exact zero here
    y2 = np.concatenate([lab, targets_for(pregr, d)], 1)
    live = np.array([0 if cs.idle == g else 1 for g in range(cs.groups)], np.int32)
    return _frozen(dict(y5=y5, w=w, b=b, y1=y1, y2=y2, live=live))


def ref_head_tail(cs, y5, w, b, y1, y2, live, targets=True, mut=None):
    """Full buffers of feat, p_cls, p_regr and, with targets, dz and losses [groups][3]."""
    feat, tf, z, tz, q = head_forward(y5, w, b, cs.nc, cs.nreg, mut)
    _, _, z0, _, q0 = head_forward(y5, w, b, cs.nc, cs.nreg)
    rg = cs.R // cs.groups
    tq = np.concatenate([np.full((rg, cs.nc), _block_tol(q0[g * rg:(g + 1) * rg], 1e-5)) for g in range(cs.groups)])
    res = dict(feat=_out(feat, tf), p_cls=_out(q, tq), p_regr=_out(z[:, cs.nc:], tz[:, cs.nc:]))
    if not targets:
        return res
    nout = cs.nc + cs.nreg
    dz, tol, zero = np.zeros((cs.R, nout)), np.zeros((cs.R, nout)), np.zeros((cs.R, nout), bool)
    losses, tl = np.full((cs.groups, 3), np.nan), np.zeros((cs.groups, 3))
    for g in range(cs.groups):
        rows = slice(g * rg, (g + 1) * rg)
        if not live[g] and mut != "idle_live":
            zero[rows] = True
            continue
        norm = slice(0, cs.R) if mut == "det_batch_norm" else rows                # mutant: one normaliser for the whole batch
        d, l = det_rows(q[norm], z[norm, cs.nc:], y1[norm], y2[norm], mut)
        dz[rows] = d[rows] if mut == "det_batch_norm" else d
        d0, l0 = det_rows(q0[rows], z0[rows, cs.nc:], y1[rows], y2[rows])
        tol[rows], tl[g] = det_outputs(d0, l0, cs.nc)
        if live[g]:
            losses[g] = l
    res.update(dz=_out(dz, tol, zero), losses=_out(losses, tl))
    return res
