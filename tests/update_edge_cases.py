"""Shared case tables, float64 references, per-element bounds and input builders of the edge tests of the optimizer and of the gradient
glue: csrc/adam.hip (radnet_adam_step, _affine, _fused, _bf16) and the kernels at the end of csrc/elementwise.hip (radnet_colsum,
radnet_scatter_strided, radnet_relu_mask, radnet_scale, radnet_affine_vec, radnet_preprocess_bgr).  Device-free check of the tables, the
references and their teeth: tests/test_update_edge_cases_reference.py; the kernels: tests/test_gpu_update_edges.py.  NumPy only: no torch,
no library.  The buffer conventions (SENTINEL prefill, TAIL floats behind every output, full-buffer references with inside / tol / zero /
old) are those of head_edge_cases.py, whose `_out` builds every fp32 output here.

Adam (Keras 2 rule), every reference in float64 on the fp32 input values; the betas, lr, eps and grad_scale are the fp32 values widened:

  lr_t = fl32(lr * sqrt(1 - b2^t) / (1 - b1^t))  in double, as adam_lr_t computes it (at t = 100000 both powers vanish: lr_t = lr)
  gq = g * gs;  m' = b1 m + (1 - b1) gq;  v' = b2 v + (1 - b2) gq^2;  p' = p - lr_t m' / (sqrt(v') + eps)
  g' = +0.0 with zero_grad, else g keeps its bits.

p, m, v, g are judged against float64 from the step's INPUTS; every step starts from fp32 state both sides share (no bound compounds).
What an entry point derives from the new weights is judged against the DEVICE's own new p, so it is exact or tightly bounded whatever
Adam's tolerance is:

  shift        = scale * p' + t0 on the bias range ................................. 2 U (|scale p'| + |t0|), fused or not
  Winograd u   = stage_filter(p' of a listed [3][3][c][n] layer, form 4) of winograd_edge_cases.py, with that module's bound
  bf16 image   [n][ldk] of a listed [k][ldw] layer: p' rounded to nearest even, transposed; columns k..ldk exactly 0 ........ bit for bit
               (fp32 columns n..ldw are updated by Adam and reach no image element)

Bounds, U = 2^-24, gamma(k) = k U / (1 - k U) (k roundings compounded; the first-order count is k U).  Every operation counts as one
rounding, counted along the association csrc/adam.hip writes; the unit is compiled with contraction allowed, so any a*b + c may lose the
rounding of its product -- the count below is the unfused one, the fused forms only remove roundings:

  1 - b1, 1 - b2   exact for betas in [0.5, 1) (Sterbenz): the reference's float64 difference is the same number.  0 roundings.
  m' = b1*m + (1 - b1)*gq     the second term passes g*gs, the multiply, the add: 3.  tol_m = gamma(3) (|b1 m| + |(1 - b1) gq|)
  v' = b2*v + ((1 - b2)*gq)*gq  gq enters twice (2), two multiplies (2), the add (1): 5.  tol_v = gamma(5) (|b2 v| + (1 - b2) gq^2)
  p' = p - (lr_t*m') / (sqrtf(v') + eps), step = lr_t m' / (sqrt(v') + eps):
       tol_p = tol_m lr_t / (sqrt(v') + eps)                                           the device's m' carried through
             + tol_v |m'| lr_t / (2 sqrt(v_lo) (sqrt(v_lo) + eps)^2), v_lo = v' - tol_v   the device's v' carried through (the function is
                                                                                       convex in v': its slope at the lower end bounds the
                                                                                       difference); v' = 0: eps stands for sqrt, tol_v = 0
             + gamma(7) |step|    sqrtf 2, the add of eps 1, lr_t*m' 1, the division 2 (neither assumed correctly rounded), lr_t itself 1
             + U (|p| + |step|)   the subtraction
       An element with g = m = 0 has m' = 0 on both sides: p - 0 is exact, tol_p = 0 (p keeps its bits).
The constants come from this count, not from a device run.  DESIGN.md records the measured worst err / tol per quantity.

Inputs.  No intermediate is subnormal: gradients and moments are exactly 0 or large enough (|g| >= 1e-3, |m| >= 1e-6, v >= 1e-8) that
every product stays normal; `borderline_adam` counts intermediates that are neither 0 nor >= 2^-120 in magnitude and the CPU test asserts
zero, so no element is skipped.  Element classes, by position (an arena of n >= 8 holds them all; the n = 4 arena the first four):
  0 g = m = v = 0 (p must keep its bits)   1 v = 0, m != 0   2 g = 0, moments set   3 large v (up to 1e6)   4 m < 0   5 m > 0   6, 7 generic

Glue kernels (bit-exact unless a bound is stated):
  colsum           out[n] (+)= gscale[n] * sum_m g[m][n]: (rows + 1) U sum|g| |gscale| + 2 U |old| in any order of the additions; pad
                   columns n..ld hold 1e30 and reach nothing
  scatter_strided  dst[b][ih][iw] = src[b][ih/s][iw/s] where s divides both and the quotient lies inside oh x ow, +0.0 elsewhere; then
                   mask > 0 ? v : +0.0
  relu_mask        g = act > 0 ? g : +0.0 in place (a NaN activation gives +0.0)
  scale            x = fl32(x * alpha) in place
  affine_vec       out = a * b + c: 2 U (|a b| + |c|), fused or not
  preprocess_bgr   out[pix][0..3) = fl32(img[pix][0..3) - (103.939f, 116.779f, 123.68f)), channels 3..cpad +0.0"""
import collections
import functools
import math

import numpy as np

import head_edge_cases as H
import winograd_edge_cases as W

U, SENTINEL, TAIL, PAD, F = H.U, H.SENTINEL, H.TAIL, H.PAD, H.F
assert SENTINEL == np.uint32(0x7FC5A5A5) and TAIL == 64 and W.SENTINEL == SENTINEL and W.TAIL == TAIL
_out, _frozen = H._out, H._frozen
NORMAL_MIN = 2.0 ** -120                  # what `borderline_adam` asks of every non-zero intermediate (fp32 normals start at 2^-126)

MUTANTS = ("gs_once", "v_no_square", "eps_inside_sqrt", "lr_not_corrected", "stride_skips_gap", "shift_from_old_p", "bias_off_by_chunk",
           "image_truncates", "image_pad_kept", "image_untransposed", "wino_from_old_p", "colsum_drop_last_row_block",
           "colsum_scale_before_old", "scatter_no_bound", "mask_ge", "nan_passes", "preprocess_rgb_order")


def gamma(k):
    return k * U / (1.0 - k * U)


# ---------------------------------------------------------------------------------------------------------------- Adam: the step
LR, B1, B2, EPS = F(1e-3), F(0.9), F(0.999), F(1e-7)
assert 0.5 <= B1 < 1 and 0.5 <= B2 < 1                # 1 - beta is exact in fp32
STEPS_T = (1, 2, 10, 1000, 100000)
GRAD_SCALES = (F(1.0), F(0.5), F(0.25), F(1.0 / 3.0))
SWEEP_CAP = 8192 * 256                    # float4 chunks one pass of the flat sweep covers (adam_gaps: grid_for(..., 256, 8192))
WINO_MAX, BF16_MAX = 12, 16


def lr_t(t, lr=LR, b1=B1, b2=B2):
    """adam_lr_t of csrc/adam.hip: double arithmetic on the widened fp32 values, rounded to fp32 once."""
    return F(float(lr) * math.sqrt(1.0 - math.pow(float(b2), float(t))) / (1.0 - math.pow(float(b1), float(t))))


@functools.lru_cache(maxsize=None)
def adam_state(n, seed=0):
    """fp32 p, g, m, v of an arena of n floats with the element classes of the module docstring."""
    rs = np.random.RandomState(9000 + seed)
    sign = lambda: rs.choice([-1.0, 1.0], n)
    logu = lambda lo, hi: np.exp(rs.uniform(np.log(lo), np.log(hi), n))
    p = rs.standard_normal(n).astype(F)
    p[p == 0] = F(1.0)
    g = (sign() * logu(1e-3, 0.3)).astype(F)
    m = (sign() * logu(1e-6, 0.1)).astype(F)
    v = logu(1e-8, 0.1).astype(F)
    cls = np.arange(n) % 8
    if n >= 64:
        cls = rs.permutation(cls)
    g[(cls == 0) | (cls == 2)] = 0
    m[cls == 0] = 0
    v[(cls == 0) | (cls == 1)] = 0
    v[cls == 3] *= F(1e7)
    m[cls == 4] = -np.abs(m[cls == 4])
    m[cls == 5] = np.abs(m[cls == 5])
    return _frozen(dict(p=p, g=g, m=m, v=v, cls=cls))


def _adam64(p, g, m, v, t, gs, mut=None):
    """One step in float64 -> (p', m', v', step, the magnitudes the bounds multiply)."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    b1, b2, eps, gsd = float(B1), float(B2), float(EPS), float(F(gs))
    lrt = float(LR) if mut == "lr_not_corrected" else float(lr_t(t))
    gq = g * gsd
    gv = g if mut == "gs_once" else gq
    tm = (np.abs(b1 * m), np.abs((1.0 - b1) * gq))
    m2 = b1 * m + (1.0 - b1) * gq
    sq = np.abs(gv) if mut == "v_no_square" else gv * gv
    tv = (b2 * v, (1.0 - b2) * sq)
    v2 = tv[0] + tv[1]
    den = np.sqrt(v2 + eps) if mut == "eps_inside_sqrt" else np.sqrt(v2) + eps
    step = lrt * m2 / den
    return p - step, m2, v2, step, tm, tv, lrt


def adam_refs(p, g, m, v, t, gs, mut=None):
    """-> dict(p, m, v): the full buffers (arena + TAIL) of one step from the fp32 state p, g, m, v; `old` is the input state."""
    p2, m2, v2, step, tm, tv, lrt = _adam64(p, g, m, v, t, gs, mut)
    eps = float(EPS)
    tol_m = gamma(3) * (tm[0] + tm[1])
    tol_v = gamma(5) * (tv[0] + tv[1])
    rv = np.sqrt(v2)
    rlo = np.where(v2 > 0, np.sqrt(np.maximum(v2 - tol_v, 0.0)), eps)
    carry_m = tol_m * lrt / (rv + eps)
    carry_v = tol_v * np.abs(m2) * lrt / (2.0 * rlo * (rlo + eps) ** 2)
    p64 = np.asarray(p, np.float64)
    tol_p = carry_m + carry_v + gamma(7) * np.abs(step) + U * (np.abs(p64) + np.abs(step))
    tol_p = np.where((np.asarray(g) == 0) & (np.asarray(m) == 0), 0.0, tol_p)
    return dict(p=_out(p2, tol_p, old=p), m=_out(m2, tol_m, old=m), v=_out(v2, tol_v, old=v))


@functools.lru_cache(maxsize=None)
def layout_refs(name, t, gs):
    """adam_refs of the layout's own input state, computed once and shared (the layer table changes no element of p, m, v)."""
    st = adam_state(LAYOUTS[name].n)
    return _frozen(adam_refs(st["p"], st["g"], st["m"], st["v"], t, gs))


def ref_g(g, zero_grad):
    """The gradient arena after the step: +0.0 everywhere with zero_grad, the old bits without."""
    g = np.asarray(g, F)
    if zero_grad:
        return _out(np.zeros(g.shape), zero=np.ones(g.shape, bool), old=g)
    return _out(g.astype(np.float64), old=g)


def borderline_adam(p, g, m, v, t, gs):
    """Intermediates of the step that are neither exactly 0 nor normal with room to spare (the bound counts relative roundings)."""
    g64, m64, v64 = (np.asarray(x, np.float64) for x in (g, m, v))
    p2, m2, v2, step, tm, tv, lrt = _adam64(p, g, m, v, t, gs)
    gq = g64 * float(F(gs))
    vals = [g64, m64, v64, gq, tm[0], tm[1], m2, (1.0 - float(B2)) * gq, tv[0], tv[1], v2, np.sqrt(v2), lrt * m2, step, p2]
    return int(sum(((x != 0) & (np.abs(x) < NORMAL_MIN)).sum() for x in vals))


def _fma(a, b, c):
    """fl32(a * b + c) with the product unrounded: the fp32 product is exact in float64."""
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def adam_emulate(p, g, m, v, t, gs, fuse=None):
    """Honest fp32 arithmetic in the kernel's association.  fuse: None (every product rounded), "first" (b*x + t with the FIRST product
    of each sum contracted) or "second" (the second one) -- a sum of two products can lose the rounding of one of them only."""
    p, g, m, v = (np.asarray(x, F) for x in (p, g, m, v))
    c1, c2, lrt = F(1) - B1, F(1) - B2, lr_t(t)
    gq = g * F(gs)
    if fuse is None:
        m2 = B1 * m + c1 * gq
        v2 = B2 * v + c2 * gq * gq
    elif fuse == "first":
        m2 = _fma(m, B1, c1 * gq)
        v2 = _fma(v, B2, c2 * gq * gq)
    else:
        m2 = _fma(gq, c1, B1 * m)
        v2 = _fma(c2 * gq, gq, B2 * v)
    p2 = p - lrt * m2 / (np.sqrt(v2) + EPS)
    assert p2.dtype == F and m2.dtype == F and v2.dtype == F
    return p2, m2, v2


# ---------------------------------------------------------------------------------------------------------------- Adam: what is derived
def bias_inputs(bias_len, seed=0):
    rs = np.random.RandomState(9500 + seed)
    k = max(bias_len, 4)
    return _frozen(dict(scale=(rs.uniform(0.5, 1.5, k) * rs.choice([-1.0, 1.0], k)).astype(F), t0=rs.standard_normal(k).astype(F)))


def ref_shift(p_new, scale, t0, bias_off, bias_len, p_old=None, mut=None):
    """shift[j] = scale[j] * p'[bias_off + j] + t0[j], j < bias_len, from the DEVICE's new weights p_new (the whole arena)."""
    src = p_old if mut == "shift_from_old_p" else p_new
    at = bias_off + (4 if mut == "bias_off_by_chunk" else 0)
    pb = np.asarray(src, np.float64)[at:at + bias_len]
    if pb.size < bias_len:                                                     # the off-by-a-chunk mutant at the arena's end wraps
        pb = np.concatenate([pb, np.asarray(src, np.float64)[:bias_len - pb.size]])
    sc, c = np.asarray(scale, np.float64)[:bias_len], np.asarray(t0, np.float64)[:bias_len]
    return _out(sc * pb + c, 2 * U * (np.abs(sc * pb) + np.abs(c)))


def shift_emulate(p_new, scale, t0, bias_off, bias_len, fuse=False):
    pb = np.asarray(p_new, F)[bias_off:bias_off + bias_len]
    sc, c = np.asarray(scale, F)[:bias_len], np.asarray(t0, F)[:bias_len]
    return _fma(sc, pb, c) if fuse else sc * pb + c


def ref_wino(p_new, off, c, n, p_old=None, mut=None):
    """u [36][c][n] of the dense [3][3][c][n] layer at float `off` of the arena: winograd_edge_cases.stage_filter, form 4."""
    src = p_old if mut == "wino_from_old_p" else p_new
    res = W.stage_filter(np.asarray(src, F)[off:off + 9 * c * n].reshape(9 * c, n), c, n, n, 4)
    res["zero"] = np.zeros(res["inside"].shape, bool)
    return res


def wino_emulate(p_new, off, c, n):
    return W.stage_filter(np.asarray(p_new, F)[off:off + 9 * c * n].reshape(9 * c, n), c, n, n, 4, arith="kernel")["buf"][:36 * c * n]


def to_bf16(x, truncate=False):
    """fp32 -> the bits of bf16, to nearest, ties to even (finite values)."""
    b = np.ascontiguousarray(x, F).view(np.uint32)
    if truncate:
        return (b >> np.uint32(16)).astype(np.uint16)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def sentinel_halves(count):
    """`count` (even) 16-bit words of the sentinel prefill, as the device holds them."""
    assert count % 2 == 0
    return np.full(count // 2, SENTINEL, np.uint32).view(np.uint16)


def ref_bf16_image(p_new, off, k, n, ldw, ldk, mut=None):
    """The whole image buffer as 16-bit words: [n][ldk] then 2 * TAIL sentinel halves.  Column j < k of row i holds bf16(p'[j][i]),
    columns k..ldk hold 0; every word of the image is written."""
    w = np.asarray(p_new, F)[off:off + k * ldw].reshape(k, ldw)
    img = sentinel_halves(n * ldk).reshape(n, ldk).copy() if mut == "image_pad_kept" else np.zeros((n, ldk), np.uint16)
    bits = to_bf16(w[:, :n], truncate=mut == "image_truncates")
    if mut == "image_untransposed":
        flat = img.reshape(-1)
        flat[:k * n] = bits.reshape(-1)                                       # [k][n] laid down as it lies in the arena
    else:
        img[:, :k] = bits.T
    return np.concatenate([img.reshape(-1), sentinel_halves(2 * TAIL)])


# ---------------------------------------------------------------------------------------------------------------- Adam: the layouts
# wino: (off, c, n) dense [3][3][c][n] kernels, c * n a multiple of 256.  bf16: (off, k, n, ldw, ldk) kernels [k][ldw] with an image
# [n][ldk].  bias: (off, len) or None.  entries: which entry points run the layout.  A Winograd table is ALSO a bf16 table (a dense
# [9c][n] kernel with ldk = 9c rounded up to 8), so every layout with Winograd layers runs through radnet_adam_step_bf16 as well.
Layout = collections.namedtuple("Layout", "name n wino bf16 bias entries")
_UNIT = 2304                              # floats of a [3][3][c][n] layer with c * n = 256


def wino_as_bf16(wino):
    return tuple((off, 9 * c, n, n, (9 * c + 7) // 8 * 8) for off, c, n in wino)


def _wino_layout(name, n, wino, bias):
    return Layout(name, n, tuple(wino), wino_as_bf16(wino), bias, ("fused", "bf16"))


def _plain_layout(name, n):
    # radnet_adam_step without a bias range; _affine, _fused with 0 layers and _bf16 with 0 layers with the WHOLE arena as the bias range
    return Layout(name, n, (), (), (0, n), ("adam", "affine", "fused", "bf16"))


_GAP3 = [(512, 16, 16), (512 + _UNIT + 512, 32, 8), (512 + 2 * (_UNIT + 512), 8, 32)]          # gaps [0, 512) [2816, 3328) [5632, 6144) [8448, 8960)
_N3 = 8960
_TWELVE_GAPS = (0, 4, 1028, 0, 256, 4, 12, 0, 2048, 4, 516, 8)          # floats in front of each of the twelve layers
_TWELVE = []
_at = 0
for _i, _gap in enumerate(_TWELVE_GAPS):
    _at += _gap
    _TWELVE.append((_at, (16, 64, 4, 8)[_i % 4], (16, 4, 64, 32)[_i % 4]))
    _at += _UNIT
_TWELVE_N = _at + 520
_SIXTEEN = []
_at = 0
for _i in range(16):
    _at += (0, 4, 260, 8)[_i % 4]
    _k, _n = 3 + 5 * _i, 4 + 4 * (_i % 5)
    _ldw = _n + (0, 4, 0, 8)[_i % 4]
    _SIXTEEN.append((_at, _k, _n, _ldw, (_k + 7) // 8 * 8 + (8 if _i % 3 == 0 else 0)))
    _at += _k * _ldw
_SIXTEEN_N = _at + 132
# tests/test_gpu_bf16_mixed.py's RAGGED rows, then: one row of one float4; exactly one tile; 65 x 68 (four tiles, three of them ragged);
# ldw = 128 with n = 60 (the second tile column is pad only)
RAGGED = ((0, 77, 100, 100, 96), (7700, 300, 60, 64, 304), (26900, 9, 8, 8, 40),
          (27256, 1, 4, 4, 8), (27264, 64, 64, 64, 64), (31424, 65, 68, 68, 72), (35904, 10, 60, 128, 16))
RAGGED_N = 35904 + 10 * 128 + 256
RAGGED_TILES = (4, 5, 1, 1, 1, 4, 2)      # cdiv(max(k, ldk), 64) * cdiv(ldw, 64)

# over_cap: 2,097,152 + 192 float4 chunks outside two layers of 576 chunks each.  Gap 0 holds 256 chunks; gap 1 ends 64 chunks past
# the first pass of the sweep, gap 2 holds the last 128: the second pass starts in gap 1 and ends in gap 2.  The bias range lies in
# gap 2, which only the second pass reaches.
OVER_REST4 = SWEEP_CAP + 192
_OA4 = 256
_OB4 = _OA4 + 576 + (SWEEP_CAP + 64 - 256)
OVER_N = 4 * (_OB4 + 576 + 128)
OVER_BIAS = (4 * (_OB4 + 576 + 32), 256)
assert OVER_N // 4 - 2 * 576 == OVER_REST4

_TABLE = [
    _plain_layout("tiny_4", 4),
    _plain_layout("tiny_1028", 1024 + 4),
    _wino_layout("interior", 5000 + 9 * 64 * 32 + 1024, [(64, 16, 16), (5000, 64, 32)], (5000 + 9 * 64 * 32 + 1024 - 256, 128)),
    _wino_layout("descending_adjacent", 20736 + 1024, [(2304, 64, 32), (0, 16, 16)], (20736 + 1024 - 256, 128)),
    _wino_layout("whole_arena", 20736, [(2304, 64, 32), (0, 16, 16)], None),
    _wino_layout("bias_in_first_gap", _N3, _GAP3, (128, 128)),
    _wino_layout("bias_in_middle_gap", _N3, _GAP3, (2944, 128)),
    _wino_layout("bias_in_last_gap", _N3, _GAP3, (8704, 128)),
    _wino_layout("bias_touches_layer_end", _N3, _GAP3, (2816, 128)),
    _wino_layout("twelve_layers", _TWELVE_N, _TWELVE, (_TWELVE_N - 260, 256)),
    Layout("sixteen_layers", _SIXTEEN_N, (), tuple(_SIXTEEN), (_SIXTEEN_N - 128, 64), ("bf16",)),
    Layout("ragged_bf16", RAGGED_N, (), RAGGED, (27000, 128), ("bf16",)),
    Layout("over_cap", OVER_N, ((4 * _OA4, 16, 16), (4 * _OB4, 64, 4)), ((4 * _OA4, 18, 100, 128, 24), (4 * _OB4, 36, 60, 64, 40)), OVER_BIAS,
           ("fused", "bf16")),
]
LAYOUTS = collections.OrderedDict((l.name, l) for l in _TABLE)
assert len(LAYOUTS) == len(_TABLE)
# (t, grad_scale) of the steps a layout runs, each from the layout's own input state: the tiny arenas take every t, every other arena but
# over_cap every scale
STEPS_ALL = tuple((t, GRAD_SCALES[i % 4]) for i, t in enumerate(STEPS_T)) + ((3, GRAD_SCALES[0]),)
STEPS_FOUR = ((1, GRAD_SCALES[3]), (1000, GRAD_SCALES[1]), (2, GRAD_SCALES[2]), (100000, GRAD_SCALES[0]))
STEPS_ONE = ((2, GRAD_SCALES[3]),)          # over_cap: one step (its float64 reference is the suite's largest), at the scale that is no power of two


def steps_of(name):
    return STEPS_ALL if name.startswith("tiny") else STEPS_ONE if name == "over_cap" else STEPS_FOUR


def layers_of(lay, entry):
    """The layer table `entry` ("adam", "affine", "fused", "bf16") passes for the layout."""
    return lay.wino if entry == "fused" else lay.bf16 if entry == "bf16" else ()


def layer_ranges(lay, entry):
    """[(off, len)] in floats of the listed layers, in arena order."""
    if entry == "fused":
        return sorted((off, 9 * c * n) for off, c, n in lay.wino)
    if entry == "bf16":
        return sorted((off, k * ldw) for off, k, n, ldw, ldk in lay.bf16)
    return []


def gap_table(n, ranges):
    """adam_gaps of csrc/adam.hip in float4 chunks: (gap0[], pref[]) -- the sweep's index j lies in gap q when pref[q] <= j < pref[q + 1]
    and stands for chunk gap0[q] + j - pref[q]."""
    gap0, pref, at = [], [0], 0
    for off, ln in list(ranges) + [(n, 0)]:
        assert off % 4 == 0 and ln % 4 == 0 and off // 4 >= at and off + ln <= n, "a layer leaves the arena or overlaps another"
        gap0.append(at)
        pref.append(pref[-1] + off // 4 - at)
        at = (off + ln) // 4
    return gap0, pref


def sweep_chunk(gap0, pref, j, mut=None):
    """The arena chunk the sweep's index j stands for, and its gap."""
    if mut == "stride_skips_gap" and j >= SWEEP_CAP:
        return j, None
    q = max(k for k in range(len(gap0)) if pref[k] <= j)
    return gap0[q] + j - pref[q], q


def gap_of_chunk(gap0, pref, chunk):
    """The gap that holds arena chunk `chunk`, or None inside a layer."""
    for q in range(len(gap0)):
        if gap0[q] <= chunk < gap0[q] + pref[q + 1] - pref[q]:
            return q
    return None


def bf16_tiles(k, n, ldw, ldk):
    return -(-max(k, ldk) // 64) * -(-ldw // 64)


def contract_violations(lay, entry):
    """What the host checks of csrc/adam.hip would refuse in the layout, as a list of strings (empty: inside the contract)."""
    bad = []
    if lay.n % 4 or lay.n < 0:
        bad.append("arena length")
    bias = lay.bias if entry != "adam" else None
    if bias and (bias[0] % 4 or bias[1] % 4 or bias[0] < 0 or bias[0] + bias[1] > lay.n):
        bad.append("bias range")
    if entry == "fused":
        if len(lay.wino) > WINO_MAX:
            bad.append("more than 12 layers")
        bad += ["layer %d" % off for off, c, n in lay.wino if c <= 0 or n <= 0 or n % 4 or (c * n // 4) % 64 or off % 4]
    if entry == "bf16":
        if len(lay.bf16) > BF16_MAX:
            bad.append("more than 16 layers")
        bad += ["layer %d" % off for off, k, n, ldw, ldk in lay.bf16 if k <= 0 or n <= 0 or ldw < n or ldw % 4 or off % 4 or ldk < k or ldk % 8]
    at = 0
    for off, ln in layer_ranges(lay, entry):
        if off < at or off + ln > lay.n:
            bad.append("layer at %d overlaps or leaves the arena" % off)
        if bias and off < bias[0] + bias[1] and bias[0] < off + ln:
            bad.append("layer at %d overlaps the bias range" % off)
        at = off + ln
    return bad


def stride_skips_gap(lay, entry, refs, state, t, gs):
    """Mutant: from its second pass on the sweep indexes the arena as if it had no layers.  The chunks the second pass should reach keep
    their old state; the chunks it reaches instead are stepped a second time.  -> the mutated float64 p, m, v (no tails)."""
    gap0, pref = gap_table(lay.n, layer_ranges(lay, entry))
    out = {k: refs[k]["buf"][:lay.n].copy() for k in "pmv"}
    js = np.arange(SWEEP_CAP, pref[-1])
    right = np.array([sweep_chunk(gap0, pref, int(j))[0] for j in js])
    for k in "pmv":
        for c in right:
            out[k][4 * c:4 * c + 4] = state[k][4 * c:4 * c + 4]
    idx = (4 * js[:, None] + np.arange(4)).ravel()
    again = _adam64(out["p"][idx], state["g"][idx], out["m"][idx], out["v"][idx], t, gs)
    out["p"][idx], out["m"][idx], out["v"][idx] = again[0], again[1], again[2]
    return out


# ---------------------------------------------------------------------------------------------------------------- colsum
COLSUM_M = (1, 3, 127, 128, 129, 513, 4096, 4097)
COLSUM_N = (1, 63, 64, 65, 100)
COLSUM_MODES = ((False, 0), (True, 0), (False, 1), (True, 1))          # (gscale?, accumulate)
COLSUM_ORDERED_ABOVE = 128                # the ordered form switches on for m > 128 (a single row block needs no order)
COLSUM_MAX_BLOCKS = 32


def colsum_rows_per_block(m, ordered):
    r = 128
    while ordered and m > 128 and -(-m // r) > COLSUM_MAX_BLOCKS:
        r *= 2
    return r


@functools.lru_cache(maxsize=None)
def colsum_inputs(m, n, ld):
    rs = np.random.RandomState(9600 + 7 * m + 131 * n + ld)
    g = np.full((m, ld), PAD, F)
    g[:, :n] = rs.standard_normal((m, n)).astype(F)
    return _frozen(dict(g=g, gscale=(rs.uniform(0.5, 1.5, n) * rs.choice([-1.0, 1.0], n)).astype(F), old=rs.standard_normal(n).astype(F)))


def ref_colsum(g, n, gscale, old, rows, mut=None):
    """out[n] + TAIL.  gscale / old: None or fp32 [n].  rows: the rows a block sums before the partial sums meet (the bound's count)."""
    x = np.asarray(g, np.float64)[:, :n]
    if mut == "colsum_drop_last_row_block":
        x = x[:(x.shape[0] - 1) // rows * rows]
    gs = np.ones(n) if gscale is None else np.asarray(gscale, np.float64)
    o = np.zeros(n) if old is None else np.asarray(old, np.float64)
    ref = (o + x.sum(0)) * gs if mut == "colsum_scale_before_old" else o + gs * x.sum(0)
    tol = (rows + 1) * U * np.abs(np.asarray(g, np.float64)[:, :n]).sum(0) * np.abs(gs) + 2 * U * np.abs(o)
    return _out(ref, tol, old=old)


def colsum_emulate(g, n, gscale, old, rows, ordered):
    """fp32: four interleaved row sums per block, the blocks' sums in order (ordered) or added to the output one by one (atomic)."""
    x = np.asarray(g, F)[:, :n]
    parts = []
    for r0 in range(0, x.shape[0], rows):
        blk = x[r0:r0 + rows]
        lanes = []
        for ty in range(4):
            s = np.zeros(n, F)
            for rr in range(ty, blk.shape[0], 4):
                s = s + blk[rr]
            lanes.append(s)
        parts.append(lanes[0] + lanes[1] + lanes[2] + lanes[3])
    out = np.zeros(n, F) if old is None else np.asarray(old, F).copy()
    gs = np.ones(n, F) if gscale is None else np.asarray(gscale, F)
    if ordered and len(parts) > 1:
        lanes = []
        for ty in range(4):
            s = np.zeros(n, F)
            for b in range(ty, len(parts), 4):
                s = s + parts[b]
            lanes.append(s)
        return out + ((lanes[0] + lanes[1]) + lanes[2] + lanes[3]) * gs
    for part in parts:
        out = out + part * gs
    return out


# ---------------------------------------------------------------------------------------------------------------- scatter_strided
SCATTER_OHW = (3, 4)
SCATTER_KINDS = ("tight", "whole", "one_more")          # h = (oh - 1) s + 1, oh s, oh s + 1
SCATTER_CAP = 8192 * 256                  # float4 elements one pass of the launch covers
SCATTER_OVER = (1, 725, 724, 4, 2, 1449, 1448, True)          # 1449 * 1448 = 2,098,152 float4 > 2,097,152
MASK_VALUES = (0.0, -0.0, -1.5, 2.5, np.nan)


def _extent(o, s, kind):
    return {"tight": (o - 1) * s + 1, "whole": o * s, "one_more": o * s + 1}[kind]


def scatter_cases():
    """(nb, oh, ow, c, s, h, w, mask?) -- every s, kind of h (w takes the NEXT kind), c, nb, with and without a mask."""
    oh, ow = SCATTER_OHW
    out = []
    for s in (1, 2, 3):
        for ki, kind in enumerate(SCATTER_KINDS):
            for c in (4, 12):
                for nb in (1, 2):
                    for mask in (False, True):
                        out.append((nb, oh, ow, c, s, _extent(oh, s, kind), _extent(ow, s, SCATTER_KINDS[(ki + 1) % 3]), mask))
    return out


def mask_values(rs, shape):
    """Activations that exercise the `> 0` decision: 0.0, -0.0, NaN, negative and positive values of magnitude >= 1e-3."""
    a = H.activations(rs, shape)
    flat = a.reshape(-1)
    flat[rs.randint(0, flat.size, max(1, flat.size // 16))] = F(np.nan)
    for i, val in enumerate(MASK_VALUES):                                      # every class is present whenever the buffer has room
        if i < flat.size:
            flat[(7 * i) % flat.size] = F(val)
    return a


@functools.lru_cache(maxsize=None)
def scatter_inputs(case):
    nb, oh, ow, c, s, h, w, mask = case
    rs = np.random.RandomState(9700 + sum(case[:7]) % 1000)
    src = rs.standard_normal((nb, oh, ow, c)).astype(F)
    src[src == 0] = F(1.0)
    return _frozen(dict(src=src, mask=mask_values(rs, (nb, h, w, c)) if mask else None))


def _passes(act, mut=None):
    act = np.asarray(act)
    if mut == "mask_ge":
        return act >= 0
    if mut == "nan_passes":
        return ~(act <= 0)
    return act > 0


def ref_scatter(src, s, h, w, mask, mut=None):
    nb, oh, ow, c = src.shape
    dst = np.zeros((nb, h, w, c))
    copied = np.zeros((nb, h, w, c), bool)
    rows = h if mut == "scatter_no_bound" else min(h, (oh - 1) * s + 1)
    nr, nc = len(range(0, rows, s)), len(range(0, min(w, (ow - 1) * s + 1), s))
    grid = np.asarray(src, np.float64)
    if nr > oh:                                                                 # the mutant reads the row behind the compact grid
        grid = np.concatenate([grid, np.full((nb, nr - oh, ow, c), 7.0)], 1)
    dst[:, 0:rows:s, 0:(ow - 1) * s + 1:s] = grid[:, :nr, :nc]
    copied[:, 0:rows:s, 0:(ow - 1) * s + 1:s] = True
    if mask is not None:
        keep = _passes(mask, mut)
        dst, copied = np.where(keep, dst, 0.0), copied & keep
    return _out(dst, zero=~copied)


# ---------------------------------------------------------------------------------------------------------------- relu_mask, scale, affine_vec
FLAT_CAP = 4096 * 256                     # elements one pass of relu_mask / scale / affine_vec / preprocess covers
FLAT_N = (1, 255, 256, 257, FLAT_CAP + 3)
ALPHAS = (F(0.0), F(-1.0), F(1.0 / 3.0))


@functools.lru_cache(maxsize=None)
def flat_inputs(n):
    rs = np.random.RandomState(9800 + n % 1000)
    x = rs.standard_normal(n).astype(F)
    x[x == 0] = F(1.0)
    return _frozen(dict(x=x, act=mask_values(rs, (n,)), a=rs.standard_normal(n).astype(F), b=rs.standard_normal(n).astype(F),
                        c=rs.standard_normal(n).astype(F)))


def ref_relu_mask(g, act, mut=None):
    keep = _passes(act, mut)
    return _out(np.where(keep, np.asarray(g, np.float64), 0.0), zero=~keep, old=g)


def ref_scale(x, alpha):
    return _out((np.asarray(x, F) * F(alpha)).astype(np.float64), old=x)


def ref_affine(a, b, c):
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    return _out(a * b + c, 2 * U * (np.abs(a * b) + np.abs(c)))


# ---------------------------------------------------------------------------------------------------------------- preprocess_bgr
MEANS = (F(103.939), F(116.779), F(123.68))
PREPROCESS = [(h, w, cpad) for h, w in ((1, 1), (15, 17), (257, 1)) for cpad in (3, 4, 8)] + [(1025, 1024, 4)]          # 1,049,600 pixels
assert 1025 * 1024 > FLAT_CAP


@functools.lru_cache(maxsize=None)
def preprocess_inputs(h, w):
    img = np.random.RandomState(9900 + h + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    img.reshape(-1)[:3] = (0, 255, 128)
    img.setflags(write=False)
    return img


def ref_preprocess(img, cpad, mut=None):
    h, w, _ = img.shape
    px = img[..., ::-1] if mut == "preprocess_rgb_order" else img
    out = np.zeros((h, w, cpad))
    zero = np.ones((h, w, cpad), bool)
    out[..., :3] = (px.astype(F) - np.array(MEANS, F)).astype(np.float64)
    zero[..., :3] = False
    return _out(out, zero=zero)
