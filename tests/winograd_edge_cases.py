"""Shared case table and NumPy references of the Winograd edge tests, one STAGE at a time (device-free check of the table, the
references and their teeth: tests/test_winograd_edge_cases_reference.py; the kernels: tests/test_gpu_winograd_edges.py).  No torch, no
library.

The path of a 3x3 'same' convolution through csrc/winograd.hip, for F(m x m, 3x3), m = `form` in (2, 4), a = m + 2, P = a * a:

  filter        u[p][c][n]   = (G g G^T)[p]                      g = w[3][3][c][ldw]
  input         v[p][tile][c] = (B^T d B)[p]                      d = the a x a patch of x[nb][h][w][c] at rows m*ti - 1 .., zero outside the image
  gemm_batched  m[p][tile][n] = sum_c v[p][tile][c] * u[p][c][n]
  output        y[pixel][ldy] = act((A^T m A) * scale + shift)     the m x m outputs of a tile that lie inside oh x ow
  dy            dz[p][tile][n] = (A g A^T)[p]                      g = fl32(dy * gscale), ONE fp32 multiply; zero outside oh x ow
  wgrad_batched du[p][c][n]  (+)= sum_tile v[p][tile][c] * dz[p][tile][n]
  filter_grad   dw[3][3][c][ldw] (+)= G^T du G

with p = a * xi + nu and tile = (img, ti, tj) in that order.  The matrices are the published ones (Lavin & Gray, "Fast Algorithms
for Convolutional Neural Networks", 2016: F(2x2,3x3) in section 4.1, F(4x4,3x3) in section 4.3), stated here as float64 literals.

Every transform is out = L1 x L2^T with two short fixed matrices.  Per element

  tol = s * 2^-24 * (|L1| |x| |L2|^T * |scale|) + 2 * 2^-24 * (|shift| + |old|)

s = 2 * (the largest number of roundings an input term passes through in one 1-D pass) + the epilogue's roundings.  The count, from
the association csrc/radnet_wino4.h and the F(2x2) kernels write, EVERY operation counted as one rounding (also the exact ones: a
multiplication by 2, 4, 8, 1/2, 1/4), an inexact constant (1/6, 1/12, 1/24) as one more:

  F(4x4)  bt6  o[0] = d0*4 + (d4 - d2*5): d2 is multiplied, subtracted, added ........................ 3   input        s = 6
          g6   u[1] = (s + g1) * (-1/6), s = g0 + g2: add, add, multiply, the constant .............. 4   filter       s = 8
          at6  o[3] = (d34*8 + d12) + m5, d34 = m3 - m4: subtract, multiply, add, add .............. 4   output       s = 8 + 2
          a6   z[3] = e4 + o2, o2 = y3*8 + y1*2: multiply, add, add ................................ 3   dy           s = 6 (+ 1)
          gt6  w[0] = u0/4 + (s12*(-1/6) + s34/24), s12 = u1 + u2: add, multiply, constant, add, add  5   filter_grad  s = 10 + 1
  F(2x2)  filter  ((w0 + w1) + w2) / 2: 3, s = 6;  input  d0 - d2: 1, s = 2;  output  (m0 + m1) + m2: 2, s = 4 + 2;
          dy  d0 + d1: 1, s = 2 (+ 1);  filter_grad  u0 + (u1 + u2)/2: 3, s = 6 + 1

The epilogue of the output stage is one multiply and one add (ReLU is exact), filter_grad's is the add to the old value.  The dy stage
with a gscale has one rounding more, the multiply dy * gscale: the reference rounds it to fp32 (g = fl32(dy * gscale), as
fp32_edge_cases.py states the operation), and so does a kernel that keeps the product in a register -- but the compiler may contract
v * gs and the first addition of the transform into one FMA, which does NOT round the product, so the two can differ by 2^-24 |g|
(fp32_edge_cases.py's "+ 8" covers the same multiply).  The first count here left that rounding to the reference alone; the F(2x2) dy
kernel then measured 1.05 of that bound at one element of s_5x7, every other stage below 1, and the count was corrected, not tuned:
without a gscale the dy stage keeps s = 6 / 2.  Everywhere else FMA contraction only removes roundings.
The batched GEMMs use the project's (K_red + 8) * 2^-24 * (sum|a*b| + |old|), K_red = c (gemm_batched) or tiles (wgrad_batched).

With the integer-valued inputs (|x| <= 8, power-of-two scale / gscale, integer shift and old values) every intermediate of input,
output and dy of both forms, and of filter and filter_grad of F(2x2), is a small multiple of 1/4: exact in fp32 in any association.

`stage(...)` gives a stage's FULL output buffer in float64 -- every element of the tensor the kernel writes into, pitch padding, one
extra row (or TAIL extra floats) included, NaN where nothing may be written -- the mask of the elements inside the rows and the bound.
Inputs with a pitch are read through it (NaN in their padding), so the mutants of the CPU test are the same code with one parameter
changed."""
import collections
import functools

import numpy as np

U = 2.0 ** -24
SENTINEL = np.uint32(0x7FC5A5A5)          # a quiet NaN no kernel produces: the prefill of every output element
TAIL = 64                                 # floats behind a dense output (u, v, m, dz, du) that must keep the sentinel

# ---------------------------------------------------------------------------------------------------------------- matrices
BT2 = np.array([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]])
G2 = np.array([[1., 0., 0.], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0., 0., 1.]])
AT2 = np.array([[1., 1., 1., 0.], [0., 1., -1., -1.]])
BT4 = np.array([[4., 0., -5., 0., 1., 0.], [0., -4., -4., 1., 1., 0.], [0., 4., -4., -1., 1., 0.],
                [0., -2., -1., 2., 1., 0.], [0., 2., -1., -2., 1., 0.], [0., 4., 0., -5., 0., 1.]])
G4 = np.array([[1. / 4., 0., 0.], [-1. / 6., -1. / 6., -1. / 6.], [-1. / 6., 1. / 6., -1. / 6.],
               [1. / 24., 1. / 12., 1. / 6.], [1. / 24., -1. / 12., 1. / 6.], [0., 0., 1.]])
AT4 = np.array([[1., 1., 1., 1., 1., 0.], [0., 1., -1., 2., -2., 0.], [0., 1., 1., 4., 4., 0.], [0., 1., -1., 8., -8., 1.]])
FORMS = (2, 4)
STAGES = ("filter", "input", "output", "dy", "filter_grad")
S = {4: dict(filter=8, input=6, output=10, dy=6, filter_grad=11), 2: dict(filter=6, input=2, output=6, dy=2, filter_grad=7)}
EXACT = {4: ("input", "output", "dy"), 2: STAGES}          # stages whose integer-valued runs are exact in fp32
EPILOGUES = [(sc, sh, act) for sc in (True, False) for sh in (True, False) for act in (0, 1)]


def matrices(form, mut=None):
    """(L1 = L2 of each stage) of F(form x form, 3x3); `mut` changes one coefficient of the F(4x4) matrices (mutant 9)."""
    BT, G, AT = (BT4, G4, AT4) if form == 4 else (BT2, G2, AT2)
    if mut == "bt_5_to_4" and form == 4:
        BT = BT.copy()
        BT[0, 2] = -4.0
    if mut == "g_24_to_12" and form == 4:
        G = G.copy()
        G[3, 0] = 1.0 / 12.0
    return dict(filter=G, input=BT, output=AT, dy=AT.T, filter_grad=G.T)


# ---------------------------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple("Case", "name nb h w c n chain expect")
# chain: "" (transforms only), "f" (forward chain: c % 32 == 0, the batched GEMM's K tile) or "fg" (gradient chain too: c % 64 == 0,
# radnet_wgrad_batched refuses other channel counts -- the forward-only chained cases keep c = 32).
# expect[form] = (tiles, input units = tiles * c/4, output units = tiles * n/4, v2 workgroups of the input, of the output)
_TABLE = [
    Case("s_1x1", 1, 1, 1, 4, 4, "", {2: (1, 1, 1, 1, 1), 4: (1, 1, 1, 1, 1)}),                       # one pixel, one unit
    Case("s_1x5", 2, 1, 5, 4, 36, "", {2: (6, 6, 54, 1, 1), 4: (4, 4, 36, 1, 1)}),                    # h smaller than a tile, w = 1 mod 4
    Case("s_2x3", 3, 2, 3, 36, 4, "", {2: (6, 54, 6, 1, 1), 4: (3, 27, 3, 1, 1)}),                    # one tile per image, three images
    Case("s_3x2", 2, 3, 2, 4, 68, "", {2: (4, 4, 68, 1, 2), 4: (2, 2, 34, 1, 1)}),
    Case("s_4x4", 1, 4, 4, 36, 36, "", {2: (4, 36, 36, 1, 1), 4: (1, 9, 9, 1, 1)}),                   # exactly one F(4x4) tile
    Case("s_5x7", 3, 5, 7, 36, 36, "", {2: (36, 324, 324, 6, 6), 4: (12, 108, 108, 2, 2)}),           # 108 = 64 + 44 v2 units
    Case("s_6x9", 2, 6, 9, 4, 4, "", {2: (30, 30, 30, 1, 1), 4: (12, 12, 12, 1, 1)}),
    Case("s_7x8", 2, 7, 8, 36, 68, "", {2: (32, 288, 544, 5, 9), 4: (8, 72, 136, 2, 3)}),
    Case("g_9x11", 2, 9, 11, 68, 68, "", {2: (60, 1020, 1020, 16, 16), 4: (18, 306, 306, 5, 5)}),     # > 256 units: 4 / 2 grid-stride blocks
    Case("c_1x1", 1, 1, 1, 32, 4, "f", {2: (1, 8, 1, 1, 1), 4: (1, 8, 1, 1, 1)}),                     # T = 1, one K tile, n = 4
    Case("c_5x7", 2, 5, 7, 32, 36, "f", {2: (24, 192, 216, 3, 4), 4: (8, 64, 72, 1, 2)}),
    Case("c_2x3", 2, 2, 3, 64, 4, "fg", {2: (4, 64, 4, 1, 1), 4: (2, 32, 2, 1, 1)}),
    Case("c_7x8", 3, 7, 8, 64, 68, "fg", {2: (48, 768, 816, 12, 13), 4: (12, 192, 204, 3, 4)}),
]
CASES = collections.OrderedDict((c.name, c) for c in _TABLE)
assert len(CASES) == len(_TABLE)

# radnet_gemm_batched / radnet_wgrad_batched alone: (batch, T, c, n).  wgrad_batched takes c % 64 == 0 only, so the c = 32 shapes
# run the forward GEMM alone (and the GPU test pins the refusal).
BATCHED = [(16, 1, 32, 4), (36, 23, 64, 36), (16, 75, 128, 96), (36, 75, 32, 36), (16, 23, 128, 4)]
GEMM_TILES = [(64, 64, 4), (64, 64, 8), (64, 128, 4), (128, 64, 4), (128, 128, 8), (32, 64, 4), (32, 32, 4)]
GEMM_PERSIST_TILES = ((64, 64), (32, 64), (64, 128), (32, 32))
GEMM_PERSIST_Z = (2, 3, -4, 5, 7, -12)


def gemm_shapes(batch, n):
    """[(bm, bn, slices, waves)] radnet_gemm_batched must run: the shapes test_batched_launches_xcd_contiguous_numbering_changes_no_bit
    forces -- every tile with slices 1 and -1, the persistent z forms on the 4-wave tiles that have one."""
    out = []
    for bm, bn, wv in GEMM_TILES:
        if bn > 64 and n <= 64:
            continue
        out += [(bm, bn, s, wv) for s in (1, -1)]
        if wv == 4 and (bm, bn) in GEMM_PERSIST_TILES:
            out += [(bm, bn, z, wv) for z in GEMM_PERSIST_Z if abs(z) <= batch]
    return out


def wgrad_shapes(c, n):
    """[(bmk, bn, slices)] radnet_wgrad_batched must run."""
    tiles = [(64, 64), (64, 128)] + ([(128, 64)] if c % 128 == 0 else [])
    return [(bmk, bn, s) for bmk, bn in tiles if not (bn > 64 and n <= 64) for s in (1, -1)]


def geometry(cs, form):
    th, tw = -(-cs.h // form), -(-cs.w // form)
    T = cs.nb * th * tw
    return dict(th=th, tw=tw, T=T, P=(form + 2) ** 2, rows=cs.nb * cs.h * cs.w, in_units=T * cs.c // 4, out_units=T * cs.n // 4,
                filter_units=cs.c * cs.n // 4)


def pitches(cs):
    return dict(ldw=cs.n + 4, ldy=cs.n + 8, ld_dy=cs.n + 12)


def padded(a, ld, fill=np.nan):
    """A [rows][cols] matrix laid out with pitch ld, `fill` in the padding."""
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


# ---------------------------------------------------------------------------------------------------------------- numbers
@functools.lru_cache(maxsize=None)
def inputs(name, form, ints=False):
    """fp32 inputs of every stage of a case, signed everywhere: normals, or integers in [-8, 8] with power-of-two scales."""
    cs = CASES[name]
    g = geometry(cs, form)
    rs = np.random.RandomState(7000 + 10 * list(CASES).index(name) + form + int(ints))
    if ints:
        f = lambda *shape: rs.randint(-8, 9, shape).astype(np.float32)
        sgn = lambda k: (2.0 ** rs.randint(-2, 3, k) * rs.choice([-1.0, 1.0], k)).astype(np.float32)
    else:
        f = lambda *shape: rs.standard_normal(shape).astype(np.float32)
        sgn = lambda k: (rs.uniform(0.5, 1.5, k) * rs.choice([-1.0, 1.0], k)).astype(np.float32)
    d = dict(w=f(9 * cs.c, cs.n), x=f(cs.nb, cs.h, cs.w, cs.c), m=f(g["P"], g["T"], cs.n), dy=f(g["rows"], cs.n),
             du=f(g["P"], cs.c, cs.n), dw0=f(9 * cs.c, cs.n), scale=sgn(cs.n), shift=f(cs.n), gscale=sgn(cs.n))
    for v in d.values():
        v.setflags(write=False)
    return d


# ---------------------------------------------------------------------------------------------------------------- 1-D transforms
# The associations csrc/radnet_wino4.h and the F(2x2) kernels of csrc/winograd.hip write, on lists of arrays of any float type.
def _k(x, v):
    return x.dtype.type(v)


def bt6(d):
    p, q = d[4] - d[2] * _k(d[0], 4), d[3] - d[1] * _k(d[0], 4)
    r, t = d[4] - d[2], (d[3] - d[1]) * _k(d[0], 2)
    return [d[0] * _k(d[0], 4) + (d[4] - d[2] * _k(d[0], 5)), p + q, p - q, r + t, r - t, d[1] * _k(d[0], 4) + (d[5] - d[3] * _k(d[0], 5))]


def at6(m):
    s12, d12, s34, d34 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return [(m[0] + s12) + s34, d34 * _k(m[0], 2) + d12, s34 * _k(m[0], 4) + s12, (d34 * _k(m[0], 8) + d12) + m[5]]


def a6(y):
    e, o = y[0] + y[2], y[1] + y[3]
    e4, o2 = y[2] * _k(y[0], 4) + y[0], y[3] * _k(y[0], 8) + y[1] * _k(y[0], 2)
    return [y[0], e + o, e - o, e4 + o2, e4 - o2, y[3]]


def g6(g):
    s = g[0] + g[2]
    m6 = _k(g[0], -1.0 / 6.0)
    a, b = g[0] * _k(g[0], 1.0 / 24.0) + g[2] * _k(g[0], 1.0 / 6.0), g[1] * _k(g[0], 1.0 / 12.0)
    return [g[0] * _k(g[0], 0.25), (s + g[1]) * m6, (s - g[1]) * m6, a + b, a - b, g[2]]


def gt6(u):
    s12, s34 = u[1] + u[2], u[3] + u[4]
    m6, p6, p12, p24 = (_k(u[0], v) for v in (-1.0 / 6.0, 1.0 / 6.0, 1.0 / 12.0, 1.0 / 24.0))
    return [u[0] * _k(u[0], 0.25) + (s12 * m6 + s34 * p24), (u[2] - u[1]) * p6 + (u[3] - u[4]) * p12, (s12 * m6 + s34 * p6) + u[5]]


def _half(x):
    return x * _k(x, 0.5)


def g4(w):
    return [w[0], _half((w[0] + w[1]) + w[2]), _half((w[0] - w[1]) + w[2]), w[2]]


def bt4(d):
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def at4(m):
    return [(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]]


def a4(d):
    return [d[0], d[0] + d[1], d[0] - d[1], _k(d[0], 0) - d[1]]


def gt4(u):
    hs, hd = _half(u[1] + u[2]), _half(u[1] - u[2])
    return [u[0] + hs, hd, hs + u[3]]


ONE_D = {4: dict(filter=g6, input=bt6, output=at6, dy=a6, filter_grad=gt6), 2: dict(filter=g4, input=bt4, output=at4, dy=a4, filter_grad=gt4)}


def transform(kind, form, X, arith="f64", mut=None):
    """out[i][j][...] = sum_ab L[i][a] L[j][b] X[a][b][...] of stage `kind`.  arith: "f64" (the reference: float64 matrix products),
    "kernel" (the kernels' association, rows first, in X's own type) or "matmul" (plain products with the matrices rounded to X's type)."""
    L = matrices(form, mut)[kind]
    if arith == "f64":
        return np.einsum("ia,jb,ab...->ij...", L, L, X.astype(np.float64))
    if arith == "matmul":
        Lf = L.astype(X.dtype)
        t = np.zeros((L.shape[0],) + X.shape[1:], X.dtype)
        for i in range(L.shape[0]):
            for a in range(L.shape[1]):
                if Lf[i, a] != 0:
                    t[i] = t[i] + Lf[i, a] * X[a]
        out = np.zeros((L.shape[0], L.shape[0]) + X.shape[2:], X.dtype)
        for j in range(L.shape[0]):
            for b in range(L.shape[1]):
                if Lf[j, b] != 0:
                    out[:, j] = out[:, j] + Lf[j, b] * t[:, b]
        return out
    fn = ONE_D[form][kind]
    t = np.stack(fn([X[a] for a in range(X.shape[0])]))                       # along the rows, for every column
    return np.stack(fn([t[:, b] for b in range(t.shape[1])]), axis=1)         # then along the columns


def absbound(kind, form, X):
    """|L| |X| |L|^T: what the bound multiplies."""
    L = np.abs(matrices(form)[kind])
    return np.einsum("ia,jb,ab...->ij...", L, L, np.abs(X.astype(np.float64)))


# ---------------------------------------------------------------------------------------------------------------- gather / scatter
def tile_list(nb, h, w, form, swap=False):
    """[(img, ti, tj)] in list order; `swap` (mutant 4): a kernel that takes the row index for the column index."""
    th, tw = -(-h // form), -(-w // form)
    out = [(img, ti, tj) for img in range(nb) for ti in range(th) for tj in range(tw)]
    return [(img, tj, ti) for img, ti, tj in out] if swap else out


def patches(x, form, mode="zero", swap=False):
    """[a][a][tiles][c] of x [nb][h][w][c] in x's type.  mode: "zero" (the operation), "replicate" (mutant 1: border taps clamped to the
    image) or "no_image_pad" (mutant 2: the batch read as one tall image, rows above / below an image are its neighbour's)."""
    nb, h, w, c = x.shape
    a = form + 2
    tl = tile_list(nb, h, w, form, swap)
    d = np.zeros((a, a, len(tl), c), x.dtype)
    tall = x.reshape(nb * h, w, c)
    for t, (img, ti, tj) in enumerate(tl):
        for i in range(a):
            for j in range(a):
                ih, iw = form * ti - 1 + i, form * tj - 1 + j
                if mode == "replicate":
                    ih, iw = min(max(ih, 0), h - 1), min(max(iw, 0), w - 1)
                if mode == "no_image_pad":
                    ok = 0 <= img * h + ih < nb * h and 0 <= iw < w
                else:
                    ok = 0 <= ih < h and 0 <= iw < w
                if ok:
                    d[i, j, t] = tall[img * h + ih, iw]
    return d


def read_rows(buf, rows, n, ld, ld_used=None):
    """[rows][n] of a buffer laid out with pitch ld, as a reader that believes the pitch is ld_used sees it (mutant 7)."""
    ld_used = ld if ld_used is None else ld_used
    flat = np.concatenate([np.asarray(buf, np.float32).ravel(), np.full(rows * max(ld, ld_used), np.nan, np.float32)])
    return flat[:rows * ld_used].reshape(rows, ld_used)[:, :n]


def dy_blocks(g, nb, oh, ow, form, swap=False):
    """[m][m][tiles][n] of g [nb*oh*ow][n]: the block of each tile, zero past oh / ow."""
    tl = tile_list(nb, oh, ow, form, swap)
    d = np.zeros((form, form, len(tl), g.shape[1]), g.dtype)
    for t, (img, ti, tj) in enumerate(tl):
        for i in range(form):
            for j in range(form):
                y, x = form * ti + i, form * tj + j
                if y < oh and x < ow:
                    d[i, j, t] = g[(img * oh + y) * ow + x]
    return d


def scatter(o, nb, oh, ow, form, ld, n, ld_used=None, swap=False, overrun=False):
    """The [(rows + 1)][ld] buffer (NaN = untouched) after the m x m outputs o [m][m][tiles][n] were stored, in tile order.  ld_used:
    the pitch the writer believes (mutant 6); overrun (mutant 3): no test against oh / ow, the pixel index simply runs on."""
    ld_used = ld if ld_used is None else ld_used
    rows = nb * oh * ow
    flat = np.full((rows + 1) * ld, np.nan)
    for t, (img, ti, tj) in enumerate(tile_list(nb, oh, ow, form, swap)):
        for i in range(form):
            for j in range(form):
                y, x = form * ti + i, form * tj + j
                if not overrun and (y >= oh or x >= ow):
                    continue
                at = ((img * oh + y) * ow + x) * ld_used
                if 0 <= at and at + n <= flat.size:
                    flat[at:at + n] = o[i, j, t]
    return flat.reshape(rows + 1, ld)


# ---------------------------------------------------------------------------------------------------------------- stages
MUTANTS = ("replicate", "no_image_pad", "overrun", "swap_titj", "transpose_p", "dense_ldy", "dense_ld_dy", "no_gscale", "gscale_next_quad",
           "bt_5_to_4", "g_24_to_12", "shift_dropped_without_scale", "accumulate_drops_old", "relu_without_act")


def _dense(out, bound, s):
    """Full buffer, inside mask and tol of a dense output followed by TAIL floats."""
    tail = np.full(TAIL, np.nan)
    return dict(buf=np.concatenate([out.ravel(), tail]), inside=np.concatenate([np.ones(out.size, bool), np.zeros(TAIL, bool)]),
                tol=np.concatenate([s * U * bound.ravel(), np.zeros(TAIL)]), shape=out.shape)


def _positions(t, mut):
    """[a][a][...] -> [P][...], p = a * xi + nu -- or transposed (mutant 5)."""
    if mut == "transpose_p":
        t = np.swapaxes(t, 0, 1)
    return t.reshape((-1,) + t.shape[2:])


def stage_filter(w, c, n, ldw, form, arith="f64", mut=None):
    """w: the [9c][ldw] buffer.  -> u [P][c][n]."""
    g = read_rows(w, 9 * c, n, ldw).reshape(3, 3, c, n)
    if arith == "f64":
        g = g.astype(np.float64)
    return _dense(_positions(transform("filter", form, g, arith, mut), mut), _positions(absbound("filter", form, g), mut), S[form]["filter"])


def stage_input(x, form, arith="f64", mut=None):
    """x [nb][h][w][c] -> v [P][tiles][c]."""
    mode = mut if mut in ("replicate", "no_image_pad") else "zero"
    d = patches(x if arith != "f64" else x.astype(np.float64), form, mode, mut == "swap_titj")
    return _dense(_positions(transform("input", form, d, arith, mut), mut), _positions(absbound("input", form, patches(x, form)), mut), S[form]["input"])


def stage_output(m, nb, oh, ow, n, ldy, form, scale=None, shift=None, act=0, arith="f64", mut=None):
    """m [P][tiles][n] -> the [(rows + 1)][ldy] buffer of y."""
    a = form + 2
    mm = np.asarray(m).reshape(a, a, -1, n)
    if mut == "transpose_p":
        mm = np.swapaxes(mm, 0, 1)
    if arith == "f64":
        mm = mm.astype(np.float64)
    o = transform("output", form, mm, arith)
    ty = mm.dtype.type
    if scale is not None:
        o = o * scale.astype(ty)
    if shift is not None and not (mut == "shift_dropped_without_scale" and scale is None):
        o = o + shift.astype(ty)
    if act == 1 or mut == "relu_without_act":
        o = np.maximum(o, 0)
    bound = absbound("output", form, np.asarray(m).reshape(a, a, -1, n)) * (np.abs(scale.astype(np.float64)) if scale is not None else 1.0)
    tol = S[form]["output"] * U * bound + 2 * U * (np.abs(shift.astype(np.float64)) if shift is not None else 0.0)
    buf = scatter(o, nb, oh, ow, form, ldy, n, n if mut == "dense_ldy" else None, mut == "swap_titj", mut == "overrun")
    tolbuf = np.nan_to_num(scatter(tol, nb, oh, ow, form, ldy, n), nan=0.0)
    inside = np.zeros(buf.shape, bool)
    inside[:-1, :n] = True
    return dict(buf=buf.ravel(), inside=inside.ravel(), tol=tolbuf.ravel(), shape=buf.shape)


def stage_dy(dy, nb, oh, ow, n, ld_dy, form, gscale=None, arith="f64", mut=None):
    """dy: the [rows][ld_dy] buffer -> dz [P][tiles][n]; g = fl32(dy * gscale) in every arithmetic."""
    rows = nb * oh * ow

    def blocks(m_):
        g = read_rows(dy, rows, n, ld_dy, n if m_ == "dense_ld_dy" else None)
        if gscale is not None and m_ != "no_gscale":
            g = g * (np.roll(gscale, -4) if m_ == "gscale_next_quad" else gscale)[None, :]          # ONE fp32 multiply
        return dy_blocks(g, nb, oh, ow, form, m_ == "swap_titj")
    d = blocks(mut)
    if arith == "f64":
        d = d.astype(np.float64)
    s = S[form]["dy"] + (1 if gscale is not None else 0)          # the multiply by gscale: see the count above
    return _dense(_positions(transform("dy", form, d, arith), mut), _positions(absbound("dy", form, blocks(None)), mut), s)


def stage_filter_grad(du, c, n, ldw, form, old=None, arith="f64", mut=None):
    """du [P][c][n] -> the [(9c + 1)][ldw] buffer of dw; old: the dense [9c][n] values it is added to (accumulate = 1)."""
    a = form + 2
    uu = np.asarray(du).reshape(a, a, c, n)
    if mut == "transpose_p":
        uu = np.swapaxes(uu, 0, 1)
    if arith == "f64":
        uu = uu.astype(np.float64)
    o = transform("filter_grad", form, uu, arith, mut).reshape(9 * c, n)
    tol = S[form]["filter_grad"] * U * absbound("filter_grad", form, np.asarray(du).reshape(a, a, c, n)).reshape(9 * c, n)
    if old is not None:
        if mut != "accumulate_drops_old":
            o = old.astype(uu.dtype) + o
        tol = tol + 2 * U * np.abs(old.astype(np.float64))
    buf = np.full((9 * c + 1, ldw), np.nan)
    buf[:-1, :n] = o
    tolbuf = np.zeros(buf.shape)
    tolbuf[:-1, :n] = tol
    return dict(buf=buf.ravel(), inside=~np.isnan(buf).ravel(), tol=tolbuf.ravel(), shape=buf.shape)


def ref_gemm(v, u):
    """m[p] = v[p] @ u[p] in float64 with the project's bound, K_red = c."""
    v64, u64 = np.asarray(v, np.float64), np.asarray(u, np.float64)
    return _dense(np.einsum("ptc,pcn->ptn", v64, u64), np.einsum("ptc,pcn->ptn", np.abs(v64), np.abs(u64)), v64.shape[2] + 8)


def ref_wgrad(v, dz, old=None, mut=None):
    """du[p] (+)= v[p]^T @ dz[p] in float64, K_red = tiles; the old value takes the addend's place (accumulate = 1)."""
    v64, z64 = np.asarray(v, np.float64), np.asarray(dz, np.float64)
    out, absdot = np.einsum("ptc,ptn->pcn", v64, z64), np.einsum("ptc,ptn->pcn", np.abs(v64), np.abs(z64))
    if old is not None:
        absdot = absdot + np.abs(np.asarray(old, np.float64))
        if mut != "accumulate_drops_old":
            out = out + np.asarray(old, np.float64)
    return _dense(out, absdot, v64.shape[1] + 8)


# ---------------------------------------------------------------------------------------------------------------- per case
def variants(stage):
    """The variants every case runs of a stage: the eight epilogues, gscale or none, accumulate 0 / 1."""
    return {"output": EPILOGUES, "dy": [True, False], "filter_grad": [0, 1]}.get(stage, [None])


def applies(mut, cs, form, stage, var=None):
    """Whether a mutant changes the stage's result for this case; the CPU test also shows that the others change NOTHING."""
    th, tw = geometry(cs, form)["th"], geometry(cs, form)["tw"]
    one_pixel = cs.h == 1 and cs.w == 1              # one live element on the diagonal: patch, block and output are symmetric under transposition
    partial = cs.h % form != 0 or cs.w % form != 0
    return {
        "replicate": stage == "input",
        "no_image_pad": stage == "input" and cs.nb > 1,
        "overrun": stage == "output" and partial,
        "swap_titj": stage in ("input", "output", "dy") and max(th, tw) > 1,
        "transpose_p": stage in ("filter", "filter_grad") or (stage in ("input", "output", "dy") and not one_pixel),
        "dense_ldy": stage == "output" and cs.nb * cs.h * cs.w > 1,
        "dense_ld_dy": stage == "dy" and cs.nb * cs.h * cs.w > 1,
        "no_gscale": stage == "dy" and var is True,
        "gscale_next_quad": stage == "dy" and var is True and cs.n > 4,
        "bt_5_to_4": stage == "input" and form == 4 and not one_pixel,          # the coefficient multiplies image row / column 1 of tile 0
        "g_24_to_12": stage in ("filter", "filter_grad") and form == 4,
        "shift_dropped_without_scale": stage == "output" and var is not None and not var[0] and var[1],
        "accumulate_drops_old": stage == "filter_grad" and var == 1,
        "relu_without_act": stage == "output" and var is not None and var[2] == 0 and _has_negative(cs.name, form, var),
    }[mut]


def _has_negative(name, form, var):
    """A ReLU that should not be there shows only where an output is negative (the four outputs of a one-pixel map may all be positive)."""
    r = compute(name, form, "output", var)
    return bool((r["buf"][r["inside"]] < 0).any())


def _run(name, form, stage, var, ints, arith, mut):
    cs, d, p = CASES[name], inputs(name, form, ints), pitches(CASES[name])
    if stage == "filter":
        return stage_filter(padded(d["w"], p["ldw"]), cs.c, cs.n, p["ldw"], form, arith, mut)
    if stage == "input":
        return stage_input(d["x"], form, arith, mut)
    if stage == "output":
        return stage_output(d["m"], cs.nb, cs.h, cs.w, cs.n, p["ldy"], form, d["scale"] if var[0] else None, d["shift"] if var[1] else None,
                            var[2], arith, mut)
    if stage == "dy":
        return stage_dy(padded(d["dy"], p["ld_dy"]), cs.nb, cs.h, cs.w, cs.n, p["ld_dy"], form, d["gscale"] if var else None, arith, mut)
    return stage_filter_grad(d["du"], cs.c, cs.n, p["ldw"], form, d["dw0"] if var else None, arith, mut)


@functools.lru_cache(maxsize=None)
def compute(name, form, stage, var=None, ints=False):
    """dict(buf, inside, tol, shape) of a stage of a case on its own inputs: float64, computed once, read-only."""
    res = _run(name, form, stage, var, ints, "f64", None)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def emulate(name, form, stage, var=None, ints=False, arith="kernel"):
    """The same stage in fp32: the kernels' association ("kernel") or plain matrix products ("matmul"), without FMA."""
    return _run(name, form, stage, var, ints, arith, None)


def mutant(name, form, stage, var, mut):
    assert mut in MUTANTS
    return _run(name, form, stage, var, False, "f64", mut)
