"""Shared case table and NumPy references of the fp32 implicit-GEMM conv edge tests (device-free check of the table, the references
and their teeth: tests/test_fp32_edge_cases_reference.py; the kernels: tests/test_gpu_fp32_edges.py).  No torch, no library.

The operations are stated as include/radnet_hip.h states them, with g = dy * gscale as ONE fp32 multiply before the sum:

  fwd    y[m][j]  = act( (sum_k im2col(x)[m][k] * w[k][j]) * scale[j] + shift[j] + addend[m][j] )
  dgrad  dx[p][c] = mask[p][c] > 0 ? (sum_{ky,kx,j<n} g[q(p,ky,kx)][j] * w[(ky,kx,c)][j]) + dx_add[p][c] : 0            (stride 1)
  wgrad  dw[k][j] (+)= sum_m im2col(x)[m][k] * g[m][j];   db[j] (+)= sum_m g[m][j]

`compute(name, side, mode)` gives the FULL output of a case (every row and column) in float64, sum |a*b| per element and the
per-element bound.  The bound is derived, not tuned: an fp32 sum of K products in any order, with or without FMA contraction, lies
within gamma_K * sum|a_k b_k| of the exact sum, gamma_K = K u / (1 - K u), u = 2^-24; a split of the reduction (ordered slabs or
atomics) only changes the order.  So

  tol = (K_red + 8) * 2^-24 * (absdot * |scale| + |shift| + |addend|)

with K_red = kh*kw*c (fwd), kh*kw*n (dgrad), M (wgrad and db); the + 8 covers the gscale multiply and the epilogue's multiplies and
adds; dx_add (dgrad) / the old dw (wgrad mode 1) take the addend's place.  Sigmoid columns (act = 2) get the pre-activation bound
times 1/4 (the largest slope) plus SIGMOID_SLACK.

Pitches are wider than the rows everywhere, pairwise different on the output side and multiples of 4 (two cases: NOT multiples of 4,
see ODD_PITCH); input-side padding holds NaN, every output element starts as SENTINEL.  `compute` reads and writes its operands
through those pitches, so that the mutants of the CPU test ("the addend read with the output's pitch") are the same code with one
parameter changed."""
import collections
import functools

import numpy as np

from bf16_edge_cases import SENTINEL, col2im_gather, im2col, padded  # noqa: F401  (SENTINEL, padded: re-exported to the tests)

U = 2.0 ** -24
# Absolute slack of a sigmoid column: a few ulp of expf and one division at values <= 1.  Measured on one MI355X over the sigmoid
# columns of these cases (f_s2_pad_br, every launch shape): worst |gpu - float64 reference| = 4.3e-07 = 1.8 * 2^-22 INCLUDING the
# pre-activation error times its slope, worst err / tol 0.012 -- the device's sigmoid is inside the derived figure, which stands.
SIGMOID_SLACK = 2.0 ** -22

Case = collections.namedtuple("Case", "name kind nb h w c kh kw stride pad n splits expect opts")
# pad = (top, left, bottom, right), bottom / right being what oh / ow imply; splits = forced reduction splits beyond {1, -1};
# expect = what the comment claims (M, P, nrt = reduction tiles of 32), checked on the CPU


def _case(name, kind, shape, kw=None, pad=None, splits=(), expect=None, **opts):
    nb, h, w, c, kh, stride, p, n = shape
    return Case(name, kind, nb, h, w, c, kh, kh if kw is None else kw, stride, (p, p, p, p) if pad is None else pad, n, tuple(splits),
                expect or {}, opts)


_ALL = dict(gscale=True, dx_add=True, dx_mask=True)
# opts: fwd act (0 none, 1 relu, 2 sigmoid on act_cols) / col_block ; dgrad gscale / dx_add / dx_mask ; wgrad gscale / modes / db ; pitch overrides
_TABLE = [
    # ---- forward (c % 32 == 0 or c == 4, n % 4 == 0, kh * kw <= 32 unless c == 4)
    _case("f_ragged_mn", "fwd", (1, 9, 15, 32, 1, 1, 0, 68), act=1, expect=dict(M=135, nrt=1)),      # M = 2*64 + 7, N = 64 + 4, one K tile
    _case("f_m1_n4", "fwd", (1, 1, 1, 32, 1, 1, 0, 4), act=0, expect=dict(M=1, nrt=1)),
    _case("f_same_3x3_two_images", "fwd", (2, 9, 11, 32, 3, 1, 1, 36), act=1, expect=dict(M=198, nrt=9)),   # image boundary (row 99) inside tile 1
    _case("f_valid_3x3", "fwd", (2, 7, 8, 32, 3, 1, 0, 36), act=0, expect=dict(M=60)),               # no padding at all
    _case("f_s2_pad_br", "fwd", (2, 13, 11, 32, 3, 2, 0, 100), pad=(0, 0, 2, 2), act=2, act_cols=20, expect=dict(oh=7, ow=6)),
    _case("f_pad_t_ne_l", "fwd", (2, 8, 9, 32, 3, 1, 0, 36), pad=(1, 0, 1, 0), act=1, expect=dict(oh=8, ow=7)),
    _case("f_1x3", "fwd", (2, 5, 9, 32, 1, 1, 0, 40), kw=3, pad=(0, 1, 0, 1), act=1),
    _case("f_3x1", "fwd", (2, 9, 5, 32, 3, 1, 0, 40), kw=1, pad=(1, 0, 1, 0), act=0),
    _case("f_5x5", "fwd", (1, 7, 6, 32, 5, 1, 2, 8), act=1, expect=dict(nrt=25)),                    # 25 taps of the 32-bit row mask
    _case("f_deep_k", "fwd", (1, 6, 7, 1056, 1, 1, 0, 100), act=1, splits=(2, 3, 33), expect=dict(M=42, nrt=33)),
    _case("f_stem", "fwd", (2, 11, 13, 4, 7, 2, 3, 68), act=1, expect=dict(M=84, nrt=7)),            # c == 4 path, channel 3 NON-zero, K = 196
    _case("f_col_block", "fwd", (1, 9, 15, 32, 1, 1, 0, 32), act=0, col_block=True, expect=dict(M=135)),   # y = right half of a [135][64] tensor
    _case("f_odd_pitch", "fwd", (2, 9, 11, 32, 3, 1, 1, 36), act=1, pitch=dict(ldy=39, ld_add=41)),  # pitches that are no multiple of 4
    # ---- data gradient (stride 1, n % 32 == 0, c % 4 == 0, dense dy)
    _case("d_ragged", "dgrad", (1, 9, 15, 68, 1, 1, 0, 32), expect=dict(P=135, nrt=1), **_ALL),      # c = 64 + 4
    _case("d_same_3x3_all", "dgrad", (2, 9, 11, 36, 3, 1, 1, 32), expect=dict(nrt=9), **_ALL),
    _case("d_same_3x3_bare", "dgrad", (2, 9, 11, 36, 3, 1, 1, 32), gscale=False, dx_add=False, dx_mask=False),
    _case("d_same_3x3_add_only", "dgrad", (2, 9, 11, 36, 3, 1, 1, 32), gscale=True, dx_add=True, dx_mask=False),
    _case("d_same_3x3_mask_only", "dgrad", (2, 9, 11, 36, 3, 1, 1, 32), gscale=False, dx_add=False, dx_mask=True),
    _case("d_valid_3x3", "dgrad", (2, 7, 8, 8, 3, 1, 0, 32), **_ALL),                                # the gather runs with padding k - 1 - pad = 2
    _case("d_pad_t_ne_l", "dgrad", (2, 8, 9, 36, 3, 1, 0, 32), pad=(1, 0, 1, 0), **_ALL),
    _case("d_1x3", "dgrad", (2, 5, 9, 36, 1, 1, 0, 32), kw=3, pad=(0, 1, 0, 1), **_ALL),
    _case("d_3x1", "dgrad", (2, 9, 5, 36, 3, 1, 0, 32), kw=1, pad=(1, 0, 1, 0), gscale=False, dx_add=False, dx_mask=True),
    _case("d_deep", "dgrad", (2, 6, 7, 100, 3, 1, 1, 352), splits=(2, 3, 99), expect=dict(nrt=99), **_ALL),
    _case("d_odd_pitch", "dgrad", (2, 9, 11, 36, 3, 1, 1, 32), pitch=dict(ld_dx=39, ld_dx_add=41, ld_dx_mask=43), **_ALL),
    # ---- weight gradient (c % 64 == 0, n % 4 == 0, ld_dy % 4 == 0).  The issue's table has c = 64 everywhere, at which the forced k
    # tile of 128 is refused (c % bmk != 0) and the 128-row templates would never run: w_s2_1x1 and w_1x3 have c = 128 instead.
    _case("w_ragged_db", "wgrad", (1, 9, 15, 64, 1, 1, 0, 68), gscale=True, modes=(0, 1, 2), db=True, expect=dict(M=135, nrt=5)),   # 4 tiles + 7 rows
    _case("w_m1", "wgrad", (1, 1, 1, 64, 1, 1, 0, 4), gscale=False, modes=(0, 1), db=True, expect=dict(M=1, nrt=1)),
    _case("w_s2_3x3", "wgrad", (2, 13, 11, 64, 3, 2, 1, 36), gscale=True, modes=(0,), expect=dict(M=84)),
    _case("w_s2_1x1", "wgrad", (3, 14, 14, 128, 1, 2, 0, 72), gscale=True, modes=(2,), db=True, expect=dict(M=147)),
    _case("w_pad_br", "wgrad", (2, 13, 11, 64, 3, 2, 0, 40), pad=(0, 0, 2, 2), gscale=True, modes=(0,)),
    _case("w_1x3", "wgrad", (2, 5, 9, 128, 1, 1, 0, 40), kw=3, pad=(0, 1, 0, 1), gscale=True, modes=(1,)),
    _case("w_3x1_s2", "wgrad", (2, 9, 5, 64, 3, 2, 0, 40), kw=1, pad=(1, 0, 1, 0), gscale=False, modes=(0,), db=True),
    _case("w_deep_m", "wgrad", (1, 31, 35, 64, 1, 1, 0, 8), gscale=True, modes=(0, 1, 2), db=True, splits=(2, 3, 8),
          expect=dict(M=1085, nrt=34)),                                                              # 33 * 32 + 29 rows
    # ---- both gradients from one descriptor (radnet_conv_bwd against the two calls): wgrad's and dgrad's constraints together
    _case("b_3x3", "bwd", (2, 9, 11, 64, 3, 1, 1, 32), splits=(2, 3), modes=(0, 1, 2), db=True, **_ALL),
    _case("b_1x1", "bwd", (2, 9, 11, 64, 1, 1, 0, 64), splits=(2,), modes=(0, 1, 2), db=True, **_ALL),
]
CASES = collections.OrderedDict((c.name, c) for c in _TABLE)
assert len(CASES) == len(_TABLE)
ODD_PITCH = ("f_odd_pitch", "d_odd_pitch")
# The epilogue of the forward / data-gradient kernel (csrc/conv_igemm_body.h) reads the addend and the mask and writes the output
# with 4-byte buffer instructions only, one element each, at (row * pitch + column) * 4: any pitch >= n is addressed correctly and no
# access is wider than its element.  Their 16-byte accesses go to x / dy (dense), w (ldw % 4 == 0, checked) and the slabs.  The
# weight-gradient kernel reads dy 16 bytes at a time and its launcher already refuses ld_dy % 4 != 0 and ldw % 4 != 0.


def sides(cs):
    """The operations a case runs: its kind, or (wgrad, dgrad) for a conv_bwd case -- the order of the two calls."""
    return ("wgrad", "dgrad") if cs.kind == "bwd" else (cs.kind,)


# ---------------------------------------------------------------------------------------------------------------- geometry
def geometry(cs, side=None):
    """oh, ow, M (output pixels), P (input pixels), K (kh*kw*c), rows x cols of `side`'s output, its reduction length and tiles."""
    side = side or sides(cs)[0]
    pt, pl, pb, pr = cs.pad
    oh, ow = (cs.h + pt + pb - cs.kh) // cs.stride + 1, (cs.w + pl + pr - cs.kw) // cs.stride + 1
    M, P, K = cs.nb * oh * ow, cs.nb * cs.h * cs.w, cs.kh * cs.kw * cs.c
    if side == "fwd":
        rows, cols, kred = M, cs.n, K
    elif side == "dgrad":
        rows, cols, kred = P, cs.c, cs.kh * cs.kw * cs.n
    else:
        rows, cols, kred = K, cs.n, M
    return dict(oh=oh, ow=ow, M=M, P=P, K=K, rows=rows, cols=cols, kred=kred, nrt=(kred + 31) // 32)


def pitches(cs):
    """Row pitches in floats: every one wider than its row, the output-side ones pairwise different."""
    p = dict(ldw=cs.n + 4, ldy=cs.n + 8, ld_add=cs.n + 12, ld_dx=cs.c + 4, ld_dx_add=cs.c + 8, ld_dx_mask=cs.c + 12,
             ld_dy=cs.n if "dgrad" in sides(cs) else cs.n + 8)          # radnet_conv_dgrad takes dense dy only
    if cs.opts.get("col_block"):
        p["ldy"] = 2 * cs.n
    p.update(cs.opts.get("pitch", {}))
    return p


def igemm_shapes(cs, side):
    """(launch shapes [(bm, bn, slices, waves)] a forward / dgrad case must run, the number left out by a documented rule).
    Tiles 64x64, 128x128, 128x64, 64x128 with 4 and 8 waves; 32x64 and 32x32 with 4 waves only and not for the 4-channel stem
    (run_igemm: 32-row tiles are 4-wave, channel-tiled).  Slices {1, -1} and the case's named splits with both signs; |s| <= nk."""
    nk = geometry(cs, side)["nrt"]
    out, left = [], 0
    for s in [1, -1] + [v * sg for v in cs.splits for sg in (1, -1)]:
        for bm, bn in [(64, 64), (128, 128), (128, 64), (64, 128), (32, 64), (32, 32)]:
            for wv in (4, 8):
                if bm == 32 and wv == 8:
                    continue                                   # not a shape: the issue lists the 32-row tiles with 4 waves
                if (bm == 32 and cs.c == 4 and side == "fwd") or abs(s) > nk:
                    left += 1
                    continue
                out.append((bm, bn, s, wv))
    return out, left


def wgrad_shapes(cs):
    """[(bmk, bn, splits)]: tiles {64, 128}^2 with c % bmk == 0, splits {1, 2, 3, 8} with at least one 32-row tile per split."""
    nmt = geometry(cs, "wgrad")["nrt"]
    out, left = [], 0
    for s in (1, 2, 3, 8):
        for bmk in (64, 128):
            for bn in (64, 128):
                if cs.c % bmk or (s > 1 and nmt // s < 1):
                    left += 1
                    continue
                out.append((bmk, bn, s))
    return out, left


# ---------------------------------------------------------------------------------------------------------------- numbers
@functools.lru_cache(maxsize=None)
def inputs(name):
    """Dense fp32 inputs of a case from its seed (its position in the table): plain normals, weights scaled by 1 / sqrt(K)."""
    cs = CASES[name]
    g = geometry(cs)
    rs = np.random.RandomState(4000 + list(CASES).index(name))
    f = lambda *shape: rs.standard_normal(shape).astype(np.float32)
    d = dict(w=(rs.standard_normal((g["K"], cs.n)) / np.sqrt(g["K"])).astype(np.float32))
    if cs.kind != "dgrad":
        d["x"] = f(cs.nb, cs.h, cs.w, cs.c)
    if cs.kind == "fwd":
        d["scale"] = rs.uniform(0.5, 1.5, cs.n).astype(np.float32)
        d["shift"], d["addend"] = f(cs.n), f(g["M"], cs.n)
    else:
        d["dy"] = f(g["M"], cs.n)
        d["gscale"] = rs.uniform(0.5, 1.5, cs.n).astype(np.float32) if cs.opts.get("gscale") else None
    if "dgrad" in sides(cs):
        d["dx_add"] = f(g["P"], cs.c) if cs.opts.get("dx_add") else None
        d["dx_mask"] = f(g["P"], cs.c) if cs.opts.get("dx_mask") else None
    if "wgrad" in sides(cs):
        d["dw0"], d["db0"] = f(g["K"], cs.n), f(cs.n)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def _view(dense, ld, ld_used):
    """What a reader that believes the pitch is `ld_used` sees of a [rows][cols] matrix stored with pitch `ld` (NaN padding)."""
    rows, cols = dense.shape
    if ld_used == ld:
        return dense.astype(np.float64)
    flat = padded(dense, ld).ravel()
    flat = np.concatenate([flat, np.full(max(0, rows * ld_used - flat.size), np.nan, np.float32)])
    return flat[:rows * ld_used].reshape(rows, ld_used)[:, :cols].astype(np.float64)


def _stored(out, ld, ld_used):
    """What lies in [rows) x [cols) of a buffer of pitch `ld` after a writer that believes the pitch is `ld_used` stored `out`."""
    rows, cols = out.shape
    if ld_used == ld:
        return out
    flat = np.full(rows * max(ld, ld_used) + cols, np.nan)
    for r in range(rows):
        flat[r * ld_used:r * ld_used + cols] = out[r]
    return flat[:rows * ld].reshape(rows, ld)[:, :cols]


def gather(src, nb, H, W, OH, OW, kh, kw, stride, pt, pl, wrap=False):
    """[nb*OH*OW][kh][kw][C] float64 of src [nb][H][W][C]: zeros for taps outside the image -- or, with `wrap` (a mutant), what a
    gather that only tests the top / left edge and the end of the tensor reads: the next row's / image's pixels."""
    C_ = src.shape[-1]
    flat = src.reshape(nb * H * W, C_).astype(np.float64)
    m = np.arange(nb * OH * OW)
    img, r = m // (OH * OW), m % (OH * OW)
    oy, ox = r // OW, r % OW
    A = np.zeros((m.size, kh, kw, C_), np.float64)
    for ky in range(kh):
        for kx in range(kw):
            iy, ix = oy * stride - pt + ky, ox * stride - pl + kx
            lin = (img * H + iy) * W + ix
            ok = (iy >= 0) & (ix >= 0) & (lin < nb * H * W) if wrap else (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            A[ok, ky, kx, :] = flat[lin[ok]]
    return A


MUTANTS = ("dense_ldw", "dense_ldy", "dense_ld_add", "dense_ld_dx", "dense_ld_dx_add", "dense_ld_dx_mask", "dense_ld_dy", "dense_ld_dw",
           "swap_ldy_ld_add", "swap_pad", "swap_khkw", "wrap_taps", "drop_last_tap", "drop_last_k_tile", "stem_ch3_zero", "no_gscale",
           "mask_before_add", "mode1_as_mode0", "db_without_gscale", "skip_last_row")


def applies(mut, cs, side, mode=0):
    """Whether a mutant changes anything for this case (the CPU test lists the ones that do not)."""
    pt, pl, pb, pr = cs.pad
    g = geometry(cs, side)
    o = cs.opts
    falls_off = (g["oh"] - 1) * cs.stride - pt + cs.kh - 1 >= cs.h or (g["ow"] - 1) * cs.stride - pl + cs.kw - 1 >= cs.w
    if side == "dgrad":          # the gather runs over dy with padding k - 1 - pad: taps fall off its bottom / right edge when that is > 0... on the far side
        falls_off = (cs.h - 1) + pt >= g["oh"] or (cs.w - 1) + pl >= g["ow"]
    many = g["rows"] > 1                 # a pitch has no effect on a one-row matrix (f_m1_n4; w_m1's dy)
    return {
        "dense_ldw": side != "wgrad", "dense_ldy": side == "fwd" and many, "dense_ld_add": side == "fwd" and many,
        "dense_ld_dx": side == "dgrad", "dense_ld_dx_add": side == "dgrad" and bool(o.get("dx_add")),
        "dense_ld_dx_mask": side == "dgrad" and bool(o.get("dx_mask")),
        "dense_ld_dy": side == "wgrad" and cs.kind == "wgrad" and g["M"] > 1,          # a conv_bwd case has dense dy: nothing to misread
        "dense_ld_dw": side == "wgrad",
        "swap_ldy_ld_add": (side == "fwd" and many) or (side == "dgrad" and bool(o.get("dx_add"))),
        "swap_pad": pt != pl, "swap_khkw": cs.kh != cs.kw, "wrap_taps": falls_off,
        "drop_last_tap": cs.kh * cs.kw > 1, "drop_last_k_tile": True,
        "stem_ch3_zero": side == "fwd" and cs.c == 4,
        "no_gscale": side != "fwd" and bool(o.get("gscale")),
        "mask_before_add": side == "dgrad" and bool(o.get("dx_add")) and bool(o.get("dx_mask")),
        "mode1_as_mode0": side == "wgrad" and mode == 1,
        "db_without_gscale": side == "wgrad" and bool(o.get("db")) and bool(o.get("gscale")),
        "skip_last_row": g["rows" if side != "wgrad" else "M"] % 32 != 0,
    }[mut]


def _compute(name, side, mode, mut):
    cs, d, p = CASES[name], inputs(name), pitches(CASES[name])
    g = geometry(cs, side)
    kh, kw, (pt, pl) = cs.kh, cs.kw, cs.pad[:2]
    plain = mut is None
    if mut == "swap_pad":
        pt, pl = pl, pt
    if mut == "swap_khkw":
        kh, kw = kw, kh
    wrap = mut == "wrap_taps"
    taps, n, c = kh * kw, cs.n, cs.c
    dense = lambda key, cols: cols if mut == "dense_" + key else p[key]
    res = {}
    if side != "fwd":
        dy = _view(d["dy"], p["ld_dy"], dense("ld_dy", n)).astype(np.float32)
        gm = dy * d["gscale"][None, :] if d["gscale"] is not None and mut != "no_gscale" else dy          # ONE fp32 multiply
        gm = gm.astype(np.float64)
    if side in ("fwd", "wgrad"):
        x = np.array(d["x"])
        if mut == "stem_ch3_zero":
            x[..., 3] = 0
        A = im2col(x, cs) if plain else gather(x, cs.nb, cs.h, cs.w, g["oh"], g["ow"], kh, kw, cs.stride, pt, pl, wrap).reshape(g["M"], -1)
    if side == "fwd":
        Wm = _view(d["w"], p["ldw"], dense("ldw", n))
        if mut == "drop_last_tap":
            A[:, (taps - 1) * c:] = 0
        if mut == "drop_last_k_tile":
            A[:, (g["nrt"] - 1) * 32:] = 0
        dot, absdot = A @ Wm, np.abs(A) @ np.abs(Wm)
        ld_add_used, ldy_used = dense("ld_add", n), dense("ldy", n)
        if mut == "swap_ldy_ld_add":
            ld_add_used, ldy_used = p["ldy"], p["ld_add"]
        add = _view(d["addend"], p["ld_add"], ld_add_used)
        sc, sh = d["scale"].astype(np.float64)[None, :], d["shift"].astype(np.float64)[None, :]
        pre = dot * sc + sh + add
        tol = (g["kred"] + 8) * U * (absdot * np.abs(sc) + np.abs(sh) + np.abs(add))
        act, ac = cs.opts.get("act", 0), cs.opts.get("act_cols", 0)
        out = np.maximum(pre, 0) if act == 1 else pre.copy()
        if act == 2:
            out[:, :ac] = 1.0 / (1.0 + np.exp(-pre[:, :ac]))
            tol[:, :ac] = 0.25 * tol[:, :ac] + SIGMOID_SLACK
        if mut == "skip_last_row":
            out[-1] = 0
        res.update(out=_stored(out, p["ldy"], ldy_used), pre=pre)
    elif side == "dgrad":
        if plain:
            A = col2im_gather(gm, cs)
        else:      # the forward gather over dy [nb][oh][ow][n] with padding k - 1 - pad and the kernel flipped
            A = gather(gm.reshape(cs.nb, g["oh"], g["ow"], n), cs.nb, g["oh"], g["ow"], cs.h, cs.w, kh, kw, 1, kh - 1 - pt, kw - 1 - pl, wrap)
            A = A[:, ::-1, ::-1, :].reshape(g["P"], -1)
        Wm = _view(d["w"], p["ldw"], dense("ldw", n))
        B = Wm.reshape(taps, c, n).transpose(0, 2, 1).reshape(taps * n, c)                               # [(ky, kx, j)][c]
        A = np.array(A)
        if mut == "drop_last_tap":
            A[:, (taps - 1) * n:] = 0
        if mut == "drop_last_k_tile":
            A[:, (g["nrt"] - 1) * 32:] = 0
        dot, absdot = A @ B, np.abs(A) @ np.abs(B)
        ld_add_used, ld_dx_used = dense("ld_dx_add", c), dense("ld_dx", c)
        if mut == "swap_ldy_ld_add":
            ld_add_used, ld_dx_used = p["ld_dx"], p["ld_dx_add"]
        add = _view(d["dx_add"], p["ld_dx_add"], ld_add_used) if d["dx_add"] is not None else np.zeros_like(dot)
        keep = _view(d["dx_mask"], p["ld_dx_mask"], dense("ld_dx_mask", c)) > 0 if d["dx_mask"] is not None else np.ones(dot.shape, bool)
        out = np.where(keep, dot, 0.0) + add if mut == "mask_before_add" else np.where(keep, dot + add, 0.0)
        tol = (g["kred"] + 8) * U * (absdot + np.abs(add))
        if mut == "skip_last_row":
            out[-1] = 0
        res.update(out=_stored(out, p["ld_dx"], ld_dx_used))
    else:
        A, gm = np.array(A), np.array(gm)
        if mut == "drop_last_tap":
            A[:, (taps - 1) * c:] = 0
        if mut == "drop_last_k_tile":
            A[(g["nrt"] - 1) * 32:] = 0
            gm[(g["nrt"] - 1) * 32:] = 0
        if mut == "skip_last_row":
            A[-1] = 0
            gm[-1] = 0
        dot, absdot = A.T @ gm, np.abs(A).T @ np.abs(gm)
        old = d["dw0"].astype(np.float64) if mode == 1 else np.zeros_like(dot)          # mode 2 adds to the zeros the caller wrote
        out = dot + (0.0 if mut == "mode1_as_mode0" else old)
        tol = (g["kred"] + 8) * U * (absdot + np.abs(old))
        old_b = d["db0"].astype(np.float64) if mode == 1 else np.zeros(n)
        gb = _view(d["dy"], p["ld_dy"], dense("ld_dy", n)) if mut == "db_without_gscale" else gm
        res.update(out=_stored(out, p["ldw"], dense("ld_dw", n) if mut == "dense_ld_dw" else p["ldw"]),
                   db=gb.sum(0) + (0.0 if mut == "mode1_as_mode0" else old_b), db_tol=(g["kred"] + 8) * U * (np.abs(gm).sum(0) + np.abs(old_b)))
    res.update(absdot=absdot, tol=tol)
    return res


@functools.lru_cache(maxsize=None)
def compute(name, side=None, mode=0):
    """dict(out, absdot, tol [, pre, db, db_tol]) of the case's true result -- float64, every output element; computed once, read-only."""
    res = _compute(name, side or sides(CASES[name])[0], mode, None)
    for v in res.values():
        v.setflags(write=False)
    return res


def mutant(name, side, mode, mut):
    """The output (and db) a kernel with one defect would give: `compute` with one parameter changed."""
    assert mut in MUTANTS and applies(mut, CASES[name], side, mode)
    return _compute(name, side, mode, mut)
