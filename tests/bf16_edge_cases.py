"""Shared case table and NumPy references of the bf16 matrix-core conv edge tests (device-free check of the table and the references:
tests/test_bf16_edge_cases_reference.py; the kernels: tests/test_gpu_bf16_edges.py).  No torch, no library.

The three operations are stated as include/radnet_hip.h and the kernel headers (csrc/conv_bf16.hip, csrc/conv_bf16_bwd.hip) state them,
with bf16() = round to nearest, ties to even and g = dy * gscale as ONE fp32 multiply before rounding:

  fwd    y[m][j]  = act( (sum_k bf16(im2col(x))[m][k] * bf16(w)[k][j]) * scale[j] + shift[j] + addend[m][j] )
  dgrad  dx[p][c] = mask[p][c] > 0 ? (sum_{ky,kx,j<n} bf16(g)[q(p,ky,kx)][j] * bf16(w)[(ky,kx,c)][j]) + dx_add[p][c] : 0      (stride 1)
  wgrad  dw[k][j] (+)= sum_m bf16(im2col(x))[m][k] * bf16(g)[m][j];   db[j] (+)= sum_m g[m][j] (unrounded)

For every case `reference(name)` gives the FULL output (every row and column) in float64 over bf16-rounded operands (`ref`), the same
over the unrounded operands (`ref_u`), the raw sums before the epilogue (`dot`, `dot_u`), sum |a*b| per element (`absdot`) and the bound
of the existing bf16 kernel tests, 1e-5 * sum|a*b| (* scale) + 1e-6 * (1 + |tail|) (`tol`).  Rounded operands come from the `_biased`
recipe of tests/test_gpu_bf16_predict.py: half of them lie in (1 + 2^-9, 1 + 2^-8) and round DOWN, so a result computed from unrounded
operands falls outside the bound.

Pitches are wider than the rows everywhere (the C ABI takes any pitch at least as wide as the row); what lies in a pitch's padding
is NaN on the input side and a sentinel NaN on the output side."""
import collections
import functools

import numpy as np

SENTINEL = np.uint32(0x7FC5A5A5)          # a quiet NaN no kernel produces: the prefill of every output element, pitch padding included

Case = collections.namedtuple("Case", "name kind nb h w c kh kw stride pad n template tiles opts")
# pad = (top, left, bottom, right); template = (BM, BN) the case must land on; tiles = the tile count the issue lists (None: not listed)


def _case(name, kind, shape, template, tiles=None, kw=None, pad=None, **opts):
    nb, h, w, c, kh, stride, p, n = shape
    return Case(name, kind, nb, h, w, c, kh, kh if kw is None else kw, stride, (p, p, p, p) if pad is None else pad, n, template, tiles, opts)


# opts: fwd act (0 none, 1 relu, 2 sigmoid on act_cols) ; dgrad gscale / dx_add / dx_mask ; wgrad gscale / modes (dw_accumulate) / db
_TABLE = [
    # ---- forward
    _case("fwd_128x128_ragged", "fwd", (1, 127, 129, 72, 1, 1, 0, 136), (128, 128), 256, act=1),       # M = 128*128 - 1, N = 128 + 8, K padding in tile 3
    _case("fwd_128x64_ragged", "fwd", (1, 128, 129, 72, 1, 1, 0, 72), (128, 64), 258, act=0),          # N = 64 + 8
    _case("fwd_deep_k", "fwd", (1, 6, 7, 1032, 1, 1, 0, 100), (64, 64), 2, act=2, act_cols=20),        # M = 42 < one tile, 33 K tiles
    _case("fwd_s2_3x3_split", "fwd", (2, 13, 11, 24, 3, 2, 1, 100), (64, 64), act=1),                  # the existing ragged shape, now split
    _case("fwd_s2_3x3_pad_br", "fwd", (2, 13, 11, 24, 3, 2, 0, 100), (64, 64), pad=(0, 0, 2, 2), act=2, act_cols=20),   # oh = ceil(h / 2): bottom / right taps fall off
    _case("fwd_1x3", "fwd", (2, 5, 9, 16, 1, 1, 0, 40), (64, 64), kw=3, pad=(0, 1, 0, 1), act=1),
    _case("fwd_3x1", "fwd", (2, 9, 5, 16, 3, 1, 0, 40), (64, 64), kw=1, pad=(1, 0, 1, 0), act=0),
    # ---- data gradient
    _case("dgrad_128x128_ragged", "dgrad", (1, 45, 46, 2056, 1, 1, 0, 72), (128, 128), 289, gscale=True, dx_add=True, dx_mask=True),   # P = 2070, c = 2048 + 8
    _case("dgrad_128x64_ragged", "dgrad", (1, 33, 31, 2056, 1, 1, 0, 72), (128, 64), 264, gscale=True, dx_add=False, dx_mask=False),   # P = 1023
    _case("dgrad_3x3_n24_all", "dgrad", (2, 9, 11, 40, 3, 1, 1, 24), (64, 64), gscale=True, dx_add=True, dx_mask=True),    # taps change inside a tile, 2 images
    _case("dgrad_3x3_n24_bare", "dgrad", (2, 9, 11, 40, 3, 1, 1, 24), (64, 64), gscale=False, dx_add=False, dx_mask=False),
    _case("dgrad_n12_c8", "dgrad", (1, 7, 5, 8, 3, 1, 1, 12), (64, 64), 1, gscale=True, dx_add=True, dx_mask=False),       # n % 8 == 4, c = 8, P = 35
    _case("dgrad_30_tiles", "dgrad", (2, 6, 7, 136, 3, 1, 1, 100), (64, 64), gscale=True, dx_add=False, dx_mask=True),     # splits 2, 3, 30
    _case("dgrad_one_tile", "dgrad", (3, 5, 5, 72, 1, 1, 0, 20), (64, 64), gscale=False, dx_add=True, dx_mask=True),       # one reduction tile
    _case("dgrad_1x3", "dgrad", (2, 5, 9, 16, 1, 1, 0, 40), (64, 64), kw=3, pad=(0, 1, 0, 1), gscale=True, dx_add=True, dx_mask=True),
    _case("dgrad_3x1", "dgrad", (2, 9, 5, 16, 3, 1, 0, 40), (64, 64), kw=1, pad=(1, 0, 1, 0), gscale=False, dx_add=False, dx_mask=True),
    # ---- weight gradient
    _case("wgrad_128x128_ragged", "wgrad", (1, 10, 10, 456, 3, 1, 1, 1032), (128, 128), gscale=True, modes=(0,)),          # K = 32*128 + 8, 4 reduction tiles
    _case("wgrad_128x64_ragged", "wgrad", (1, 10, 10, 4104, 1, 1, 0, 520), (128, 64), 297, gscale=False, modes=(1,)),      # n = 512 + 8
    _case("wgrad_s2_3x3", "wgrad", (2, 13, 11, 24, 3, 2, 1, 104), (64, 64), gscale=True, modes=(0,)),                      # M = 84
    _case("wgrad_s2_1x1", "wgrad", (3, 14, 14, 72, 1, 2, 0, 72), (64, 64), gscale=True, modes=(2,)),                       # K = 72
    _case("wgrad_modes_db", "wgrad", (2, 9, 11, 40, 3, 1, 1, 24), (64, 64), gscale=True, modes=(0, 1, 2), db=True),
    _case("wgrad_m1_k8", "wgrad", (1, 1, 1, 8, 1, 1, 0, 8), (64, 64), 1, gscale=False, modes=(0, 1)),                      # M = 1, K = 8
    _case("wgrad_9_tiles", "wgrad", (2, 12, 11, 40, 3, 1, 1, 24), (64, 64), gscale=True, modes=(1,)),                      # M = 264: a split of 8 exists
    _case("wgrad_1x3", "wgrad", (2, 5, 9, 16, 1, 1, 0, 40), (64, 64), kw=3, pad=(0, 1, 0, 1), gscale=True, modes=(0,)),
    _case("wgrad_3x1", "wgrad", (2, 9, 5, 16, 3, 2, 0, 40), (64, 64), kw=1, pad=(1, 0, 1, 0), gscale=False, modes=(0,)),   # and stride 2
]
CASES = collections.OrderedDict((c.name, c) for c in _TABLE)
assert len(CASES) == len(_TABLE)

# splits that must exist (a subset of {2, 3, nrt} beyond 1), from the issue's table: checked against the reduction tile count on the CPU
NEEDS_SPLITS = {"fwd_128x128_ragged": (2, 3), "fwd_deep_k": (2, 3, 33), "fwd_s2_3x3_split": (2, 3, 7), "dgrad_128x128_ragged": (2, 3),
                "dgrad_30_tiles": (2, 3, 30), "dgrad_one_tile": (), "wgrad_128x128_ragged": (2, 3, 4), "wgrad_m1_k8": (), "wgrad_9_tiles": (2, 3, 9)}
SINGLE_TILE = ("dgrad_one_tile", "wgrad_m1_k8")          # one reduction tile: taps * n8 <= 32 / M < 32


def gpu_order():
    """Case names alternating forward, dgrad, wgrad: the three kernels share a context's arrival counters and slab area."""
    by = {k: [c.name for c in _TABLE if c.kind == k] for k in ("fwd", "dgrad", "wgrad")}
    out = []
    for i in range(max(len(v) for v in by.values())):
        out += [v[i] for v in (by["fwd"], by["dgrad"], by["wgrad"]) if i < len(v)]
    return out


# ---------------------------------------------------------------------------------------------------------------- geometry
def geometry(cs):
    """oh, ow, M (output pixels), P (input pixels), K (kh*kw*c), n8, (rows, cols) of the launch's output and its reduction tiles."""
    pt, pl, pb, pr = cs.pad
    oh, ow = (cs.h + pt + pb - cs.kh) // cs.stride + 1, (cs.w + pl + pr - cs.kw) // cs.stride + 1
    M, P, K, n8 = cs.nb * oh * ow, cs.nb * cs.h * cs.w, cs.kh * cs.kw * cs.c, (cs.n + 7) // 8 * 8
    if cs.kind == "fwd":
        rows, cols, nrt = M, cs.n, (K + 31) // 32
    elif cs.kind == "dgrad":
        rows, cols, nrt = P, cs.c, (cs.kh * cs.kw * n8 + 31) // 32
    else:
        rows, cols, nrt = K, cs.n, (M + 31) // 32
    return dict(oh=oh, ow=ow, M=M, P=P, K=K, n8=n8, rows=rows, cols=cols, nrt=nrt)


def splits(cs):
    """Every split of {1, 2, 3, nrt} the case's reduction tile count allows (at most 64)."""
    nrt = geometry(cs)["nrt"]
    return sorted(s for s in {1, 2, 3, nrt} if s <= min(nrt, 64))


def pitches(cs):
    """Row pitches in floats (weights: bf16 elements), every one wider than its row and the output-side ones pairwise different."""
    g = geometry(cs)
    return dict(ldw=cs.n + 3, ldk=(g["K"] + 31) // 32 * 32 + 8, ldy=cs.n + 3, ld_add=cs.n + 5,
                ld_dy=g["n8"] + 4, ldkd=(cs.kh * cs.kw * g["n8"] + 31) // 32 * 32 + 8, ld_dx=cs.c + 8, ld_dx_add=cs.c + 3, ld_dx_mask=cs.c + 5,
                ld_dw=cs.n + 4, ld_dy_w=cs.n + 4)


# ---------------------------------------------------------------------------------------------------------------- numbers
def bf16_bits(a):
    """Round to nearest, ties to even, fp32 -> bf16 bit patterns (uint16); finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(a):
    """fp32 values rounded to bf16, as float64."""
    return (bf16_bits(a).astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(np.shape(a))


def _biased(rs, shape, scale=1.0):
    """Half the values in (1 + 2^-9, 1 + 2^-8) -- bf16 rounds every one of them DOWN -- the rest normal; scale: a power of two."""
    v = rs.uniform(1 + 2.0 ** -9, 1 + 2.0 ** -8, shape)
    return (np.where(rs.rand(*shape) < 0.5, v, rs.randn(*shape)) * scale).astype(np.float32)


def _pow2(v):
    return 2.0 ** -int(round(np.log2(v)))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Dense fp32 inputs of a case from its seed (its position in the table); the tests lay them out with `pitches` / `padded`."""
    cs = CASES[name]
    g = geometry(cs)
    rs = np.random.RandomState(1000 + list(CASES).index(name))
    taps = cs.kh * cs.kw
    d = dict(w=_biased(rs, (g["K"], cs.n), _pow2(np.sqrt(g["K"] if cs.kind == "fwd" else taps * cs.n))))
    if cs.kind != "dgrad":
        d["x"] = _biased(rs, (cs.nb, cs.h, cs.w, cs.c))
    if cs.kind == "fwd":
        d["scale"] = rs.uniform(0.5, 1.5, cs.n).astype(np.float32)
        d["shift"] = rs.randn(cs.n).astype(np.float32)
        d["addend"] = rs.randn(g["M"], cs.n).astype(np.float32)
    else:
        d["dy"] = _biased(rs, (g["M"], cs.n), _pow2(np.sqrt(g["M"])) if cs.kind == "wgrad" else 1.0)
        d["gscale"] = rs.uniform(0.5, 1.5, cs.n).astype(np.float32) if cs.opts.get("gscale") else None
    if cs.kind == "dgrad":
        d["dx_add"] = rs.randn(g["P"], cs.c).astype(np.float32) if cs.opts.get("dx_add") else None
        d["dx_mask"] = rs.randn(g["P"], cs.c).astype(np.float32) if cs.opts.get("dx_mask") else None
    if cs.kind == "wgrad":
        d["dw0"] = rs.randn(g["K"], cs.n).astype(np.float32)
        d["db0"] = rs.randn(cs.n).astype(np.float32)
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


def padded(a, ld, fill=np.nan):
    """A [rows][cols] matrix laid out with pitch ld, `fill` in the padding."""
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


# ---------------------------------------------------------------------------------------------------------------- references
def im2col(x, cs):
    """[M][kh*kw*c] float64: k = (ky, kx, channel), zeros for taps outside the image."""
    g = geometry(cs)
    pt, pl = cs.pad[0], cs.pad[1]
    m = np.arange(g["M"])
    img, r = m // (g["oh"] * g["ow"]), m % (g["oh"] * g["ow"])
    oy, ox = r // g["ow"], r % g["ow"]
    A = np.zeros((g["M"], cs.kh, cs.kw, cs.c), np.float64)
    for ky in range(cs.kh):
        for kx in range(cs.kw):
            iy, ix = oy * cs.stride - pt + ky, ox * cs.stride - pl + kx
            ok = (iy >= 0) & (iy < cs.h) & (ix >= 0) & (ix < cs.w)
            A[ok, ky, kx, :] = x[img[ok], iy[ok], ix[ok], :]
    return A.reshape(g["M"], -1)


def col2im_gather(gm, cs):
    """dgrad's A operand [P][kh*kw*n]: element (p, (ky, kx, j)) = g[q(p, ky, kx)][j], zero where q falls off the output grid."""
    g = geometry(cs)
    pt, pl = cs.pad[0], cs.pad[1]
    p = np.arange(g["P"])
    img, r = p // (cs.h * cs.w), p % (cs.h * cs.w)
    ih, iw = r // cs.w, r % cs.w
    A = np.zeros((g["P"], cs.kh, cs.kw, cs.n), np.float64)
    for ky in range(cs.kh):
        for kx in range(cs.kw):
            qh, qw = ih + pt - ky, iw + pl - kx
            ok = (qh >= 0) & (qh < g["oh"]) & (qw >= 0) & (qw < g["ow"])
            A[ok, ky, kx, :] = gm[(img[ok] * g["oh"] + qh[ok]) * g["ow"] + qw[ok]]
    return A.reshape(g["P"], -1)


def g_matrix(name):
    """dy * gscale as one fp32 multiply (fp32 array)."""
    d = inputs(name)
    return d["dy"] * d["gscale"][None, :] if d["gscale"] is not None else d["dy"].copy()


def _act(v, act, act_cols):
    if act == 1:
        return np.maximum(v, 0)
    if act == 2:
        v = v.copy()
        v[:, :act_cols] = 1.0 / (1.0 + np.exp(-v[:, :act_cols]))
    return v


def finish(name, dot, mode=0):
    """The epilogue of the case's kernel on a raw sum `dot` (float64): what the output must be for that sum."""
    cs, d = CASES[name], inputs(name)
    if cs.kind == "fwd":
        tail = d["shift"].astype(np.float64)[None, :] + d["addend"].astype(np.float64)
        return _act(dot * d["scale"].astype(np.float64)[None, :] + tail, cs.opts.get("act", 0), cs.opts.get("act_cols", 0))
    if cs.kind == "dgrad":
        v = dot + (d["dx_add"].astype(np.float64) if d["dx_add"] is not None else 0.0)
        return np.where(d["dx_mask"] > 0, v, 0.0) if d["dx_mask"] is not None else v
    return dot + (d["dw0"].astype(np.float64) if mode == 1 else 0.0)       # mode 2 adds to the zeros the caller wrote


@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(dot, dot_u, absdot) of the case's raw sums -- every output element, float64; computed once, read-only."""
    cs, d = CASES[name], inputs(name)
    w = d["w"].astype(np.float64)
    if cs.kind == "fwd":
        A, B = im2col(d["x"], cs), w
        Ab, Bb = bf16_round(A), bf16_round(d["w"])
    elif cs.kind == "dgrad":
        gm = g_matrix(name)
        tr = lambda m: m.reshape(cs.kh, cs.kw, cs.c, cs.n).transpose(0, 1, 3, 2).reshape(cs.kh * cs.kw * cs.n, cs.c)      # [(ky, kx, j)][c]
        A, B = col2im_gather(gm.astype(np.float64), cs), tr(w)
        Ab, Bb = col2im_gather(bf16_round(gm), cs), tr(bf16_round(d["w"]))
    else:
        gm = g_matrix(name)
        A, B = im2col(d["x"], cs).T, gm.astype(np.float64)
        Ab, Bb = bf16_round(A), bf16_round(gm)
    out = dict(dot=Ab @ Bb, dot_u=A @ B, absdot=np.abs(Ab) @ np.abs(Bb))
    if cs.kind == "wgrad":
        out["db_u"] = g_matrix(name).astype(np.float64).sum(0)              # the bias gradient: fp64 column sum of the UNROUNDED dy * gscale
        out["db_abs"] = np.abs(g_matrix(name).astype(np.float64)).sum(0)
    for v in out.values():
        v.setflags(write=False)
    return out


def expected(name, mode=0):
    """(ref, ref_u, tol) for the whole output: the bound is the existing bf16 tests', 1e-5 * sum|a*b| (* scale) + 1e-6 * (1 + |tail|)."""
    cs, d, r = CASES[name], inputs(name), reference(name)
    if cs.kind == "fwd":
        tail = np.abs(d["shift"].astype(np.float64)[None, :] + d["addend"].astype(np.float64))
        tol = 1e-5 * r["absdot"] * d["scale"].astype(np.float64)[None, :] + 1e-6 * (1.0 + tail)
    elif cs.kind == "dgrad":
        tol = 1e-5 * r["absdot"] + 1e-6 * (1.0 + (np.abs(d["dx_add"].astype(np.float64)) if d["dx_add"] is not None else 0.0))
    else:
        tol = 1e-5 * r["absdot"] + 1e-6 * (1.0 + (np.abs(d["dw0"].astype(np.float64)) if mode == 1 else 0.0))
    return finish(name, r["dot"], mode), finish(name, r["dot_u"], mode), tol
