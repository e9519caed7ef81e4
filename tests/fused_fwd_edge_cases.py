"""Case tables and NumPy references of the edge tests of the two fused forward launches, radnet_conv_fwd_pair and
radnet_conv_bottleneck (device-free check of the tables, the references and their teeth: tests/test_fused_fwd_edge_cases_reference.py;
the kernels: tests/test_gpu_fused_fwd_edges.py).  No torch, no library.  Built on tests/fp32_edge_cases.py: its gather, its pitch
idiom (`_view` / `_stored`: an operand read or written through a pitch, so that a mutant is the same code with one parameter changed),
its sentinel, its bound and its sigmoid rule.

Every problem is a list of forward layers as include/radnet_hip.h states them,

  y[m][j] = act( (sum_k im2col(x)[m][k] * w[k][j]) * scale[j] + shift[j] + addend[m][j] ),

a PAIR two independent ones, a BOTTLENECK a chain: db (3x3 'same', 64 columns, ReLU), dc (1x1 on db's output, + addend, ReLU), da (1x1
on dc's output, 64 columns, ReLU) or nothing.  `pair(name)` / `chain(name, with_next)` give every output BUFFER in float64 -- [M + 1][pitch],
NaN wherever nothing may be written: the pitch padding, the extra row, the sentinel columns of p_col_blocks -- and a bound of the same
shape.  The bound is derived, not tuned.  One layer (fp32_edge_cases.py): an fp32 sum of K products in any order, with or without FMA
contraction, lies within (K + 8) u sum|a b| of the exact sum after the epilogue's multiplies and adds, u = 2^-24.  A chain carries the
error of its input along; the ReLU is 1-Lipschitz and a 1x1 convolution is linear, so with E_in the bound of the layer's input

  E = (K + 8) u (((|x| + E_in) @ |w|) |scale| + |shift| + |addend|) + (E_in @ |w|) |scale|

which for the bottleneck is E1 = (9c + 8) u (A1 |sb| + |bb|), E2 = (64 + 8) u (A2 |sc| + |shc| + |add|) + (E1 @ |wc|) |sc| with
A2 = (|t2| + E1) @ |wc|, and E3 = (N2 + 8) u (A3 |sa| + |ba|) + (E2 @ |wa|) |sa| with A3 = (|y| + E2) @ |wa|.  It holds for the fused
launch and for the separate launches alike (they are not bit-equal: different reduction orders).  Sigmoid columns: a quarter of the
pre-activation bound plus SIGMOID_SLACK.  The integer cases (p_exact, b_exact) have sum|a b| below 2^24 units at every layer: every
partial sum in any order is exact and the device must return the float64 result itself.

Measured on one MI355X (worst |gpu - float64| / bound over all elements of all cases and pinnings; reported, not used to set the bound):
  radnet_conv_fwd_pair, one launch      0.072 (p_pitch, tile 64x64; p_deep_k with 33 K tiles: 0.002) -- and the bits of radnet_conv_fwd
                                        of each descriptor forced to the same tile with 4 waves, on every case and tile
  radnet_conv_fwd_pair, two launches    0.058 (p_diff_m)
  radnet_conv_bottleneck, one launch    0.0007 (b_c32, y; every other case 0.0002 .. 0.0005)
  radnet_conv_bottleneck, separate      0.0075 for the chains (b_c32; every other case 0.002 .. 0.004), 0.024 for b_fb_dc_own_x
                                        (dc on an input of its own: a one-layer bound with K = 64)
The chain's bound is loose by construction: it adds the worst case of every layer, and E_in @ |w| takes every input error with the
same sign.  p_exact and b_exact: 0 on every path, as derived.
"""
import collections
import functools

import numpy as np

import fp32_edge_cases as F
from fp32_edge_cases import SENTINEL, SIGMOID_SLACK, U, _stored, _view, gather, im2col, padded  # noqa: F401  (re-exported to the tests)

Layer = collections.namedtuple("Layer", "c k stride pad n act act_cols scale shift addend ldw ldy ld_add")
# scale / shift / addend: whether the pointer is set; ldw / ldy / ld_add: row pitches in floats (ld_add is 0 without an addend)


def layer(c, n, k=1, stride=1, pad=0, act=1, act_cols=0, scale=True, shift=True, addend=False, ldw=None, ldy=None, ld_add=None):
    return Layer(c, k, stride, pad, n, act, act_cols, scale, shift, addend, ldw or n, ldy or n, (ld_add or n) if addend else 0)


def grid(shape, l):
    """(oh, ow, M, K) of layer l on an input of shape (nb, h, w)."""
    nb, h, w = shape
    oh, ow = (h + 2 * l.pad - l.k) // l.stride + 1, (w + 2 * l.pad - l.k) // l.stride + 1
    return oh, ow, nb * oh * ow, l.k * l.k * l.c


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================================ one layer
def fwd_layer(shape, l, x, p, E_in=None, mut=None):
    """(out, tol, pre) [M][n] in float64 of one layer on x [nb*h*w][c] (float64, dense) with parameters p = dict(w, scale, shift,
    addend) (dense fp32, None where the pointer is null), read through the layer's pitches.  E_in: the bound of x's own error."""
    nb, h, w = shape
    oh, ow, M, K = grid(shape, l)
    A = gather(x.reshape(nb, h, w, l.c), nb, h, w, oh, ow, l.k, l.k, l.stride, l.pad, l.pad, wrap=mut == "wrap_taps").reshape(M, K)
    EA = np.zeros_like(A)
    if E_in is not None:
        assert l.k == 1 and l.stride == 1 and E_in.shape == A.shape
        EA = E_in
    W = _view(p["w"], l.ldw, l.ldw)
    if mut == "w3_no_chunk_offset":                                     # every 64-row chunk multiplies the FIRST 64 rows of the matrix
        W = np.tile(W[:64], (K // 64, 1))
    sc = p["scale"].astype(np.float64)[None, :] if l.scale else np.ones((1, l.n))
    sh = p["shift"].astype(np.float64)[None, :] if l.shift else np.zeros((1, l.n))
    if mut == "shift_prev_chunk":                                       # 64-column chunk c takes the shift of chunk c - 1
        sh = np.roll(sh, 64, axis=1)
    add = _view(p["addend"], l.ld_add, l.ldy if mut == "add_with_ldy" else l.ld_add) if l.addend else np.zeros((M, l.n))
    pre = (A @ W) * sc + sh + add
    tol = (K + 8) * U * (((np.abs(A) + EA) @ np.abs(W)) * np.abs(sc) + np.abs(sh) + np.abs(add)) + (EA @ np.abs(W)) * np.abs(sc)
    out = np.maximum(pre, 0) if l.act == 1 and mut != "no_relu" else pre.copy()
    if l.act == 2:
        out[:, :l.act_cols] = 1.0 / (1.0 + np.exp(-pre[:, :l.act_cols]))
        tol[:, :l.act_cols] = 0.25 * tol[:, :l.act_cols] + SIGMOID_SLACK
    return out, tol, pre


class Buffers:
    """The output buffers of a problem: name -> float64 [rows + 1][ld], NaN where nothing was written; the bound likewise."""

    def __init__(self):
        self.val, self.tol, self.pre = {}, {}, {}

    def new(self, key, rows, ld):
        if key not in self.val:
            self.val[key], self.tol[key], self.pre[key] = (np.full((rows + 1, ld), np.nan) for _ in range(3))

    def put(self, key, out, tol, pre, ld_used=None, c0=0, rows=None):
        """Store `out` (and its bound) as a writer that believes the pitch is `ld_used` would; rows = how many of them (a mutant: M + 1)."""
        ld = self.val[key].shape[1]
        ld_used = ld_used or ld
        for dst, src in ((self.val[key], out), (self.tol[key], tol), (self.pre[key], pre)):
            flat = dst.reshape(-1)
            for r in range(src.shape[0] if rows is None else rows):
                a = r * ld_used + c0
                n = max(0, min(src.shape[1], flat.size - a))
                flat[a:a + n] = src[min(r, src.shape[0] - 1), :n]

    def freeze(self):
        for d in (self.val, self.tol, self.pre):
            for v in d.values():
                v.setflags(write=False)
        return self


def verdict(got, untouched, ref, tol):
    """(worst err / tol inside -- inf for a non-finite element --, elements outside the bound, elements outside the rows that were
    written).  got: the buffer; untouched: where it still holds what it was prefilled with; ref / tol: NaN outside the rows."""
    inside = ~np.isnan(ref)
    err = np.abs(got[inside].astype(np.float64) - ref[inside])
    ratio = np.where(np.isfinite(err), err / np.maximum(tol[inside], 1e-300), np.inf)
    ratio = np.where(err == 0, 0.0, ratio)
    return float(ratio.max()), int((ratio > 1).sum()), int((~untouched[~inside]).sum())


def _rs(table, name):
    return np.random.RandomState(7000 + list(table).index(name))


def _params(rs, l, M, exact=False, ints=(-1, 1)):
    """Weights normal / sqrt(K), scale in [0.5, 1.5), shift and addend normal -- or small integers and a power-of-two scale."""
    K = l.k * l.k * l.c
    if exact:
        p = dict(w=rs.randint(ints[0], ints[1] + 1, (K, l.n)).astype(np.float32), scale=np.full(l.n, 2.0 ** -3, np.float32),
                 shift=rs.randint(-2, 3, l.n).astype(np.float32), addend=rs.randint(-2, 3, (M, l.n)).astype(np.float32))
    else:
        p = dict(w=(rs.standard_normal((K, l.n)) / np.sqrt(K)).astype(np.float32), scale=rs.uniform(0.5, 1.5, l.n).astype(np.float32),
                 shift=(0.5 * rs.standard_normal(l.n)).astype(np.float32), addend=rs.standard_normal((M, l.n)).astype(np.float32))
    for key, have in (("scale", l.scale), ("shift", l.shift), ("addend", l.addend)):
        if not have:
            p[key] = None
    return p


def _readonly(d):
    for v in d.values():
        if isinstance(v, dict):
            _readonly(v)
        elif v is not None:
            v.setflags(write=False)
    return d


# ================================================================================================================ the pair
Pair = collections.namedtuple("Pair", "name shapes layers same_x col_block tiles exact expect")
TILES = ((64, 64), (32, 64), (32, 32))


def _pair(name, shape, l1, l2, shape2=None, same_x=True, col_block=False, tiles=TILES, exact=False, **expect):
    return Pair(name, (shape, shape2 or shape), (l1, l2), same_x, col_block, tiles, exact, expect)


_EPI1 = dict(act=1, addend=True)                       # ReLU + addend + scale + shift
_EPI2 = dict(act=2, act_cols=20, scale=False)          # sigmoid on the first 20 columns, no scale
_PAIRS = [
    _pair("p_ragged", (1, 9, 15), layer(32, 68), layer(32, 36, act=0), M=135),            # M = 2*64 + 7; cdiv(N, bn) differs between the tiles
    _pair("p_m1", (1, 1, 1), layer(32, 4), layer(32, 4, act=0), M=1),
    _pair("p_n_order", (1, 9, 15), layer(32, 36), layer(32, 132, act=0), M=135),
    _pair("p_n_order_swapped", (1, 9, 15), layer(32, 132, act=0), layer(32, 36), M=135),
    _pair("p_s2_1x1", (3, 14, 14), layer(64, 40, stride=2), layer(64, 100, stride=2, act=0), M=147),
    _pair("p_3x3_two_images", (2, 9, 11), layer(32, 36, k=3, pad=1, **_EPI1), layer(32, 100, k=3, pad=1, **_EPI2), M=198),
    _pair("p_two_inputs", (1, 9, 15), layer(32, 68), layer(32, 36, act=0), same_x=False, M=135),
    _pair("p_deep_k", (1, 6, 7), layer(1056, 100), layer(1056, 36, act=0), M=42, nk=33),
    _pair("p_pitch", (1, 9, 15), layer(32, 68, ldw=72, ldy=76, ld_add=80, **_EPI1), layer(32, 36, ldw=44, ldy=48, ld_add=52, act=0, addend=True), M=135),
    _pair("p_col_blocks", (1, 9, 15), layer(32, 68, ldy=68 + 36 + 8), layer(32, 36, act=0, ldy=68 + 36 + 8), col_block=True, M=135),
    _pair("p_exact", (2, 5, 7), layer(32, 68, k=3, pad=1, addend=True), layer(32, 36, k=3, pad=1, act=0), exact=True, M=70),
    # ---- what the paired launch does not take: the two calls (run on the device as fallbacks; p_diff_m also feeds a mutant)
    _pair("p_diff_m", (1, 9, 15), layer(32, 68), layer(32, 132, act=0), shape2=(1, 5, 15), same_x=False, tiles=(), M=135),   # 3 and 2 row tiles of 64
    _pair("p_diff_k", (1, 9, 15), layer(32, 68), layer(64, 36, act=0), same_x=False, tiles=(), M=135),
    _pair("p_stem", (2, 11, 13), layer(4, 68, k=7, stride=2, pad=3), layer(4, 36, k=7, stride=2, pad=3, act=0), tiles=(), M=84),
]
PAIRS = collections.OrderedDict((c.name, c) for c in _PAIRS)
assert len(PAIRS) == len(_PAIRS)
PAIR_FALLBACK_SHAPES = ("p_diff_m", "p_diff_k", "p_stem")


@functools.lru_cache(maxsize=None)
def pair_inputs(name):
    cs = PAIRS[name]
    rs = _rs(PAIRS, name)
    d = {}
    for i, (shape, l) in enumerate(zip(cs.shapes, cs.layers)):
        nb, h, w = shape
        if i == 0 or not cs.same_x:
            x = rs.randint(-2, 3, (nb * h * w, l.c)) if cs.exact else rs.standard_normal((nb * h * w, l.c))
            d["x%d" % (i + 1)] = x.astype(np.float32)
        d["p%d" % (i + 1)] = _params(rs, l, grid(shape, l)[2], cs.exact)
    if cs.same_x:
        d["x2"] = d["x1"]
    return _readonly(d)


def pair_slot(cs, i):
    """(buffer name, first column, pitch) of the i-th output: p_col_blocks writes the left and right column blocks of ONE tensor."""
    if cs.col_block:
        return "y", (0 if i == 0 else cs.layers[0].n), cs.layers[i].ldy
    return "y%d" % (i + 1), 0, cs.layers[i].ldy


PAIR_MUTANTS = collections.OrderedDict([          # mutant -> the cases that must catch it
    ("add_with_ldy", ("p_pitch",)), ("y_with_ld_add", ("p_pitch",)), ("wrap_taps", ("p_3x3_two_images",)),
    ("second_with_n1", ("p_n_order",)), ("gx1_for_second", ("p_diff_m",))])


def _pair_outputs(name, mut=None):
    cs, d = PAIRS[name], pair_inputs(name)
    return [fwd_layer(cs.shapes[i], cs.layers[i], d["x%d" % (i + 1)].astype(np.float64), d["p%d" % (i + 1)],
                      mut=mut if mut in ("add_with_ldy", "wrap_taps") else None) for i in range(2)]


def _pair_buffers(name, outs, mut=None, units=None):
    """The buffers after both problems stored `outs` -- whole, or (units) one output tile at a time."""
    cs = PAIRS[name]
    b = Buffers()
    for i in range(2):
        key, c0, ld = pair_slot(cs, i)
        b.new(key, grid(cs.shapes[i], cs.layers[i])[2], ld)
    if units is None:
        for i, (out, tol, pre) in enumerate(outs):
            key, c0, ld = pair_slot(cs, i)
            b.put(key, out, tol, pre, cs.layers[i].ld_add if mut == "y_with_ld_add" and cs.layers[i].addend else None, c0)
        return b
    bm, bn = units[0]
    for i, tm, tn in units[1]:
        key, c0, ld = pair_slot(cs, i)
        sub = tuple(a[tm * bm:(tm + 1) * bm, tn * bn:(tn + 1) * bn] for a in outs[i])
        if sub[0].size:
            flat_rows = np.arange(tm * bm, tm * bm + sub[0].shape[0])
            for dst, src in zip((b.val[key], b.tol[key], b.pre[key]), sub):
                dst[flat_rows[:, None], c0 + tn * bn + np.arange(sub[0].shape[1])[None, :]] = src
    return b


@functools.lru_cache(maxsize=None)
def pair(name):
    """Buffers (val, tol, pre) of the case's true result: float64, every element of every buffer; computed once, read-only."""
    return _pair_buffers(name, _pair_outputs(name)).freeze()


def pair_units(cs, bm, bn, mut=None):
    """[(problem, row tile, column tile)] per workgroup of the paired launch on tile bm x bn: workgroups [0, n1) run the first problem,
    [n1, n1 + n2) the second, each numbered row tile fastest with ITS OWN row-tile count."""
    (M1, N1), (M2, N2) = ((grid(cs.shapes[i], cs.layers[i])[2], cs.layers[i].n) for i in range(2))
    gx1, gx2 = cdiv(M1, bm), cdiv(M2, bm)
    n1, n2 = gx1 * cdiv(N1, bn), gx2 * cdiv(N1 if mut == "second_with_n1" else N2, bn)
    out = []
    for b in range(n1 + n2):
        if b < n1:
            out.append((0, b % gx1, b // gx1))
        else:
            gx = gx1 if mut == "gx1_for_second" else gx2
            out.append((1, (b - n1) % gx, (b - n1) // gx))
    return out


def pair_by_tiles(name, bm, bn, mut=None):
    """The buffers after a launch that maps workgroups to tiles as pair_units says (each tile stores the true values of its part)."""
    return _pair_buffers(name, _pair_outputs(name), units=((bm, bn), pair_units(PAIRS[name], bm, bn, mut)))


def pair_mutant(name, mut, tile=(64, 64)):
    assert name in PAIR_MUTANTS[mut]
    if mut in ("second_with_n1", "gx1_for_second"):
        return pair_by_tiles(name, tile[0], tile[1], mut)
    return _pair_buffers(name, _pair_outputs(name, mut), mut)


# ================================================================================================================ the bottleneck
Bneck = collections.namedtuple("Bneck", "name shape layers linked forms exact fusable expect")
# layers = (db, dc, da); linked = dc reads db's output (False: an input of its own); forms = the with_next values the case runs;
# fusable = whether radnet_conv_bottleneck may take the one-launch form (False: a fallback, or a pitched intermediate)


def _bneck(name, shape, c=64, n2=128, db=None, dc=None, da=None, linked=True, forms=(False, True), exact=False, fusable=True, **expect):
    db = dict(dict(k=3, pad=1), **(db or {}))
    dc = dict(dict(addend=True), **(dc or {}))
    lb = layer(c, db.pop("n", 64), **db)
    lc = layer(dc.pop("c", lb.n), n2, **dc)
    la = layer(n2, (da or {}).pop("n", 64), **(da or {}))
    return Bneck(name, shape, (lb, lc, la), linked, forms, exact, fusable, expect)


def straddling(M, bm):
    """First rows (row0 = tile + 32 wm + 4 hi) of the lanes whose 16 accumulator rows row0 + {0..3, 8..11, 16..19, 24..27} lie on
    both sides of M: such a lane stores some registers and must drop the others."""
    out = []
    for m0 in range(0, M, bm):
        for wm in range(bm // 32):
            for hi in range(2):
                row0 = m0 + 32 * wm + 4 * hi
                rows = [row0 + (r & 3) + 8 * (r >> 2) for r in range(16)]
                if row0 < M and rows[-1] >= M:
                    out.append(row0)
    return out


_NULLS = [("sb", 0, "scale"), ("bb", 0, "shift"), ("sc", 1, "scale"), ("shc", 1, "shift"), ("add", 1, "addend"), ("sa", 2, "scale"), ("ba", 2, "shift")]


def _null_cases():
    out = []
    for tag, i, field in _NULLS:
        kw = {("db", "dc", "da")[i]: {field: False}}
        out.append(_bneck("b_nulls_" + tag, (1, 5, 13), forms=(True,) if i == 2 else (False, True), M=65, **kw))
    off = dict(scale=False, shift=False)
    out.append(_bneck("b_nulls_all", (1, 5, 13), db=dict(off), dc=dict(off, addend=False), da=dict(off), M=65))
    return out


_BNECKS = [
    _bneck("b_m_small", (1, 3, 5), M=15, straddle64=[0, 4], straddle32=[0, 4]),            # rows_ok false for the whole second wave row
    _bneck("b_m_seams_29", (1, 1, 29), M=29, straddle64=[4], straddle32=[4]),
    _bneck("b_m_seams_35", (1, 5, 7), M=35, straddle64=[32], straddle32=[32]),
    _bneck("b_m_seams_61", (1, 1, 61), M=61, straddle64=[36], straddle32=[36]),
    _bneck("b_m_seams_64", (1, 8, 8), M=64, straddle64=[], straddle32=[]),
    _bneck("b_m_seams_65", (1, 5, 13), M=65, straddle64=[64], straddle32=[64]),
    _bneck("b_two_images", (3, 5, 7), M=105),                                              # image seams at rows 35 and 70 inside tiles
    _bneck("b_h1", (1, 1, 9), M=9),
    _bneck("b_w1", (1, 7, 1), M=7),
    _bneck("b_n2_64", (1, 5, 13), n2=64, M=65, chunks=1),
    _bneck("b_n2_320", (2, 9, 11), n2=320, M=198, chunks=5),                               # the largest case
    _bneck("b_c32", (1, 5, 13), c=32, M=65, K1=288),
    _bneck("b_c96", (1, 5, 13), c=96, M=65, K1=864),
] + _null_cases() + [
    _bneck("b_pitch", (1, 5, 13), db=dict(ldw=68), dc=dict(ldw=132, ldy=136, ld_add=140), forms=(False,), M=65),
    _bneck("b_pitch_next", (1, 5, 13), db=dict(ldw=68), dc=dict(ldw=132, ld_add=140), da=dict(ldw=72, ldy=76), forms=(True,), M=65),
    _bneck("b_relu_exact", (1, 5, 13), M=65),                                              # shifts at the column medians: see bneck_inputs
    _bneck("b_exact", (2, 5, 7), exact=True, M=70),
    # ---- the pitched intermediates: the separate launches read a pitched db->y / dc->y as dense, the fused launch never sees the pitch
    _bneck("b_pitched_t2", (1, 5, 13), db=dict(ldy=72), fusable=False, M=65),
    _bneck("b_pitched_y_with_next", (1, 5, 13), dc=dict(ldy=136), forms=(True,), fusable=False, M=65),
    # ---- what the fused launch does not take
    _bneck("b_fb_db_n32", (1, 5, 13), db=dict(n=32), fusable=False, M=65),
    _bneck("b_fb_db_addend", (1, 5, 13), db=dict(addend=True), fusable=False, M=65),
    _bneck("b_fb_dc_act0", (1, 5, 13), dc=dict(act=0), fusable=False, M=65),
    _bneck("b_fb_dc_own_x", (1, 5, 13), linked=False, fusable=False, M=65),
    _bneck("b_fb_n2_96", (1, 5, 13), n2=96, fusable=False, M=65),
    _bneck("b_fb_da_n32", (1, 5, 13), da=dict(n=32), forms=(True,), fusable=False, M=65),
]
BNECKS = collections.OrderedDict((c.name, c) for c in _BNECKS)
assert len(BNECKS) == len(_BNECKS)
PITCHED_INTERMEDIATE = ("b_pitched_t2", "b_pitched_y_with_next")
BNECK_KEYS = ("t2", "y", "t")


@functools.lru_cache(maxsize=None)
def bneck_inputs(name):
    cs = BNECKS[name]
    rs = _rs(BNECKS, name)
    nb, h, w = cs.shape
    M = nb * h * w
    lb, lc, la = cs.layers
    d = dict(x=(rs.randint(-2, 3, (M, lb.c)) if cs.exact else rs.standard_normal((M, lb.c))).astype(np.float32))
    d["x2"] = None if cs.linked else rs.standard_normal((M, lc.c)).astype(np.float32)
    for key, l in zip(("pb", "pc", "pa"), cs.layers):
        d[key] = _params(rs, l, M, cs.exact)
    if name == "b_relu_exact":
        # every column's shift = minus the median of the rest of its pre-activation: about half of t2, y and t are negative before the ReLU
        x = d["x"].astype(np.float64)
        for key, l in zip(("pb", "pc", "pa"), cs.layers):
            p = dict(d[key], shift=np.zeros(l.n, np.float32))
            out, _, pre = fwd_layer(cs.shape if l.k == 3 else (1, 1, M), l, x, p)
            d[key]["shift"] = (-np.median(pre, axis=0)).astype(np.float32)
            x = fwd_layer(cs.shape if l.k == 3 else (1, 1, M), l, x, d[key])[0]
    return _readonly(d)


BNECK_MUTANTS = collections.OrderedDict([         # mutant -> (layer it changes, the cases -- with the trailing reduce or not -- that must catch it)
    ("add_with_ldy", (1, (("b_pitch", False),))),
    ("y_with_ld_add", (1, (("b_pitch", False),))),
    ("shift_prev_chunk", (1, (("b_n2_320", True), ("b_m_seams_65", False)))),
    ("w3_no_chunk_offset", (2, (("b_m_seams_65", True), ("b_n2_320", True)))),
    ("no_relu", (0, (("b_relu_exact", False), ("b_relu_exact", True)))),
    ("no_relu_2", (1, (("b_relu_exact", True),))),
    ("wrap_taps", (0, (("b_two_images", False), ("b_w1", True)))),
    ("store_row_m", (1, (("b_m_small", False), ("b_m_seams_65", True)))),
])


def _chain(name, with_next, mut=None):
    cs, d = BNECKS[name], bneck_inputs(name)
    nb, h, w = cs.shape
    M = nb * h * w
    lb, lc, la = cs.layers
    at = BNECK_MUTANTS[mut][0] if mut else -1
    m = lambda i: ("no_relu" if mut == "no_relu_2" else mut) if at == i and mut not in ("y_with_ld_add", "store_row_m") else None
    b = Buffers()
    t2, E1, pre1 = fwd_layer(cs.shape, lb, d["x"].astype(np.float64), d["pb"], mut=m(0))
    b.new("t2", M, lb.ldy)
    b.put("t2", t2, E1, pre1)
    flat = (1, 1, M)
    # radnet_conv_desc has no pitch for x: a layer reads the buffer before it as a dense [M][c] matrix, whatever pitch it was written with
    dense = lambda buf, c: buf.reshape(-1)[:M * c].reshape(M, c)
    if cs.linked:
        x2, E_in = dense(b.val["t2"], lc.c), dense(b.tol["t2"], lc.c)
    else:
        x2, E_in = d["x2"].astype(np.float64), None
    y, E2, pre2 = fwd_layer(flat, lc, x2, d["pc"], E_in, mut=m(1))
    b.new("y", M, lc.ldy)
    b.put("y", y, E2, pre2, lc.ld_add if mut == "y_with_ld_add" else None, rows=M + 1 if mut == "store_row_m" else None)
    if with_next:
        t, E3, pre3 = fwd_layer(flat, la, dense(b.val["y"], la.c), d["pa"], dense(b.tol["y"], la.c), mut=m(2))
        b.new("t", M, la.ldy)
        b.put("t", t, E3, pre3)
    return b


@functools.lru_cache(maxsize=None)
def chain(name, with_next):
    """Buffers t2, y (and t) of the case as the three (two) separate launches define them: float64, every element; read-only."""
    return _chain(name, with_next).freeze()


def chain_mutant(name, with_next, mut):
    assert (name, with_next) in BNECK_MUTANTS[mut][1]
    return _chain(name, with_next, mut)


# ================================================================================================================ fp32 emulations
def _emulate_layer(shape, l, x, p, order):
    """One layer in fp32 arithmetic: the products summed in the order of a k-ordered chain per output element ('chain': the matrix
    cores' order within a K tile, products and sums rounded separately) or as NumPy's own fp32 matrix product ('blas')."""
    nb, h, w = shape
    oh, ow, M, K = grid(shape, l)
    A = gather(x.reshape(nb, h, w, l.c), nb, h, w, oh, ow, l.k, l.k, l.stride, l.pad, l.pad).reshape(M, K).astype(np.float32)
    W = p["w"]
    if order == "blas":
        acc = A @ W
    else:
        acc = np.zeros((M, l.n), np.float32)
        for k in range(K):
            acc += A[:, k:k + 1] * W[k:k + 1, :]
    assert acc.dtype == np.float32
    if l.scale:
        acc = acc * p["scale"][None, :]
    if l.shift:
        acc = acc + p["shift"][None, :]
    if l.addend:
        acc = acc + p["addend"]
    if l.act == 1:
        acc = np.maximum(acc, np.float32(0))
    if l.act == 2:
        acc[:, :l.act_cols] = (1.0 / (1.0 + np.exp(-acc[:, :l.act_cols].astype(np.float64)))).astype(np.float32)
    assert acc.dtype == np.float32
    return acc


def emulate_pair(name, order):
    cs, d = PAIRS[name], pair_inputs(name)
    b = Buffers()
    for i in range(2):
        key, c0, ld = pair_slot(cs, i)
        b.new(key, grid(cs.shapes[i], cs.layers[i])[2], ld)
        out = _emulate_layer(cs.shapes[i], cs.layers[i], d["x%d" % (i + 1)], d["p%d" % (i + 1)], order).astype(np.float64)
        b.put(key, out, out, out, None, c0)
    return b


def emulate_chain(name, with_next, order):
    """fp32 emulation of the chain: t2 and y passed on as fp32 values, as both device paths do (through LDS or through memory)."""
    cs, d = BNECKS[name], bneck_inputs(name)
    M = cs.shape[0] * cs.shape[1] * cs.shape[2]
    lb, lc, la = cs.layers
    assert lb.ldy == lb.n and (lc.ldy == lc.n or not with_next), "the emulation passes dense intermediates"
    b = Buffers()
    t2 = _emulate_layer(cs.shape, lb, d["x"], d["pb"], order)
    y = _emulate_layer((1, 1, M), lc, t2 if cs.linked else d["x2"], d["pc"], order)
    outs = [("t2", lb, t2), ("y", lc, y)]
    if with_next:
        outs.append(("t", la, _emulate_layer((1, 1, M), la, y, d["pa"], order)))
    for key, l, out in outs:
        b.new(key, M, l.ldy)
        b.put(key, out.astype(np.float64), out, out)
    return b


# ================================================================================================================ tuning-table lines
def single_line(shape, l, tile=(64, 64)):
    """Kind-0 line of one layer's own launch: `kind M N K C npos stride a b slices ms waves`."""
    oh, ow, M, K = grid(shape, l)
    return "0 %d %d %d %d %d %d %d %d 1 0.01 4" % (M, l.n, K, l.c, l.k * l.k, l.stride, tile[0], tile[1])


def pair_line(cs, a, b, slices):
    """Kind 32: N = N1 * 65536 + N2; slices 1 = the paired launch on tile a x b, 2 = the two launches."""
    l1, l2 = cs.layers
    oh, ow, M, K = grid(cs.shapes[0], l1)
    return "32 %d %d %d %d %d %d %d %d %d 0.01 4" % (M, l1.n * 65536 + l2.n, K, l1.c, l1.k * l1.k, l1.stride, a, b, slices)


def bneck_line(cs, with_next, rows, slices, b=64):
    """Kind 33: N = N2 * 65536 + (64 with the trailing reduce), K = 9c, 9 taps, stride 1; slices 1 = fused with `rows` rows per workgroup."""
    lb, lc, la = cs.layers
    M = cs.shape[0] * cs.shape[1] * cs.shape[2]
    return "33 %d %d %d %d 9 1 %d %d %d 0.01 4" % (M, lc.n * 65536 + (64 if with_next else 0), 9 * lb.c, lb.c, rows, b, slices)


TABLE_HEADER = "# radnet tuned GEMM launch shapes v2\n"
