"""radnet_conv_wgrad_multi (csrc/conv_wgrad.hip): the weight gradients of several layers in one launch per tile shape, and Adam in the
tile epilogue.

1. Gradients only: dW and db of every problem are the bits of its own radnet_conv_wgrad call -- same tile, same slices, same slice
   order -- for tables whose problems get different tile shapes (several launches) and for forced 2 and 3 slices, with ordered
   reductions and with atomics.  Atomic sums of three slices depend on the arrival order, in the single launch too: there the two are
   compared to the ordered result within fp32 rounding of a three-term sum instead.
2. With the optimizer block: w, m, v after two steps are the bits of "radnet_conv_wgrad into the zeroed gradient arena, then
   radnet_adam_step", and the gradient arena is never written.
3. radnet_adam_step_tail, the one launch that follows it in a train step, against radnet_adam_step_affine on the arena's tail plus
   radnet_winograd4_filter per 3x3 layer, bit for bit.

"Zero live rows" is read as the engine uses the word: the rows of a problem's dy all belong to an image that takes no classifier step,
i.e. dy is zero there; its gradient is exactly zero in both forms."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_kernels import conv_desc  # noqa: E402

# name, nb, h, w, cin, cout, k, stride, pad
PROBLEMS = [
    ("a", 2, 7, 7, 64, 64, 3, 1, 1),         # M = 98: ragged against the 32-row reduction tile
    ("b", 2, 7, 7, 128, 64, 1, 1, 0),
    ("c", 2, 14, 14, 64, 128, 1, 2, 0),      # the res5a geometry: 14x14 -> 7x7
    ("d", 2, 7, 7, 64, 256, 1, 1, 0),
]
# forced (k tile, n tile, slices) or None: the launch policy's own choice (64x64, 128x64, 64x128, 64x128 here: three launches, no slices)
FORCED = [None, (64, 64, 2), (64, 64, 3), (64, 128, 2)]


@pytest.fixture(scope="module")
def ctx():
    from radnet_hip import lib as L
    c = L.Context(0)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    c.check(c.lib.radnet_set_workspace(c.h, ws.data_ptr(), ws.numel()), "ws")
    c._ws = ws
    yield c
    c.lib.radnet_force_config(c.h, 0, 0, 0)
    c.lib.radnet_set_deterministic(c.h, 1)
    c.close()


@pytest.fixture(scope="module")
def data():
    """Inputs of the four problems, made once: x, two output gradients (step 1 / step 2) and the per-channel factor."""
    out = {}
    for name, nb, h, w, cin, cout, k, stride, pad in PROBLEMS:
        g = torch.Generator().manual_seed(ord(name))
        oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        out[name] = dict(x=torch.randn(nb, h, w, cin, generator=g).cuda(), dy=[torch.randn(nb, oh, ow, cout, generator=g).cuda() for _ in range(2)],
                         gs=(torch.rand(cout, generator=g) + 0.5).cuda(), oh=oh, ow=ow)
    return out


def _desc(L, prob, dat, dy, dw, db, mode=2):
    name, nb, h, w, cin, cout, k, stride, pad = prob
    d = conv_desc(L, dat["x"], dw, dw, nb, h, w, cin, dat["oh"], dat["ow"], k, stride, pad, cout, cout)
    d.dy, d.ld_dy, d.gscale = dy.data_ptr(), cout, dat["gs"].data_ptr()
    d.dw, d.dw_accumulate = dw.data_ptr(), mode
    d.db = db.data_ptr() if db is not None else None
    return d


def _array(L, descs):
    arr = (L.ConvDesc * len(descs))()
    for i, d in enumerate(descs):
        arr[i] = d
    return arr


def _grads(ctx, L, probs, data, multi, step=0, zero_first=False):
    """(dW, db) per problem from the single launches or from one radnet_conv_wgrad_multi call, into zeroed buffers (write mode 2)."""
    outs, descs = [], []
    for i, p in enumerate(probs):
        name, nb, h, w, cin, cout, k = p[:7]
        dy = data[name]["dy"][step]
        if zero_first and i == 0:
            dy = torch.zeros_like(dy)
        dw, db = torch.zeros(k * k * cin, cout, device="cuda"), torch.zeros(cout, device="cuda")
        outs.append((dw, db, dy))
        descs.append(_desc(L, p, data[name], dy, dw, db))
    if multi:
        ctx.check(ctx.lib.radnet_conv_wgrad_multi(ctx.h, _array(L, descs), len(descs), None), "wgrad_multi")
    else:
        for d in descs:
            ctx.check(ctx.lib.radnet_conv_wgrad(ctx.h, C.byref(d)), "wgrad")
    torch.cuda.synchronize()
    return [(dw, db) for dw, db, _ in outs]


def _force(ctx, forced):
    a, b, s = forced if forced is not None else (0, 0, 0)
    ctx.check(ctx.lib.radnet_force_config(ctx.h, a, b, s), "force")


@pytest.mark.parametrize("deterministic", [1, 0])
@pytest.mark.parametrize("forced", FORCED)
def test_multi_launch_matches_the_single_launches_bit_for_bit(ctx, data, forced, deterministic):
    from radnet_hip import lib as L
    ctx.check(ctx.lib.radnet_set_deterministic(ctx.h, deterministic), "deterministic")
    _force(ctx, forced)
    try:
        tables = [(PROBLEMS, False), (PROBLEMS[3:], False), (PROBLEMS, True)]      # four problems; one problem; first problem without live rows
        for probs, zero_first in tables:
            one = _grads(ctx, L, probs, data, False, zero_first=zero_first)
            many = _grads(ctx, L, probs, data, True, zero_first=zero_first)
            for p, (dw1, db1), (dwm, dbm) in zip(probs, one, many):
                if not deterministic and forced is not None and forced[2] > 2:
                    # three atomic partial sums: (a + b) + c in arrival order.  Each ordering is within 2 roundings of the exact sum, at most
                    # 2 * 2^-24 * (|a| + |b| + |c|); |a| + |b| + |c| <= sum_m |x| |dy gs| <= 98 * 5.5 * 5.5 * 1.5 for these inputs
                    tol = 4 * 2.0 ** -24 * 98 * 5.5 * 5.5 * 1.5
                    assert (dw1 - dwm).abs().max().item() <= tol and (db1 - dbm).abs().max().item() <= tol, (p[0], forced)
                else:
                    assert torch.equal(dw1, dwm), (p[0], forced, deterministic)
                    assert torch.equal(db1, dbm), (p[0], forced, deterministic)
            if zero_first:
                assert not many[0][0].any() and not many[0][1].any()
                assert many[1][0].abs().max().item() > 0
    finally:
        _force(ctx, None)
        ctx.lib.radnet_set_deterministic(ctx.h, 1)


LR, B1, B2, EPS, GSCALE = 1e-3, 0.9, 0.999, 1e-7, 0.25


def _arena(probs):
    offs, at = [], 0
    for p in probs:
        offs.append(at)
        at += p[6] * p[6] * p[4] * p[5]
    return offs, at


@pytest.mark.parametrize("forced", FORCED)
def test_epilogue_adam_matches_wgrad_then_adam_bit_for_bit(ctx, data, forced):
    from radnet_hip import lib as L
    offs, n = _arena(PROBLEMS)
    gen = torch.Generator().manual_seed(7)
    p0 = (torch.randn(n, generator=gen) * 0.05).cuda()
    ref = dict(p=p0.clone(), g=torch.zeros(n, device="cuda"), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"))
    new = dict(p=p0.clone(), g=torch.zeros(n, device="cuda"), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"))
    dbs = {k: [torch.zeros(p[5], device="cuda") for p in PROBLEMS] for k in ("ref", "new")}
    _force(ctx, forced)
    try:
        for t in (1, 2):

            def descs(ar, db):
                out = []
                for p, off, b in zip(PROBLEMS, offs, db):
                    k, cin, cout = p[6], p[4], p[5]
                    out.append(_desc(L, p, data[p[0]], data[p[0]]["dy"][t - 1], ar["g"][off:off + k * k * cin * cout].view(k * k * cin, cout), b))
                return out

            for d in descs(ref, dbs["ref"]):
                ctx.check(ctx.lib.radnet_conv_wgrad(ctx.h, C.byref(d)), "wgrad")
            assert ref["g"].abs().max().item() > 0
            ctx.call("radnet_adam_step", ref["p"], ref["g"], ref["m"], ref["v"], C.c_int64(n), t, C.c_float(LR), C.c_float(B1), C.c_float(B2),
                     C.c_float(EPS), C.c_float(GSCALE), 1)
            opt = L.WgradAdam()
            opt.p, opt.g, opt.m, opt.v, opt.n, opt.t = new["p"].data_ptr(), new["g"].data_ptr(), new["m"].data_ptr(), new["v"].data_ptr(), n, t
            opt.lr, opt.beta1, opt.beta2, opt.eps, opt.grad_scale = LR, B1, B2, EPS, GSCALE
            ctx.check(ctx.lib.radnet_conv_wgrad_multi(ctx.h, _array(L, descs(new, dbs["new"])), len(PROBLEMS), C.byref(opt)), "wgrad_multi + adam")
            torch.cuda.synchronize()
            for key in ("p", "m", "v"):
                assert torch.equal(ref[key], new[key]), (key, t, forced)
            assert not new["g"].any(), "the gradient arena was written"
            assert not ref["g"].any()
            for a, b in zip(dbs["ref"], dbs["new"]):
                assert torch.equal(a, b)
        assert not torch.equal(new["p"], p0) and new["v"].abs().max().item() > 0
    finally:
        _force(ctx, None)


def test_epilogue_adam_refuses_what_has_no_final_writer(ctx, data):
    """Slices added with atomics have no last writer, and a gradient that is added to an earlier one is not the whole gradient."""
    from radnet_hip import lib as L
    p = PROBLEMS[1]
    n = p[4] * p[5]
    ar = [torch.zeros(n, device="cuda") for _ in range(4)]
    opt = L.WgradAdam()
    opt.p, opt.g, opt.m, opt.v, opt.n, opt.t = ar[0].data_ptr(), ar[1].data_ptr(), ar[2].data_ptr(), ar[3].data_ptr(), n, 1
    opt.lr, opt.beta1, opt.beta2, opt.eps, opt.grad_scale = LR, B1, B2, EPS, 1.0
    d = _desc(L, p, data[p[0]], data[p[0]]["dy"][0], ar[1].view(p[4], p[5]), None)
    try:
        ctx.check(ctx.lib.radnet_set_deterministic(ctx.h, 0), "deterministic")
        _force(ctx, (64, 64, 2))
        assert ctx.lib.radnet_conv_wgrad_multi(ctx.h, _array(L, [d]), 1, C.byref(opt)) != 0
        ctx.check(ctx.lib.radnet_set_deterministic(ctx.h, 1), "deterministic")
        d.dw_accumulate = 1
        assert ctx.lib.radnet_conv_wgrad_multi(ctx.h, _array(L, [d]), 1, C.byref(opt)) != 0
        outside = torch.zeros(n, device="cuda")
        d.dw_accumulate, d.dw = 2, outside.data_ptr()
        assert ctx.lib.radnet_conv_wgrad_multi(ctx.h, _array(L, [d]), 1, C.byref(opt)) != 0
        torch.cuda.synchronize()
        assert not ar[0].any() and not ar[2].any() and not ar[3].any()
    finally:
        _force(ctx, None)
        ctx.lib.radnet_set_deterministic(ctx.h, 1)


def test_adam_tail_matches_affine_adam_on_the_tail_plus_filter_transforms(ctx):
    """radnet_adam_step_tail (what follows the optimizer epilogue in a train step): Adam over [sweep_from, n) with the folded shifts, and
    the F(4x4,3x3) filters of the listed kernels from the weights as they are -- bit for bit radnet_adam_step_affine on the tail followed
    by radnet_winograd4_filter per layer; nothing in front of sweep_from is touched."""
    from radnet_hip import lib as L
    sizes = [("k1", 64 * 64), ("A", 9 * 64 * 64), ("k2", 64 * 128), ("B", 9 * 64 * 128), ("bias", 256), ("dense", 1024)]
    off, at = {}, 0
    for name, sz in sizes:
        off[name] = at
        at += sz
    n, sweep, nb = at, off["bias"], 256
    gen = torch.Generator().manual_seed(11)
    init = {k: torch.randn(n, generator=gen).cuda() * (0.05 if k != "v" else 1.0) for k in ("p", "g", "m", "v")}
    init["v"] = init["v"].abs() * 1e-3
    scale, t0 = (torch.rand(nb, generator=gen) + 0.5).cuda(), torch.randn(nb, generator=gen).cuda()
    layers = [("A", 64, 64), ("B", 64, 128)]
    scal = (2, C.c_float(LR), C.c_float(B1), C.c_float(B2), C.c_float(EPS), C.c_float(GSCALE), 1)

    ref = {k: v.clone() for k, v in init.items()}
    ref_shift = torch.zeros(nb, device="cuda")
    ctx.call("radnet_adam_step_affine", ref["p"][sweep:], ref["g"][sweep:], ref["m"][sweep:], ref["v"][sweep:], C.c_int64(n - sweep), *scal,
             C.c_int64(0), C.c_int64(nb), scale, t0, ref_shift)
    ref_u = []
    for name, c, k in layers:
        u = torch.full((36, c, k), float("nan"), device="cuda")
        ctx.call("radnet_winograd4_filter", ref["p"][off[name]:], c, k, k, u)
        ref_u.append(u)

    new = {k: v.clone() for k, v in init.items()}
    new_shift = torch.zeros(nb, device="cuda")
    new_u = [torch.full((36, c, k), float("nan"), device="cuda") for _, c, k in layers]
    arr = (L.AdamWino * len(layers))()
    for i, (name, c, k) in enumerate(layers):
        arr[i].off, arr[i].c, arr[i].n, arr[i].u = off[name], c, k, new_u[i].data_ptr()
    ctx.call("radnet_adam_step_tail", new["p"], new["g"], new["m"], new["v"], C.c_int64(n), *scal, C.c_int64(sweep), C.c_int64(nb), scale, t0,
             new_shift, arr, len(layers), C.c_int64(sweep))
    torch.cuda.synchronize()
    for k in ("p", "g", "m", "v"):
        assert torch.equal(ref[k], new[k]), k
        assert torch.equal(new[k][:sweep], init[k][:sweep]), k            # the front of the arena is nobody's in this launch
    assert not new["g"][sweep:].any() and not torch.equal(new["p"][sweep:], init["p"][sweep:])
    assert torch.equal(ref_shift, new_shift) and new_shift.abs().max().item() > 0
    for a, b in zip(ref_u, new_u):
        assert torch.equal(a, b) and not torch.isnan(b).any()
    # refused: a sweep that starts at 0, a layer that reaches past sweep_from, a bias range in front of it
    h = ctx.h
    args = lambda sw, boff: (h, new["p"].data_ptr(), new["g"].data_ptr(), new["m"].data_ptr(), new["v"].data_ptr(), n, 3, LR, B1, B2, EPS, 1.0, 1,
                             boff, nb, scale.data_ptr(), t0.data_ptr(), new_shift.data_ptr(), arr, len(layers), sw)
    assert ctx.lib.radnet_adam_step_tail(*args(0, sweep)) != 0
    assert ctx.lib.radnet_adam_step_tail(*args(off["B"] + 64, sweep)) != 0
    assert ctx.lib.radnet_adam_step_tail(*args(sweep, off["k2"])) != 0
    torch.cuda.synchronize()
    for k in ("p", "m", "v"):
        assert torch.equal(ref[k], new[k]), k
