"""Edge shapes, pitches and forced launch shapes of the fp32 implicit-GEMM convolutions (radnet_conv_fwd / _dgrad / _wgrad / _bwd:
csrc/conv_mfma.hip, csrc/conv_wgrad.hip, conv_igemm_body.h, conv_wgrad_body.h) against the full-output float64 references of
tests/fp32_edge_cases.py (proved against the oracle, and shown to have teeth, by tests/test_fp32_edge_cases_reference.py).

Every case runs the cost model's launch shape and then every forced one: output tiles 64x64, 128x128, 128x64, 64x128 with 4 and 8
waves, 32x64 and 32x32 with 4; slices {1, -1} and the case's named splits with both signs; the weight gradient tiles {64, 128}^2 with
splits {1, 2, 3, 8}, in every dw_accumulate mode of the case.  After EVERY launch, for EVERY output element |gpu - ref| <= tol with

  tol = (K_red + 8) * 2^-24 * (sum|a*b| * |scale| + |shift| + |addend|)

(the worst case of an fp32 sum of K_red products in any order; see fp32_edge_cases.py), nothing inside the rows is NaN, and every
element outside them -- the pitch padding, one extra row, the left half of f_col_block's wider tensor -- still holds the sentinel
bits it was prefilled with.  Input pitches differ from the output's and from each other and hold NaN in their padding.  The split
cases run with ordered and with atomic reductions; ordered, two runs of a shape give the same bits.  radnet_conv_bwd gives the bits
of radnet_conv_wgrad followed by radnet_conv_dgrad.  The comparison runs on the device; four scalars come back per launch.

Measured on one MI355X: worst err / tol 0.085 forward (f_col_block), 0.063 dgrad (d_ragged), 0.147 wgrad and 0.092 db (w_m1: one
term added to the old value), 0.003 and below for the deep reductions; the module takes 3.3 s, its slowest case (f_ragged_mn, the
first to touch the device) 0.6 s, every other one below 0.15 s.

`-s` prints the launch shapes run and the worst err / tol per case, and a summary per kind at the module's end."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fp32_edge_cases as F  # noqa: E402

S_INT = int(F.SENTINEL)
WORST = {}                   # kind -> (max err / tol, case, launch shape)
SIGMOID_WORST = [0.0]        # max |gpu - ref| over the sigmoid columns


@pytest.fixture(scope="module")
def ctx():
    """The module's one context: a 256 MB workspace, autotune off, torch's current stream."""
    from radnet_hip import lib as L
    cx = L.Context(0)
    ws = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    cx.check(cx.lib.radnet_set_workspace(cx.h, ws.data_ptr(), ws.numel()), "set_workspace")
    cx.check(cx.lib.radnet_set_autotune(cx.h, 0), "set_autotune")
    cx._ws = ws
    cx._det = cx.lib.radnet_get_deterministic(cx.h)
    yield cx
    torch.cuda.synchronize()
    _restore(cx)
    for kind, (ratio, name, shape) in sorted(WORST.items()):
        print("\nfp32 edges: worst err / tol of %s = %.4f (%s, %s)" % (kind, ratio, name, shape), end="")
    print("\nfp32 edges: worst |gpu - ref| of a sigmoid column = %.3g = %.3f * 2^-22" % (SIGMOID_WORST[0], SIGMOID_WORST[0] * 2.0 ** 22))
    cx.close()


def _restore(cx):
    cx.lib.radnet_force_config(cx.h, 0, 0, 0)
    cx.lib.radnet_force_waves(cx.h, 0)
    cx.lib.radnet_set_deterministic(cx.h, cx._det)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the cached inputs are read-only


def _ptr(t):
    return None if t is None else t.data_ptr()


class _Output:
    """An output of a case on the device: [rows + 1][ld] fp32 prefilled with the sentinel, the result in [rows) x [c0, c0 + cols);
    the reference and the bound live on the device once, a launch's verdict is four scalars."""

    def __init__(self, ref, tol, ld, c0=0):
        self.rows, self.cols, self.ld, self.c0 = ref.shape[0], ref.shape[1], ld, c0
        self.ref, self.tol = _dev(np.ascontiguousarray(ref)), _dev(np.ascontiguousarray(tol))
        outside = np.ones((self.rows + 1, ld), bool)
        outside[:self.rows, c0:c0 + self.cols] = False
        self.outside = _dev(outside)

    def fresh(self, inside=None):
        buf = torch.full((self.rows + 1, self.ld), S_INT, dtype=torch.int32, device="cuda").view(torch.float32)
        if inside is not None:
            buf[:self.rows, self.c0:self.c0 + self.cols] = inside
        return buf

    def ptr(self, buf):
        return buf.data_ptr() + 4 * self.c0

    def judge(self, buf, what, kind):
        got = buf[:self.rows, self.c0:self.c0 + self.cols].double()
        err = (got - self.ref).abs()
        ratio = torch.nan_to_num(err / self.tol.clamp_min(1e-300), nan=float("inf"))
        stats = torch.stack([(~(err <= self.tol)).sum().double(), torch.isnan(got).sum().double(),
                             ((buf.view(torch.int32) != S_INT) & self.outside).sum().double(), ratio.max()]).tolist()
        bad, nans, spilled, worst = int(stats[0]), int(stats[1]), int(stats[2]), stats[3]
        if worst > WORST.get(kind, (-1.0,))[0]:
            WORST[kind] = (worst, what[0], what[1:])
        assert nans == 0, (what, "%d NaN inside the rows" % nans)
        assert spilled == 0, (what, "%d elements outside the rows lost their sentinel" % spilled,
                              torch.nonzero((buf.view(torch.int32) != S_INT) & self.outside)[:4].tolist())
        assert bad == 0, (what, "%d elements outside the bound, worst err / tol %.3f at %s" % (
            bad, worst, np.unravel_index(int(ratio.argmax()), (self.rows, self.cols))))
        return worst


class _Problem:
    """One case on the device: inputs laid out with the case's pitches (NaN in every padding), one _Output per result."""

    def __init__(self, name):
        from radnet_hip import lib as L
        self.L, self.name, self.cs = L, name, F.CASES[name]
        cs, d, p = self.cs, F.inputs(name), F.pitches(F.CASES[name])
        self.g, self.p, self.d = F.geometry(cs), p, d
        self.w = _dev(F.padded(d["w"], p["ldw"]))
        self.x = _dev(d.get("x"))
        self.out, self.db = {}, {}
        if cs.kind == "fwd":
            self.scale, self.shift, self.addend = _dev(d["scale"]), _dev(d["shift"]), _dev(F.padded(d["addend"], p["ld_add"]))
            r = F.compute(name)
            self.out["fwd", 0] = _Output(r["out"], r["tol"], p["ldy"], cs.n if cs.opts.get("col_block") else 0)
        else:
            self.dy, self.gscale = _dev(F.padded(d["dy"], p["ld_dy"])), _dev(d["gscale"])
        if "dgrad" in F.sides(cs):
            self.add = _dev(F.padded(d["dx_add"], p["ld_dx_add"])) if d["dx_add"] is not None else None
            self.mask = _dev(F.padded(d["dx_mask"], p["ld_dx_mask"])) if d["dx_mask"] is not None else None
            r = F.compute(name, "dgrad")
            self.out["dgrad", 0] = _Output(r["out"], r["tol"], p["ld_dx"])
        if "wgrad" in F.sides(cs):
            for mode in cs.opts["modes"]:
                r = F.compute(name, "wgrad", mode)
                self.out["wgrad", mode] = _Output(r["out"], r["tol"], p["ldw"])
                self.db[mode] = _Output(r["db"][None, :], r["db_tol"][None, :], cs.n + 8) if cs.opts.get("db") else None
            self.dw0, self.db0 = _dev(d["dw0"]), _dev(d["db0"][None, :])

    def desc(self):
        cs, g, p = self.cs, self.g, self.p
        d = self.L.ConvDesc()
        d.nb, d.h, d.w_, d.c, d.oh, d.ow, d.kh, d.kw = cs.nb, cs.h, cs.w, cs.c, g["oh"], g["ow"], cs.kh, cs.kw
        d.stride, d.pad_t, d.pad_l, d.n = cs.stride, cs.pad[0], cs.pad[1], cs.n
        d.x, d.w, d.ldw = _ptr(self.x), _ptr(self.w), p["ldw"]
        if cs.kind == "fwd":
            d.scale, d.shift, d.addend = _ptr(self.scale), _ptr(self.shift), _ptr(self.addend)
            d.ldy, d.ld_add, d.act, d.act_cols = p["ldy"], p["ld_add"], cs.opts.get("act", 0), cs.opts.get("act_cols", 0)
        else:
            d.dy, d.ld_dy, d.gscale = _ptr(self.dy), p["ld_dy"], _ptr(self.gscale)
        if "dgrad" in F.sides(cs):
            d.dx_add, d.dx_mask = _ptr(self.add), _ptr(self.mask)
            d.ld_dx, d.ld_dx_add, d.ld_dx_mask = p["ld_dx"], p["ld_dx_add"], p["ld_dx_mask"]
        return d

    # ---- one launch each: the buffers come back for the verdict
    def fwd(self, cx):
        o, d = self.out["fwd", 0], self.desc()
        buf = o.fresh()
        d.y = o.ptr(buf)
        cx.check(cx.lib.radnet_conv_fwd(cx.h, C.byref(d)), self.name)
        return buf

    def _wgrad_buffers(self, d, mode):
        o, ob = self.out["wgrad", mode], self.db[mode]
        dw = o.fresh(None if mode == 0 else self.dw0 if mode == 1 else 0.0)
        db = None if ob is None else ob.fresh(None if mode == 0 else self.db0 if mode == 1 else 0.0)
        d.dw, d.dw_accumulate, d.db = dw.data_ptr(), mode, _ptr(db)
        return dw, db

    def dgrad(self, cx):
        o, d = self.out["dgrad", 0], self.desc()
        dx = o.fresh()
        d.dx = dx.data_ptr()
        cx.check(cx.lib.radnet_conv_dgrad(cx.h, C.byref(d)), self.name)
        return dx

    def wgrad(self, cx, mode):
        d = self.desc()
        dw, db = self._wgrad_buffers(d, mode)
        cx.check(cx.lib.radnet_conv_wgrad(cx.h, C.byref(d)), self.name)
        return dw, db

    def two_calls(self, cx, mode):
        d = self.desc()
        dw, db = self._wgrad_buffers(d, mode)
        dx = self.out["dgrad", 0].fresh()
        d.dx = dx.data_ptr()
        cx.check(cx.lib.radnet_conv_wgrad(cx.h, C.byref(d)), self.name)
        cx.check(cx.lib.radnet_conv_dgrad(cx.h, C.byref(d)), self.name)
        return dw, db, dx

    def bwd(self, cx, mode):
        d = self.desc()
        dw, db = self._wgrad_buffers(d, mode)
        dx = self.out["dgrad", 0].fresh()
        d.dx = dx.data_ptr()
        cx.check(cx.lib.radnet_conv_bwd(cx.h, C.byref(d)), self.name)
        return dw, db, dx

    def judge_wgrad(self, dw, db, mode, what):
        worst = self.out["wgrad", mode].judge(dw, what, "wgrad")
        if db is not None:
            self.db[mode].judge(db, what, "db")
        return worst


def _same_bits(a, b):
    return a is b or torch.equal(a.view(torch.int32), b.view(torch.int32))


def _force(cx, bm, bn, s, wv=0):
    cx.check(cx.lib.radnet_force_config(cx.h, bm, bn, s), "force_config")
    cx.check(cx.lib.radnet_force_waves(cx.h, wv), "force_waves")


def _sigmoid_distance(pr, buf):
    cs = pr.cs
    if cs.opts.get("act") == 2:
        o = pr.out["fwd", 0]
        ac = cs.opts["act_cols"]
        SIGMOID_WORST[0] = max(SIGMOID_WORST[0], float((buf[:o.rows, :ac].double() - o.ref[:, :ac]).abs().max()))


IGEMM = [n for n, cs in F.CASES.items() if cs.kind in ("fwd", "dgrad")]
WGRAD = [n for n, cs in F.CASES.items() if cs.kind == "wgrad"]
BWD = [n for n, cs in F.CASES.items() if cs.kind == "bwd"]


@pytest.mark.parametrize("name", IGEMM)
def test_forward_and_dgrad_case_every_launch_shape(ctx, name):
    cs = F.CASES[name]
    side = cs.kind
    pr = _Problem(name)
    run = pr.fwd if side == "fwd" else pr.dgrad
    o = pr.out[side, 0]
    shapes, left = F.igemm_shapes(cs, side)
    ran, worst = 0, 0.0
    try:
        buf = run(ctx)                                             # nothing forced: the cost model's choice
        worst = o.judge(buf, (name, "cost model"), side)
        _sigmoid_distance(pr, buf)
        for det in ((1, 0) if cs.splits else (1,)):                # the split cases: ordered and atomic reductions
            ctx.check(ctx.lib.radnet_set_deterministic(ctx.h, det), "set_deterministic")
            for bm, bn, s, wv in shapes:
                _force(ctx, bm, bn, s, wv)
                buf = run(ctx)
                worst = max(worst, o.judge(buf, (name, bm, bn, s, wv, "det %d" % det), side))
                _sigmoid_distance(pr, buf)
                if det == 1:
                    ran += 1
                    if cs.splits:
                        assert _same_bits(buf, run(ctx)), ("two runs differ", name, bm, bn, s, wv)
    finally:
        _restore(ctx)
    print("%s: %d forced launch shapes (+ the cost model's), %d left out by a launcher rule, worst err / tol %.4f" % (name, ran, left, worst))
    assert ran == len(shapes) and ran >= (8 if cs.c == 4 else 10) * (2 + 2 * len(cs.splits))


@pytest.mark.parametrize("name", WGRAD)
def test_wgrad_case_every_launch_shape_and_mode(ctx, name):
    cs = F.CASES[name]
    pr = _Problem(name)
    shapes, left = F.wgrad_shapes(cs)
    ran, worst = 0, 0.0
    try:
        for mode in cs.opts["modes"]:
            dw, db = pr.wgrad(ctx, mode)                           # nothing forced
            worst = max(worst, pr.judge_wgrad(dw, db, mode, (name, "cost model", "mode %d" % mode)))
            for det in ((1, 0) if cs.splits else (1,)):
                ctx.check(ctx.lib.radnet_set_deterministic(ctx.h, det), "set_deterministic")
                for bmk, bn, s in shapes:
                    _force(ctx, bmk, bn, s)
                    dw, db = pr.wgrad(ctx, mode)
                    worst = max(worst, pr.judge_wgrad(dw, db, mode, (name, bmk, bn, s, "mode %d" % mode, "det %d" % det)))
                    if det == 1:
                        ran += 1
                        if cs.splits:
                            dw2, db2 = pr.wgrad(ctx, mode)
                            assert _same_bits(dw, dw2) and _same_bits(db, db2), ("two runs differ", name, bmk, bn, s, mode)
            _restore(ctx)
    finally:
        _restore(ctx)
    print("%s: %d forced launch shapes x modes (+ the cost model's), %d left out (c %% bmk, splits > tiles), worst err / tol %.4f" % (
        name, ran, left, worst))
    tiles = 4 if cs.c % 128 == 0 else 2
    assert ran == len(shapes) * len(cs.opts["modes"]) and len(shapes) >= tiles * (1 + len(cs.splits))


# conv_bwd: one launch when both problems run as 64- or 32-row x 64-column, 4-wave workgroups, the two calls otherwise -- both forms
# are forced here.  c = 64: a forced k tile of 128 is refused by the weight gradient, so the 128-row tiles are not in the list.
BWD_SHAPES = [(64, 64, 4), (32, 64, 4), (32, 32, 4), (64, 128, 4), (64, 64, 8), (64, 128, 8)]


@pytest.mark.parametrize("name", BWD)
def test_conv_bwd_is_the_two_calls_bit_for_bit(ctx, name):
    cs = F.CASES[name]
    pr = _Problem(name)
    ran = 0
    try:
        for mode in cs.opts["modes"]:
            for s in [1, -1] + [v * sg for v in cs.splits for sg in (1, -1)]:
                for bm, bn, wv in BWD_SHAPES:
                    _force(ctx, bm, bn, s, wv)
                    what = (name, bm, bn, s, wv, "mode %d" % mode)
                    dw_a, db_a, dx_a = pr.two_calls(ctx, mode)
                    dw_b, db_b, dx_b = pr.bwd(ctx, mode)
                    for dw, db, dx in ((dw_a, db_a, dx_a), (dw_b, db_b, dx_b)):
                        pr.judge_wgrad(dw, db, mode, what)
                        pr.out["dgrad", 0].judge(dx, what, "dgrad")
                    assert _same_bits(dw_a, dw_b) and _same_bits(db_a, db_b) and _same_bits(dx_a, dx_b), ("conv_bwd is not the two calls", what)
                    ran += 1
    finally:
        _restore(ctx)
    print("%s: %d forced launch shapes x modes" % (name, ran))
    assert ran == len(cs.opts["modes"]) * (2 + 2 * len(cs.splits)) * len(BWD_SHAPES)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(ctx):
    """What the launchers do not take comes back as an error code with a message, and no output element is touched."""
    from radnet_hip import lib as L
    zeros = torch.zeros(1 << 20, device="cuda")                    # every input pointer: large enough for any of the shapes below
    out = torch.full((1 << 20,), S_INT, dtype=torch.int32, device="cuda")

    def desc(nb=2, h=9, w=11, c=32, k=3, pad=1, n=36, **over):
        d = L.ConvDesc()
        d.nb, d.h, d.w_, d.c, d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.n = nb, h, w, c, k, k, 1, pad, pad, n
        d.oh, d.ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
        d.x = d.w = d.scale = d.shift = d.addend = d.dy = d.gscale = d.dx_add = d.dx_mask = zeros.data_ptr()
        d.y = d.dx = d.dw = d.db = out.data_ptr()
        d.ldw, d.ldy, d.ld_add, d.ld_dy, d.ld_dx, d.ld_dx_add, d.ld_dx_mask = n + 4, n + 8, n + 12, n, c + 4, c + 8, c + 12
        for key, v in over.items():
            setattr(d, key, v)
        return d

    lib = ctx.lib
    refused = [
        ("6x6 kernel, c = 32: 36 taps", lib.radnet_conv_fwd, desc(k=6, pad=0), -3),      # RADNET_ERR_UNSUPPORTED; -1: RADNET_ERR_ARG
        ("ld_add < n", lib.radnet_conv_fwd, desc(ld_add=32), -1),
        ("dgrad, ld_dy != n", lib.radnet_conv_dgrad, desc(n=32, ld_dy=40), -1),
        ("dgrad, n % 32 != 0", lib.radnet_conv_dgrad, desc(n=36), -3),
        ("wgrad, c = 32", lib.radnet_conv_wgrad, desc(c=32), -3),
        ("wgrad, ld_dy % 4 != 0", lib.radnet_conv_wgrad, desc(c=64, ld_dy=39), -1),
        ("wgrad, ldw % 4 != 0", lib.radnet_conv_wgrad, desc(c=64, ldw=39), -1),
        ("fwd, ldw % 4 != 0", lib.radnet_conv_fwd, desc(ldw=39), -1),
    ]
    for what, fn, d, code in refused:
        rc = fn(ctx.h, C.byref(d))
        msg = lib.radnet_last_error(ctx.h)
        assert rc == code, (what, rc)
        assert msg and len(msg) > 0, what
    torch.cuda.synchronize()
    assert bool((out == S_INT).all()), "a refused call wrote to its output"
    # the context still works
    pr = _Problem("f_m1_n4")
    pr.out["fwd", 0].judge(pr.fwd(ctx), ("f_m1_n4", "after the refusals"), "fwd")
