"""Edge shapes, pitches and epilogue variants of the Winograd path, one STAGE at a time: the ten transform entry points of
csrc/winograd.hip (F(2x2,3x3) and F(4x4,3x3): filter, input, output, dy, filter_grad; the F(4x4) input / output in their six-wave
LDS form and, in a child process, their one-thread form), the 1-D transforms of csrc/radnet_wino4.h behind them, and
radnet_gemm_batched / radnet_wgrad_batched -- against the float64 per-stage references of tests/winograd_edge_cases.py (proved to
compose to the convolution and its gradient, and shown to have teeth, by tests/test_winograd_edge_cases_reference.py).

Every stage of every case and form runs on known signed inputs; input, output and dy (and F(2x2)'s filter and filter_grad) a second
time on integer-valued ones.  After EVERY launch, for EVERY element inside the rows |gpu - ref| <= tol with

  tol = s * 2^-24 * (|L1| |x| |L2|^T * |scale|) + 2 * 2^-24 * (|shift| + |old|)           s: counted in winograd_edge_cases.py

nothing inside the rows is NaN, the integer runs are equal to float64 element for element, and every element outside the rows --
pitch padding (ldw = n + 4, ldy = n + 8), one extra row, 64 floats behind every dense tensor -- still holds the sentinel bits.
Inputs with a pitch (w, dy: ld_dy = n + 12) hold NaN in their padding.  The output stage runs {scale, none} x {shift, none} x
{act 0, 1}, dy with and without gscale, filter_grad with accumulate 0 and 1.  The chained run feeds each stage the device's previous
output (transforms -> batched GEMM -> output; dy -> reduction over tiles -> filter_grad) and checks each against float64 of that one
stage applied to what the device fed it; its end result also passes tolerances.check at the 2e-4 of test_gpu_kernels.py's two
Winograd tests.  The batched GEMMs run every forced launch shape of test_batched_launches_xcd_contiguous_numbering_changes_no_bit
(persistent z forms and slices = -1 included; wgrad_batched with accumulate 0, 1, 2) under (K_red + 8) * 2^-24 * (sum|a*b| + |old|).
The comparison runs on the device; a launch's verdict is five scalars.

Measured on one MI355X, worst err / tol -- F(2x2): filter 0.33, input 0.89 (s_4x4), output 0.41, dy 0.88 (s_7x8, without gscale),
filter_grad 0.40; F(4x4): filter 0.42, input 0.37, output 0.28, dy 0.34, filter_grad 0.38 (all g_9x11); gemm_batched 0.069 alone and
0.064 chained, wgrad_batched 0.092 alone and 0.16 chained (c_2x3, two tiles); the one-thread kernels give the six-wave kernels' bits in
all 39 buffers.  F(2x2)'s input and dy sit close to 1 because their bound has nothing to spare: one rounding per pass, s = 2.  The dy
stage with a gscale measured 1.05 at one element (s_5x7, F(2x2)) under a count that forgot the multiply by gscale, which the
compiler fuses into the first addition; the count was corrected in winograd_edge_cases.py (+ 1 where there is a gscale), see there.
The module takes 5.7 s: 2.2 s the child process, 0.9 s the first case to touch the device, every other test 0.15 s or less.  In
the same run of the whole suite the largest case of test_gpu_kernels.py's test_winograd_conv3x3_vs_oracle took 1.9 s (F(2x2)) and
1.2 s (F(4x4)); the other twelve cases of the two Winograd tests there stayed below 0.62 s each and were not listed singly.

`-s` prints the worst err / tol per case, and per stage and form at the module's end."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import winograd_edge_cases as W  # noqa: E402

S_INT = int(W.SENTINEL)
WORST = {}                   # (stage, form) -> (max err / tol, case, variant)
ERR_ARG, ERR_UNSUPPORTED = -1, -3
V1_RUNS = [("input", None), ("output", (True, True, 1)), ("output", (False, True, 0))]          # what the child process runs, F(4x4)


def _context():
    from radnet_hip import lib as L
    cx = L.Context(0)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    cx.check(cx.lib.radnet_set_workspace(cx.h, ws.data_ptr(), ws.numel()), "set_workspace")
    cx.check(cx.lib.radnet_set_autotune(cx.h, 0), "set_autotune")
    cx._ws = ws
    return cx


@pytest.fixture(scope="module")
def ctx():
    """The module's one context: a 64 MB workspace, autotune off, torch's current stream."""
    cx = _context()
    yield cx
    torch.cuda.synchronize()
    _restore(cx)
    for (stage, form), (ratio, name, var) in sorted(WORST.items(), key=str):
        print("\nwinograd edges: worst err / tol of %s F(%sx%s) = %.4f (%s, %s)" % (stage, form, form, ratio, name, var), end="")
    print()
    cx.close()


def _restore(cx):
    cx.lib.radnet_force_config(cx.h, 0, 0, 0)
    cx.lib.radnet_force_waves(cx.h, 0)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the cached inputs are read-only


class _Output:
    """A stage's output buffer on the device: every element prefilled with the sentinel; reference, bound and the mask of the
    elements inside the rows live on the device, a launch's verdict is five scalars."""

    def __init__(self, res):
        self.inside = _dev(res["inside"])
        self.ref = _dev(np.where(res["inside"], res["buf"], 0.0))
        self.tol = _dev(res["tol"])
        self.size, self.shape = res["buf"].size, res["shape"]

    def fresh(self, old=None):
        buf = torch.full((self.size,), S_INT, dtype=torch.int32, device="cuda").view(torch.float32)
        if old is not None:
            buf[self.inside] = old.reshape(-1)
        return buf

    def judge(self, buf, what, key, exact=False):
        got = buf.double()
        err = torch.where(self.inside, (got - self.ref).abs(), torch.zeros_like(got))
        ok = torch.where(self.inside, err <= self.tol, torch.ones_like(self.inside))
        ratio = torch.where(err > 0, err / self.tol.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        spilled = (buf.view(torch.int32) != S_INT) & ~self.inside
        stats = torch.stack([(~ok).sum().double(), (torch.isnan(got) & self.inside).sum().double(), spilled.sum().double(), ratio.max(),
                             ((got != self.ref) & self.inside).sum().double()]).tolist()
        bad, nans, lost, worst, unequal = int(stats[0]), int(stats[1]), int(stats[2]), stats[3], int(stats[4])
        if worst > WORST.get(key, (-1.0,))[0]:
            WORST[key] = (worst, what[0], what[1:])
        assert nans == 0, (what, "%d NaN inside the rows" % nans)
        assert lost == 0, (what, "%d elements outside the rows lost their sentinel" % lost, torch.nonzero(spilled)[:4].tolist())
        assert bad == 0, (what, "%d elements outside the bound, worst err / tol %.3f at flat index %d" % (bad, worst, int(ratio.argmax())))
        if exact:
            assert unequal == 0, (what, "%d elements of an integer-valued run differ from float64" % unequal)
        return worst


def _fn(form, stage):
    return ("radnet_winograd4_" if form == 4 else "radnet_winograd_") + stage


class _Case:
    """One case and form on the device: inputs laid out with the case's pitches (NaN in every padding)."""

    def __init__(self, name, form, ints=False):
        self.name, self.form, self.ints = name, form, ints
        self.cs, self.p, self.g = W.CASES[name], W.pitches(W.CASES[name]), W.geometry(W.CASES[name], form)
        d = self.d = W.inputs(name, form, ints)
        self.w, self.x, self.m = _dev(W.padded(d["w"], self.p["ldw"])), _dev(d["x"]), _dev(d["m"])
        self.dy, self.du, self.dw0 = _dev(W.padded(d["dy"], self.p["ld_dy"])), _dev(d["du"]), _dev(d["dw0"])
        self.scale, self.shift, self.gscale = _dev(d["scale"]), _dev(d["shift"]), _dev(d["gscale"])

    def launch(self, cx, stage, var, out, src=None):
        """One launch of `stage` into a fresh buffer of `out`; src: the device tensor to read instead of the case's own input."""
        cs, p = self.cs, self.p
        buf = out.fresh(self.dw0 if stage == "filter_grad" and var else None)
        if stage == "filter":
            cx.call(_fn(self.form, stage), self.w, cs.c, cs.n, p["ldw"], buf)
        elif stage == "input":
            cx.call(_fn(self.form, stage), self.x, cs.nb, cs.h, cs.w, cs.c, buf)
        elif stage == "output":
            cx.call(_fn(self.form, stage), self.m if src is None else src, cs.nb, cs.h, cs.w, cs.n, self.scale if var[0] else None,
                    self.shift if var[1] else None, var[2], buf, p["ldy"])
        elif stage == "dy":
            cx.call(_fn(self.form, stage), self.dy, cs.nb, cs.h, cs.w, cs.n, p["ld_dy"], self.gscale if var else None, buf)
        else:
            cx.call(_fn(self.form, stage), self.du if src is None else src, cs.c, cs.n, p["ldw"], buf, int(var))
        return buf

    def run(self, cx, stage, var):
        out = _Output(W.compute(self.name, self.form, stage, var, self.ints))
        exact = self.ints and stage in W.EXACT[self.form]
        return out.judge(self.launch(cx, stage, var, out), (self.name, stage, var, "ints" if self.ints else "real"), (stage, self.form), exact)


ALL = [(name, form) for name in W.CASES for form in W.FORMS]


@pytest.mark.parametrize("name,form", ALL)
def test_every_stage_alone(ctx, name, form):
    worst, launches = {}, 0
    for ints in (False, True):
        pr = _Case(name, form, ints)
        for stage in W.STAGES:
            if ints and stage not in W.EXACT[form]:
                continue
            for var in W.variants(stage):
                worst[stage] = max(worst.get(stage, 0.0), pr.run(ctx, stage, var))
                launches += 1
    print("%s F(%dx%d): %d launches, worst err / tol %s" % (name, form, form, launches, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert launches == 14 + (11 if form == 4 else 14)


def _host(buf, out):
    """The inside of a device buffer as the float32 array of the stage's shape."""
    return buf[out.inside].cpu().numpy().reshape(out.shape if len(out.shape) == 3 else (out.shape[0] - 1, -1))


CHAINED = [(name, form) for name, form in ALL if W.CASES[name].chain]


@pytest.mark.parametrize("name,form", CHAINED)
def test_chained_stages_on_the_device_s_own_outputs(ctx, name, form):
    from oracle import dense
    from tolerances import check
    cs, pr = W.CASES[name], _Case(name, form)
    p, g, d = pr.p, pr.g, pr.d
    what = lambda s: (name, s, "chained")
    uo, vo = _Output(W.compute(name, form, "filter")), _Output(W.compute(name, form, "input"))
    u, v = pr.launch(ctx, "filter", None, uo), pr.launch(ctx, "input", None, vo)
    uo.judge(u, what("filter"), ("filter", form))
    vo.judge(v, what("input"), ("input", form))
    uh, vh = _host(u, uo), _host(v, vo)
    # forward: the batched GEMM on the device's u and v, the output transform on the device's m
    mo = _Output(W.ref_gemm(vh, uh))
    m = mo.fresh()
    ctx.call("radnet_gemm_batched", v, u, m, g["P"], g["T"], cs.n, cs.c)
    mo.judge(m, what("gemm_batched"), ("gemm_batched", "chain %d" % form))
    yo = _Output(W.stage_output(_host(m, mo), cs.nb, cs.h, cs.w, cs.n, p["ldy"], form, d["scale"], d["shift"], 1))
    y = pr.launch(ctx, "output", (True, True, 1), yo, m)
    yo.judge(y, what("output"), ("output", form))
    x64, w64 = d["x"].astype(np.float64), d["w"].astype(np.float64).reshape(3, 3, cs.c, cs.n)
    ref = np.maximum(dense.conv2d(x64, w64, None, 1, (1, 1, 1, 1)).reshape(-1, cs.n) * d["scale"].astype(np.float64) + d["shift"], 0)
    check(_host(y, yo), ref, 2e-4, "winograd F(%dx%d) %s" % (form, form, name))
    if "g" not in cs.chain:
        return
    # gradient: dy -> reduction over tiles on the device's v and dz -> filter_grad on the device's du, then once more into the result
    zo = _Output(W.compute(name, form, "dy", True))
    dz = pr.launch(ctx, "dy", True, zo)
    zo.judge(dz, what("dy"), ("dy", form))
    zh = _host(dz, zo)
    do = _Output(W.ref_wgrad(vh, zh))
    du = do.fresh()
    ctx.call("radnet_wgrad_batched", v, dz, du, g["P"], g["T"], cs.c, cs.n, 0)
    do.judge(du, what("wgrad_batched"), ("wgrad_batched", "chain %d" % form))
    duh = _host(du, do)
    go = _Output(W.stage_filter_grad(duh, cs.c, cs.n, p["ldw"], form))
    dw = pr.launch(ctx, "filter_grad", 0, go, du)
    go.judge(dw, what("filter_grad"), ("filter_grad", form))
    gm = (d["dy"] * d["gscale"][None, :]).astype(np.float64).reshape(cs.nb, cs.h, cs.w, cs.n)
    _, dw_ref, _ = dense.conv2d_bwd(x64, np.zeros_like(w64), gm, 1, (1, 1, 1, 1), need_dx=False)
    check(_host(dw, go), dw_ref.reshape(9 * cs.c, cs.n), 2e-4, "winograd wgrad F(%dx%d) %s" % (form, form, name))
    ga = _Output(W.stage_filter_grad(duh, cs.c, cs.n, p["ldw"], form, d["dw0"]))
    ga.judge(pr.launch(ctx, "filter_grad", 1, ga, du), what("filter_grad +="), ("filter_grad", form))


@pytest.mark.parametrize("shape", W.BATCHED)
def test_batched_gemms_every_forced_launch_shape(ctx, shape):
    batch, T, c, n = shape
    rs = np.random.RandomState(sum(shape))
    vh, uh, zh = (rs.standard_normal(s).astype(np.float32) for s in ((batch, T, c), (batch, c, n), (batch, T, n)))
    oldh = rs.standard_normal((batch, c, n)).astype(np.float32)
    v, u, dz, old = _dev(vh), _dev(uh), _dev(zh), _dev(oldh)
    mo = _Output(W.ref_gemm(vh, uh))
    ran, worst = 0, 0.0
    try:
        m = mo.fresh()
        ctx.call("radnet_gemm_batched", v, u, m, batch, T, n, c)                       # nothing forced
        worst = mo.judge(m, (shape, "cost model"), ("gemm_batched", "alone"))
        for bm, bn, s, wv in W.gemm_shapes(batch, n):
            ctx.check(ctx.lib.radnet_force_config(ctx.h, bm, bn, s), "force_config")
            ctx.check(ctx.lib.radnet_force_waves(ctx.h, wv), "force_waves")
            m = mo.fresh()
            ctx.call("radnet_gemm_batched", v, u, m, batch, T, n, c)
            worst = max(worst, mo.judge(m, (shape, bm, bn, s, wv), ("gemm_batched", "alone")))
            ran += 1
        _restore(ctx)
        if c % 64:
            du = torch.full((batch * c * n,), S_INT, dtype=torch.int32, device="cuda")
            rc = ctx.lib.radnet_wgrad_batched(ctx.h, v.data_ptr(), dz.data_ptr(), du.data_ptr(), batch, T, c, n, 0)
            assert rc == ERR_UNSUPPORTED and bool((du == S_INT).all()), ("wgrad_batched takes c % 64 == 0 only", shape, rc)
        else:
            outs = {0: _Output(W.ref_wgrad(vh, zh)), 1: _Output(W.ref_wgrad(vh, zh, oldh))}
            outs[2] = outs[0]
            for bmk, bn, s in [(None, None, None)] + W.wgrad_shapes(c, n):
                if bmk is not None:
                    ctx.check(ctx.lib.radnet_force_config(ctx.h, bmk, bn, s), "force_config")
                for acc in (0, 1, 2):
                    du = outs[acc].fresh(None if acc == 0 else old if acc == 1 else torch.zeros_like(old))
                    ctx.call("radnet_wgrad_batched", v, dz, du, batch, T, c, n, acc)
                    worst = max(worst, outs[acc].judge(du, (shape, bmk, bn, s, "accumulate %d" % acc), ("wgrad_batched", "alone")))
                    ran += 1
    finally:
        _restore(ctx)
    print("%s: %d forced launches (+ the cost model's), worst err / tol %.4f" % (shape, ran, worst))
    assert ran >= len(W.gemm_shapes(batch, n)) + (0 if c % 64 else 3 * (1 + len(W.wgrad_shapes(c, n))) - 3)


def test_refusals_launch_nothing(ctx):
    """n % 4, c % 4, ldy < n, ld_dy % 4, ldw % 4 (and ld_dy < n, ldy % 4): RADNET_ERR_ARG with a message, no output element touched."""
    zeros = torch.zeros(1 << 16, device="cuda")
    out = torch.full((1 << 16,), S_INT, dtype=torch.int32, device="cuda")
    z, o, lib, h = zeros.data_ptr(), out.data_ptr(), ctx.lib, ctx.h
    ran = 0
    for form in W.FORMS:
        f = lambda stage: getattr(lib, _fn(form, stage))
        refused = [
            ("filter, n % 4", f("filter")(h, z, 8, 6, 8, o)),
            ("filter, ldw % 4", f("filter")(h, z, 8, 8, 10, o)),
            ("input, c % 4", f("input")(h, z, 2, 5, 7, 6, o)),
            ("output, n % 4", f("output")(h, z, 2, 5, 7, 6, z, z, 1, o, 8)),
            ("output, ldy < n", f("output")(h, z, 2, 5, 7, 8, z, z, 1, o, 4)),
            ("output, ldy % 4", f("output")(h, z, 2, 5, 7, 8, z, z, 1, o, 10)),
            ("dy, n % 4", f("dy")(h, z, 2, 5, 7, 6, 8, z, o)),
            ("dy, ld_dy % 4", f("dy")(h, z, 2, 5, 7, 8, 10, z, o)),
            ("dy, ld_dy < n", f("dy")(h, z, 2, 5, 7, 8, 4, z, o)),
            ("filter_grad, n % 4", f("filter_grad")(h, z, 8, 6, 8, o, 0)),
            ("filter_grad, ldw % 4", f("filter_grad")(h, z, 8, 8, 10, o, 1)),
        ]
        for what, rc in refused:
            assert rc == ERR_ARG, (form, what, rc)
            msg = lib.radnet_last_error(h)
            assert msg and len(msg) > 0, (form, what)
            ran += 1
    torch.cuda.synchronize()
    assert ran == 22 and bool((out == S_INT).all()), "a refused call wrote to its output"
    _Case("s_1x1", 4).run(ctx, "input", None)                     # the context still works


def _v1_buffers(cx):
    """{case__run: the full output buffer's bits} of the F(4x4) input stage and two output epilogues of every case."""
    bufs = {}
    for name in W.CASES:
        pr = _Case(name, 4)
        for i, (stage, var) in enumerate(V1_RUNS):
            out = _Output(W.compute(name, 4, stage, var))
            bufs["%s__%d" % (name, i)] = pr.launch(cx, stage, var, out).view(torch.int32).cpu().numpy()
    return bufs


def test_one_thread_kernels_give_the_six_wave_kernels_bits(ctx, tmp_path):
    """RADNET_WINO_V1 is read once per process: a fresh child computes v and y of the F(4x4) cases with the one-thread kernels.  Both
    forms satisfy the bounds and keep the sentinels; csrc/winograd.hip says they give the same bits."""
    path = str(tmp_path / "v1.npz")
    env = dict(os.environ, RADNET_WINO_V1="1")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    v1 = np.load(path)
    v2 = _v1_buffers(ctx)
    assert set(v1.files) == set(v2) and len(v2) == 3 * len(W.CASES)
    differ = []
    for key in sorted(v2):
        name, (stage, var) = key.split("__")[0], V1_RUNS[int(key.split("__")[1])]
        out = _Output(W.compute(name, 4, stage, var))
        for which, bits in (("one-thread", v1[key]), ("six-wave", v2[key])):
            out.judge(torch.from_numpy(bits.copy()).cuda().view(torch.float32), (name, stage, var, which), (stage + " " + which, 4))
        if not np.array_equal(v1[key], v2[key]):
            differ.append(key)
    print("one-thread against six-wave kernels: %d of %d buffers differ in bits %s" % (len(differ), len(v2), differ[:6]))
    assert not differ, differ


if __name__ == "__main__":          # the child of test_one_thread_kernels_give_the_six_wave_kernels_bits
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "rock-art-radnet_amd")):
        sys.path.insert(0, _p)
    assert os.environ.get("RADNET_WINO_V1") == "1"
    _cx = _context()
    _bufs = _v1_buffers(_cx)
    torch.cuda.synchronize()
    _cx.close()
    np.savez(sys.argv[1], **_bufs)
