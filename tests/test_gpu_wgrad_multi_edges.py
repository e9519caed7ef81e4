"""radnet_conv_wgrad_multi (csrc/conv_wgrad.hip: conv_wgrad_multi_kernel, wgrad_multi_plan, the cached device tables), its Adam epilogue
(conv_wgrad_body.h, OPT = true) and radnet_adam_step_tail (csrc/adam.hip) against float64, at the tables, arenas and tail layouts of
tests/wgrad_multi_cases.py (checked on the CPU, and shown to have teeth, by tests/test_wgrad_multi_cases_reference.py).

1. Gradients only.  Every table is ONE call on a context of its own (its workspace, its loaded tuning-table lines, no autotuning) with
   ordered reductions, all_default also with atomics.  Every element of every problem's dw and db lies inside the fp32 suite's bound
   (M + 8) 2^-24 sum|a b| (+ the old value in mode 1) of the float64 result; every pad column and the 64 floats behind each buffer keep the
   sentinel bits; the call's launch count (timing class 2) is the one the CPU model of the plan predicts; a second call gives the same bits.
2. Optimizer block.  g_dev = the gradient of a gradients-only call on the same context.  p, m, v over the WHOLE arena: the elements
   (k < K, j < n) of every block within update_edge_cases' tol_p / tol_m / tol_v of float64 Adam of g_dev, every other float -- pad columns,
   gaps, the bias range and the dense block behind the layers, the sentinels -- the bits it had.  The gradient arena holds a NaN pattern and
   keeps it while every result is finite: it is neither read nor written.  db to its own bound.  Two consecutive steps per state.
3. Autotuning context, empty table, mode 2, zeroed g: g is all zero afterwards, p, m, v inside the same bounds.
4. radnet_adam_step_tail: the sweep [sweep_from, n) against float64 Adam, g zeroed per zero_grad, everything in front of sweep_from
   bit-identical in p, g, m, v, every U against ref_wino and the shift against ref_shift of the device's own p, the 64 floats behind n, behind
   every U and behind the shift untouched.
5. Refusals: a negative code, a message, p / m / v unchanged.  A refused multi call has run the preparation of the problems in front of the
   refused one: their mode-0 db (and dw, when split with atomics) may already be zero -- exactly those, nothing else; in mode 2 no byte changes.

First run on one MI355X: every bound held.  Worst err / tol dw 0.108 (w_m1: one product), db 0.019, p 0.999 (the subtraction's own half
ulp, as in the Adam suite), m 0.802, v 0.866, U 0.471, shift 0.484, g 0 (bits); the module's 53 tests take 5 s, the slowest (over_cap) 1.4 s.

`-s` prints the worst err / tol per group at the module's end."""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fp32_edge_cases as P  # noqa: E402
import update_edge_cases as E  # noqa: E402
import wgrad_multi_cases as M  # noqa: E402
from test_gpu_head_edges import ERR_HIP, S_INT, _dev, _Output  # noqa: E402

WORST = {}                                # group -> (max err / tol, what)
G_NAN = 0x7FD1B2C3                        # the quiet NaN the gradient arena holds under an optimizer block
_REFS = {}                                # Entry -> device copies of its reference and bounds


@pytest.fixture(scope="module", autouse=True)
def _summary():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    yield
    _REFS.clear()
    for group, (ratio, what) in sorted(WORST.items()):
        print("\nwgrad multi edges: worst err / tol of %s = %.4f %s" % (group, ratio, what), end="")
    print()


def _note(group, ratio, what):
    if ratio > WORST.get(group, (-1.0,))[0]:
        WORST[group] = (ratio, what)


@contextlib.contextmanager
def _context(tmp_path, ws=M.WS_BIG, lines=(), autotune=0, det=1):
    """A context of its own: `ws` bytes of workspace (0: none), the tuning-table lines loaded, launch timing on (the launch counts)."""
    from radnet_hip import lib as L
    cx = L.Context(0)
    try:
        cx._ws = torch.empty(ws, dtype=torch.uint8, device="cuda") if ws else None
        cx.check(cx.lib.radnet_set_workspace(cx.h, cx._ws.data_ptr() if ws else None, ws), "set_workspace")
        cx.check(cx.lib.radnet_set_autotune(cx.h, autotune), "set_autotune")
        cx.check(cx.lib.radnet_set_deterministic(cx.h, det), "set_deterministic")
        if lines:
            table = tmp_path / "table.txt"
            table.write_text(M.TABLE_HEADER + "\n".join(lines) + "\n")
            cx.check(cx.lib.radnet_tune_load(cx.h, str(table).encode()), "tune_load")
        cx.timing(True)
        yield cx
        torch.cuda.synchronize()
    finally:
        cx.close()


def _table_context(tmp_path, t, det=1):
    return _context(tmp_path, t.ws, M.pin_lines(t.entries), det=det)


def _finish(cx, what, rc=0):
    """The return code of a call and the device's verdict on it; a device error ends the session: nothing else runs on this device."""
    msg = cx.lib.radnet_last_error(cx.h) if rc else None
    if rc == ERR_HIP:
        pytest.exit("%s: %s" % (what, msg), returncode=3)
    assert rc == 0, (what, rc, msg)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("%s: %s" % (what, e), returncode=3)


def _sentinel(count):
    return torch.full((count,), S_INT, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- problems on the device
class _Inputs:
    """What an entry's descriptor reads, uploaded once per entry."""

    def __init__(self, e):
        inp = M.problem_inputs(e)
        self.x, self.dy, self.gscale = _dev(inp["x"]), _dev(inp["dy"]), _dev(inp["gscale"])
        self.dw0, self.db0 = _dev(inp["dw0"]), _dev(inp["db0"])
        r = M.problem_ref(e)
        self.ref, self.tol, self.db_ref, self.db_tol = (_dev(np.ascontiguousarray(r[k])) for k in ("out", "tol", "db", "db_tol"))


def _inputs(e):
    if e not in _REFS:
        _REFS[e] = _Inputs(e)
    return _REFS[e]


def _desc(e, dw_ptr, db_ptr):
    from radnet_hip import lib as L
    cs, g, dm, inp = P.CASES[e.case], P.geometry(P.CASES[e.case], "wgrad"), M.dims(e), _inputs(e)
    d = L.ConvDesc()
    d.nb, d.h, d.w_, d.c, d.oh, d.ow, d.kh, d.kw = cs.nb, cs.h, cs.w, cs.c, g["oh"], g["ow"], cs.kh, cs.kw
    d.stride, d.pad_t, d.pad_l, d.n = cs.stride, cs.pad[0], cs.pad[1], dm["N"]
    d.x, d.dy, d.ld_dy = inp.x.data_ptr(), inp.dy.data_ptr() + 4 * dm["c0"], dm["ld_dy"]
    d.gscale = None if inp.gscale is None else inp.gscale.data_ptr()
    d.dw, d.ldw, d.dw_accumulate, d.db = dw_ptr, dm["ldw"], e.mode, db_ptr
    return d


def _array(descs):
    from radnet_hip import lib as L
    arr = (L.ConvDesc * max(len(descs), 1))()
    for i, d in enumerate(descs):
        arr[i] = d
    return arr


def _fresh_dw(e):
    """[K][ldw] + 64 floats of sentinel; the block's elements hold what the mode asks for (nothing, the old values, zeros)."""
    dm, inp = M.dims(e), _inputs(e)
    buf = _sentinel(dm["K"] * dm["ldw"] + M.TAIL)
    if e.mode:
        buf[:dm["K"] * dm["ldw"]].view(dm["K"], dm["ldw"])[:, :dm["N"]] = inp.dw0 if e.mode == 1 else 0.0
    return buf


def _fresh_db(e):
    dm, inp = M.dims(e), _inputs(e)
    buf = _sentinel(dm["ld_db"] + M.TAIL)
    if e.mode:
        buf[:dm["N"]] = inp.db0 if e.mode == 1 else 0.0
    return buf


def _judge_block(got, ref, tol, what, group):
    err = (got.double() - ref).abs()
    ratio = torch.nan_to_num(torch.where(err > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err)), nan=float("inf"))
    stats = torch.stack([(~(err <= tol)).sum().double(), ratio.max()]).tolist()
    assert int(stats[0]) == 0, (what, group, "%d elements outside the bound (or NaN), worst err / tol %.3f at %s" % (
        int(stats[0]), stats[1], np.unravel_index(int(ratio.argmax()), tuple(got.shape))))
    _note(group, stats[1], what)


def _judge_grads(e, dw, db, what):
    dm, inp = M.dims(e), _inputs(e)
    K, N, ldw = dm["K"], dm["N"], dm["ldw"]
    body = dw[:K * ldw].view(K, ldw)
    _judge_block(body[:, :N], inp.ref, inp.tol, what, "dw")
    assert bool((_bits(body[:, N:]) == S_INT).all()) and bool((_bits(dw[K * ldw:]) == S_INT).all()), (what, "a pad column or the tail of dw lost its sentinel")
    if db is not None:
        _judge_block(db[:N], inp.db_ref, inp.db_tol, what, "db")
        assert bool((_bits(db[N:]) == S_INT).all()), (what, "the floats behind db lost their sentinel")
    if e.zero:
        assert not body[:, :N].any() and (db is None or not db[:N].any()), (what, "a problem without live rows has a gradient")


def _multi(cx, descs, opt=None):
    """-> (return code, launches of timing class 2 this call issued)."""
    torch.cuda.synchronize()
    cx.timing_reset()
    rc = cx.lib.radnet_conv_wgrad_multi(cx.h, _array(descs), len(descs), None if opt is None else C.byref(opt))
    if rc == ERR_HIP:
        pytest.exit("radnet_conv_wgrad_multi: %s" % cx.lib.radnet_last_error(cx.h), returncode=3)
    return rc, cx.timing_read(2)[1]


def _gradients_only(cx, t, what):
    bufs = [(_fresh_dw(e), _fresh_db(e) if e.db else None) for e in t.entries]
    rc, launches = _multi(cx, [_desc(e, dw.data_ptr(), None if db is None else db.data_ptr()) for e, (dw, db) in zip(t.entries, bufs)])
    _finish(cx, what, rc)
    for i, (e, (dw, db)) in enumerate(zip(t.entries, bufs)):
        _judge_grads(e, dw, db, what + (i, e.case, "mode %d" % e.mode))
    return bufs, launches


# ---------------------------------------------------------------------------------------------------------------- 1. gradients only
@pytest.mark.parametrize("name", list(M.TABLES))
def test_gradients_of_every_table_against_float64(tmp_path, name):
    t = M.TABLES[name]
    judged = 0
    with _table_context(tmp_path, t) as cx:
        first, launches = _gradients_only(cx, t, (name, "ordered"))
        assert launches == len(M.plan(t.entries, t.ws)) == M.CLAIMS[name][0], (name, "launches", launches)
        second, _ = _gradients_only(cx, t, (name, "ordered, second call"))
        for (dw1, db1), (dw2, db2) in zip(first, second):
            assert torch.equal(_bits(dw1), _bits(dw2)) and (db1 is None or torch.equal(_bits(db1), _bits(db2))), (name, "two ordered calls differ")
            judged += 1
    skipped = sum(1 for e in t.entries if M.dims(e)["c"] % M.launch_shape(e, t.ws)["bmk"])
    assert judged == len(t.entries) and skipped == 0, "no table leaves a problem unjudged"


def test_gradients_of_all_default_with_atomic_slices(tmp_path):
    t = M.TABLES["all_default"]
    with _table_context(tmp_path, t, det=0) as cx:
        _, launches = _gradients_only(cx, t, (t.name, "atomic"))
        assert launches == len(M.plan(t.entries, t.ws, ordered=False))


def test_an_empty_list_returns_ok_and_launches_nothing(tmp_path):
    with _context(tmp_path) as cx:
        rc, launches = _multi(cx, [])
        assert rc == 0 and launches == 0


# ---------------------------------------------------------------------------------------------------------------- 2. the optimizer block
class _Arena:
    """A full arena buffer on the device (wgrad_multi_cases._arena): prefill bits, the elements that must come within their bound, the ones
    that must be +0.0; every other element must keep its bits."""

    def __init__(self, res):
        self.prefill = torch.from_numpy(res["prefill"].view(np.int32).copy()).cuda()
        self.inside, self.zero = _dev(res["inside"]), _dev(res["zero"])
        self.ref, self.tol = _dev(res["ref"]), _dev(res["tol"])

    def fresh(self):
        return self.prefill.clone().view(torch.float32)

    def judge(self, buf, what, group):
        got, bits = buf.double(), _bits(buf)
        err = torch.where(self.inside, (got - self.ref).abs(), torch.zeros_like(got))
        bad = self.inside & ~(err <= self.tol)
        moved = ~self.inside & ~self.zero & (bits != self.prefill)
        nonzero = self.zero & (bits != 0)
        ratio = torch.nan_to_num(torch.where(err > 0, err / self.tol.clamp_min(1e-300), torch.zeros_like(err)), nan=float("inf"))
        stats = torch.stack([bad.sum().double(), moved.sum().double(), nonzero.sum().double(), ratio.max() if ratio.numel() else torch.zeros((), dtype=torch.double, device="cuda")]).tolist()
        assert int(stats[1]) == 0, (what, group, "%d elements that are nobody's changed their bits" % int(stats[1]), torch.nonzero(moved)[:4].ravel().tolist())
        assert int(stats[0]) == 0, (what, group, "%d elements outside the bound (or NaN), worst err / tol %.3f at %d" % (int(stats[0]), stats[3], int(ratio.argmax())))
        assert int(stats[2]) == 0, (what, group, "%d elements that must be +0.0 hold other bits" % int(stats[2]))
        _note(group, stats[3], what)


def _opt_block(bufs, n, t, gs):
    from radnet_hip import lib as L
    opt = L.WgradAdam()
    opt.p, opt.g, opt.m, opt.v, opt.n, opt.t = bufs["p"].data_ptr(), bufs["g"].data_ptr(), bufs["m"].data_ptr(), bufs["v"].data_ptr(), n, t
    opt.lr, opt.beta1, opt.beta2, opt.eps, opt.grad_scale = float(E.LR), float(E.B1), float(E.B2), float(E.EPS), float(gs)
    return opt


def _arena_descs(t, ar, base, dbs):
    return [_desc(e, base.data_ptr() + 4 * off, None if db is None else db.data_ptr()) for e, off, db in zip(t.entries, ar.offs, dbs)]


def _device_grads(cx, t, ar, what):
    """g_dev: the gradients of a gradients-only call with the same launch shapes on this context, from a zeroed arena of their own."""
    g2 = torch.zeros(ar.n, device="cuda")
    dbs = [_fresh_db(e) if e.db else None for e in t.entries]
    rc, _ = _multi(cx, _arena_descs(t, ar, g2, dbs))
    _finish(cx, what + ("gradients only",), rc)
    host = g2.cpu().numpy()
    return [host[off:off + M.dims(e)["K"] * M.dims(e)["ldw"]].reshape(M.dims(e)["K"], M.dims(e)["ldw"])[:, :M.dims(e)["N"]] for e, off in zip(t.entries, ar.offs)]


def _step(cx, t, ar, state, bufs, step, what, grads_after=False):
    """One radnet_conv_wgrad_multi call with the optimizer block on `bufs` (p, g, m, v with their tails), judged over the whole arena."""
    tt, gs = step
    grads = None if grads_after else _device_grads(cx, t, ar, what)
    before = {k: bufs[k].clone() for k in "pgmv"}
    dbs = [_fresh_db(e) if e.db else None for e in t.entries]
    rc, launches = _multi(cx, _arena_descs(t, ar, bufs["g"], dbs), _opt_block(bufs, ar.n, tt, gs))
    _finish(cx, what, rc)
    if grads_after:                                                          # the autotuner has chosen: the same shapes again
        grads = _device_grads(cx, t, ar, what)
    refs = M.epilogue_refs(t.name, state, grads, tt, gs)
    for k in "pmv":
        res = dict(refs[k], prefill=before[k].cpu().numpy().view(np.uint32))
        _Arena(res).judge(bufs[k], what, k)
        assert bool(torch.isfinite(bufs[k][:ar.n]).all()), (what, k, "a result is not finite: the gradient arena was read")
    assert torch.equal(_bits(bufs["g"]), _bits(before["g"])), (what, "the gradient arena was written")
    for i, (e, db) in enumerate(zip(t.entries, dbs)):
        if db is not None:
            inp = _inputs(e)
            _judge_block(db[:M.dims(e)["N"]], inp.db_ref, inp.db_tol, what + (i, e.case), "db")
            assert bool((_bits(db[M.dims(e)["N"]:]) == S_INT).all()), (what, i, "the floats behind db lost their sentinel")
    return launches


def _arena_buffers(ar, state, g_bits):
    tail = np.full(M.TAIL, M.SENTINEL, np.uint32)
    bufs = {k: torch.from_numpy(np.concatenate([state[k].view(np.uint32), tail]).view(np.int32)).cuda().view(torch.float32) for k in "pmv"}
    bufs["g"] = torch.from_numpy(np.concatenate([np.full(ar.n, g_bits, np.uint32), tail]).view(np.int32)).cuda().view(torch.float32)
    return bufs


@pytest.mark.parametrize("which", M.OPT_STATES)
@pytest.mark.parametrize("name", M.OPT_TABLES)
def test_the_adam_epilogue_over_the_whole_arena_against_float64(tmp_path, name, which):
    t, ar = M.TABLES[name], M.arena_of(name)
    state = {k: np.array(v) for k, v in M.opt_state(name, which).items()}
    with _table_context(tmp_path, t) as cx:
        bufs = _arena_buffers(ar, state, G_NAN)
        for step in M.OPT_STEPS[which]:                                       # two consecutive steps: the second from the device's own state
            launches = _step(cx, t, ar, state, bufs, step, (name, which, "t=%d" % step[0], "gs=%g" % step[1]))
            assert launches == M.CLAIMS[name][0]
            state = {k: bufs[k][:ar.n].cpu().numpy() for k in "pmv"}


# ---------------------------------------------------------------------------------------------------------------- 3. autotuning
def test_the_adam_epilogue_on_an_autotuning_context_with_an_empty_table(tmp_path):
    t, ar = M.TABLES["mode2_three"], M.arena_of("mode2_three")
    state = {k: np.array(v) for k, v in M.opt_state(t.name, "random").items()}
    with _context(tmp_path, autotune=1) as cx:
        assert cx.lib.radnet_tuned_shapes(cx.h) == 0
        bufs = _arena_buffers(ar, state, 0)                                   # write mode 2: the caller has zeroed the gradient arena
        _step(cx, t, ar, state, bufs, M.OPT_STEPS["random"][0], (t.name, "autotune"), grads_after=True)
        assert cx.lib.radnet_tuned_shapes(cx.h) == len(t.entries)
        assert not bufs["g"][:ar.n].any(), "the trial launches' sums were left in the gradient arena"


# ---------------------------------------------------------------------------------------------------------------- 4. the tail
def _g_arena(lay, state, zg):
    sw = np.arange(lay.sweep_from, lay.n) if zg else np.arange(0)
    return _Arena(M._arena(state["g"], sw, np.zeros(sw.size), np.zeros(sw.size), zero_idx=sw if zg else None))


def _tail_call(cx, lay, bufs, t, gs, zg):
    """-> (return code, the U buffers, the shift buffer)."""
    from radnet_hip import lib as L
    us = [_sentinel(36 * c * n + M.TAIL) for _, c, n in lay.wino]
    arr = (L.AdamWino * max(len(lay.wino), 1))()
    for i, (off, c, n) in enumerate(lay.wino):
        arr[i].off, arr[i].c, arr[i].n, arr[i].u = off, c, n, us[i].data_ptr()
    args = [bufs[k].data_ptr() for k in "pgmv"] + [C.c_int64(lay.n), t, C.c_float(E.LR), C.c_float(E.B1), C.c_float(E.B2), C.c_float(E.EPS), C.c_float(gs), zg]
    shift = None
    if lay.bias:
        b = E.bias_inputs(lay.bias[1])
        sd, td = _dev(b["scale"]), _dev(b["t0"])
        shift = _sentinel(lay.bias[1] + M.TAIL)
        args += [C.c_int64(lay.bias[0]), C.c_int64(lay.bias[1]), sd.data_ptr(), td.data_ptr(), shift.data_ptr()]
    else:
        args += [C.c_int64(0), C.c_int64(0), None, None, None]
    rc = cx.lib.radnet_adam_step_tail(cx.h, *args, arr, len(lay.wino), C.c_int64(lay.sweep_from))
    if lay.bias:
        torch.cuda.synchronize()                                              # scale / t0 live until the launch has run
    return rc, us, shift


@pytest.mark.parametrize("name", list(M.TAILS))
def test_adam_step_tail_every_layout_against_float64(tmp_path, name):
    lay, state = M.TAILS[name], M.tail_state(name)
    launches = 0
    with _context(tmp_path, ws=0) as cx:
        for t, gs in lay.steps:
            refs = M.tail_refs(lay, state, t, gs, 1)
            outs = {k: _Arena(refs[k]) for k in "pmv"}
            del refs
            for zg in ((1,) if name == "over_cap" else (1, 0)):
                what = ("adam_tail", name, "t=%d" % t, "gs=%g" % gs, "zero_grad=%d" % zg)
                outs["g"] = _g_arena(lay, state, zg)
                bufs = {k: outs[k].fresh() for k in "pgmv"}
                rc, us, shift = _tail_call(cx, lay, bufs, t, gs, zg)
                _finish(cx, what, rc)
                for k in "pgmv":
                    outs[k].judge(bufs[k], what, k if k != "g" else "g (exact)")
                p_dev = bufs["p"][:lay.n].cpu().numpy()
                for i, (off, c, n) in enumerate(lay.wino):
                    _note("U", _Output(E.ref_wino(p_dev, off, c, n)).judge(us[i], what + ("u%d" % i,)), what)
                if lay.bias:
                    b = E.bias_inputs(lay.bias[1])
                    _note("shift", _Output(E.ref_shift(p_dev, b["scale"], b["t0"], *lay.bias)).judge(shift, what + ("shift",)), what)
                launches += 1
    assert launches == len(lay.steps) * (1 if name == "over_cap" else 2)


@pytest.mark.parametrize("name", list(M.TAIL_REFUSALS))
def test_adam_step_tail_refuses_what_lies_outside_its_contract(tmp_path, name):
    lay, fragment = M.TAIL_REFUSALS[name]
    state = M.tail_state(name)
    with _context(tmp_path, ws=0) as cx:
        tail = np.full(M.TAIL, M.SENTINEL, np.uint32)
        bufs = {k: torch.from_numpy(np.concatenate([state[k].view(np.uint32), tail]).view(np.int32)).cuda().view(torch.float32) for k in "pgmv"}
        before = {k: v.clone() for k, v in bufs.items()}
        rc, us, shift = _tail_call(cx, lay, bufs, 2, E.GRAD_SCALES[1], 1)
        msg = cx.lib.radnet_last_error(cx.h)
        assert rc < 0 and rc != ERR_HIP, (name, rc)
        assert msg and msg.decode().startswith("adam_tail:") and fragment in msg.decode(), (name, msg)
        torch.cuda.synchronize()
        for k in "pgmv":
            assert torch.equal(_bits(bufs[k]), _bits(before[k])), (name, k, "a refused call wrote to an arena")
        for u in us + ([shift] if shift is not None else []):
            assert bool((_bits(u) == S_INT).all()), (name, "a refused call wrote a transform or the shift")
        # the context still works
        ok = M.TAILS["one_layer_gaps"]
        st = M.tail_state(ok.name)
        refs = M.tail_refs(ok, st, 2, E.GRAD_SCALES[1], 1)
        outs = {k: _Arena(refs[k]) for k in "pgmv"}
        good = {k: outs[k].fresh() for k in "pgmv"}
        _finish(cx, (name, "after the refusal"), _tail_call(cx, ok, good, 2, E.GRAD_SCALES[1], 1)[0])
        for k in "pmv":
            outs[k].judge(good[k], (name, "after the refusal"), k)


# ---------------------------------------------------------------------------------------------------------------- 5. refusals of the multi call
def _refused(cx, descs, opt, what):
    rc, launches = _multi(cx, descs, opt)
    msg = cx.lib.radnet_last_error(cx.h)
    assert rc < 0 and launches == 0, (what, rc, launches)
    assert msg and msg.decode().startswith("conv_wgrad"), (what, msg)
    torch.cuda.synchronize()


def test_the_optimizer_block_refuses_what_it_cannot_step(tmp_path):
    t, ar = M.TABLES["mode2_three"], M.arena_of("mode2_three")
    state = {k: np.array(v) for k, v in M.opt_state(t.name, "random").items()}
    with _table_context(tmp_path, t) as cx:
        bufs = _arena_buffers(ar, state, 0)
        dbs = [_fresh_db(e) for e in t.entries]
        before = {k: v.clone() for k, v in bufs.items()}
        dbs_before = [db.clone() for db in dbs]
        good = lambda: _arena_descs(t, ar, bufs["g"], dbs)
        opt = _opt_block(bufs, ar.n, 3, E.GRAD_SCALES[2])
        # a gradient that is added to an earlier one is not the whole gradient
        descs = good()
        descs[0].dw_accumulate = 1
        _refused(cx, descs, opt, "mode 1 with an optimizer block")
        # slices added with atomics have no last writer (w_deep_m splits into 8)
        cx.check(cx.lib.radnet_set_deterministic(cx.h, 0), "set_deterministic")
        _refused(cx, good(), opt, "atomics with a split")
        cx.check(cx.lib.radnet_set_deterministic(cx.h, 1), "set_deterministic")
        outside = torch.zeros(M.dims(t.entries[2])["K"] * M.dims(t.entries[2])["ldw"], device="cuda")
        descs = good()
        descs[2].dw = outside.data_ptr()
        _refused(cx, descs, opt, "a dw outside the arena")
        _refused(cx, good(), _opt_block(bufs, ar.n, 0, E.GRAD_SCALES[2]), "t = 0")
        descs = good()
        descs[2].c = 96
        _refused(cx, descs, opt, "c = 96 in third place")
        # write mode 2 throughout: no byte of any buffer has changed
        for k in "pgmv":
            assert torch.equal(_bits(bufs[k]), _bits(before[k])), (k, "a refused call wrote to an arena")
        for a, b in zip(dbs, dbs_before):
            assert torch.equal(_bits(a), _bits(b)), "a refused call in write mode 2 wrote a db"
        assert not outside.any()
        # the context still works
        _step(cx, t, ar, state, bufs, M.OPT_STEPS["random"][0], (t.name, "after the refusals"))


# (ordered reductions?, with the optimizer block?)
@pytest.mark.parametrize("det,with_opt", [(1, False), (0, False), (1, True), (0, True)])
def test_a_refused_call_has_zeroed_only_the_mode0_destinations_in_front_of_it(tmp_path, det, with_opt):
    """The preparation pass runs radnet_conv_wgrad's host side problem by problem, so the memsets of write mode 0 -- db, and dw when the
    slices add with atomics -- of the problems in FRONT of the refused one are already enqueued when the call returns its error
    (include/radnet_hip.h says so).  Exactly those destinations are zero afterwards, element for element; every other byte -- their pad
    columns, the mode-2 problem, the problems behind the refused one, p, m, v -- is what it was.  Under an optimizer block with atomic
    slices the FIRST problem is the refused one, after its own preparation: its own two destinations are the zeroed ones."""
    entries = (M.entry("w_deep_m"), M.entry("b_3x3", mode=2), M.entry("w_s2_3x3"), M.entry("w_pad_br"))          # the third gets c = 96
    t = M.Table("refused_third", entries, M.WS_BIG)
    assert M.launch_shape(entries[0], t.ws, bool(det))["slices"] == 8
    offs, at = [], 0
    for e in entries:
        offs.append(at)
        at += M.dims(e)["K"] * M.dims(e)["ldw"] + 4
    ar = M.Arena(at, tuple(offs), None, None)
    state = {k: E.adam_state(ar.n)[k] for k in "pmv"}
    with _table_context(tmp_path, t, det=det) as cx:
        bufs = _arena_buffers(ar, state, S_INT & 0xFFFFFFFF)                 # the destinations hold the sentinel: a zero is the memset's
        dbs = [_fresh_db(e) for e in entries]
        for e, db in zip(entries, dbs):
            _bits(db)[:] = S_INT
        before = {k: v.clone() for k, v in bufs.items()}
        descs = _arena_descs(t, ar, bufs["g"], dbs)
        descs[2].c = 96
        _refused(cx, descs, _opt_block(bufs, ar.n, 2, E.GRAD_SCALES[1]) if with_opt else None, ("atomic slices of the first problem" if with_opt and not det else "c = 96 in third place", det, with_opt))
        for k in "pmv":
            assert torch.equal(_bits(bufs[k]), _bits(before[k])), (k, "a refused call wrote to an arena")
        want = before["g"].clone()
        if not det:                                                           # problem 0: write mode 0, split, atomics
            d0 = M.dims(entries[0])
            want[:d0["K"] * d0["ldw"]].view(d0["K"], d0["ldw"])[:, :d0["N"]] = 0.0
        assert torch.equal(_bits(bufs["g"]), _bits(want)), "dw: other bytes than the atomic mode-0 destination in front of the refused problem changed"
        for i, (e, db) in enumerate(zip(entries, dbs)):
            zeroed = i == 0
            n = M.dims(e)["N"]
            assert bool((_bits(db[:n]) == (0 if zeroed else S_INT)).all()) and bool((_bits(db[n:]) == S_INT).all()), (i, "db")
