"""Edge shapes of the pooling, RoI crop, classifier head and loss kernels: the entry points of csrc/elementwise.hip (maxpool, roi_resize
fwd / bwd, avgpool fwd / bwd_relu, dense_heads fwd / bwd, rpn_loss, det_loss) and radnet_head_tail_fwd of csrc/head_tail.hip against the
float64 references of tests/head_edge_cases.py (checked against the oracle, and shown to have teeth, by
tests/test_head_edge_cases_reference.py).

Every case of every table runs inside the contract of its entry point.  After EVERY launch, for EVERY element of the full output
buffer -- the whole tensor the kernel writes into and 64 floats behind it, prefilled with the sentinel bits (or the old values of an
accumulating launch): an element that must be written lies within its bound of head_edge_cases.py and is no NaN, an element that must
not be written still holds the sentinel, an element the contract says is zero-filled holds the bits of +0.0.  maxpool and
avgpool_bwd_relu are compared bit for bit (their bound is 0).  The RoI gradient and the RPN loss run in the ordered and in the atomic
form (radnet_set_deterministic, restored in a finally).  The head tail is launched twice on the same zeroed scratch and must give the
same bits, then once more in its inference form.  The rejection tests call an entry with arguments its host checks refuse: a negative
code, a message that names the entry, no output element touched; nothing is launched.

`-s` prints the worst err / tol per test."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import head_edge_cases as E  # noqa: E402

S_INT = int(E.SENTINEL)
ERR_HIP = -2


@pytest.fixture(scope="module")
def ctx():
    """The module's one context, on torch's current stream."""
    from radnet_hip import lib as L
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    cx = L.Context(0)
    yield cx
    torch.cuda.synchronize()
    cx.close()


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the cached inputs are read-only


class _Output:
    """One output buffer on the device: prefilled with the sentinel (or the old values); reference, bound and masks live on the device,
    a launch's verdict is six scalars."""

    def __init__(self, res):
        self.inside, self.zero = _dev(res["inside"]), _dev(res["zero"])
        self.ref = _dev(np.where(res["inside"], res["buf"], 0.0))
        self.tol = _dev(res["tol"])
        self.size = res["buf"].size
        self.old = _dev(res["old"].reshape(-1)) if "old" in res else None

    def fresh(self):
        buf = torch.full((self.size,), S_INT, dtype=torch.int32, device="cuda").view(torch.float32)
        if self.old is not None:
            buf[:self.old.numel()] = self.old
        return buf

    def judge(self, buf, what):
        got = buf.double()
        err = torch.where(self.inside, (got - self.ref).abs(), torch.zeros_like(got))
        ok = torch.where(self.inside, err <= self.tol, torch.ones_like(self.inside))
        ratio = torch.where(err > 0, err / self.tol.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        bits = buf.view(torch.int32)
        spilled = (bits != S_INT) & ~self.inside
        stats = torch.stack([(~ok).sum().double(), (torch.isnan(got) & self.inside).sum().double(), spilled.sum().double(), ratio.max(),
                             ((bits != 0) & self.zero).sum().double(), (self.inside & (bits == S_INT)).sum().double()]).tolist()
        bad, nans, lost, worst, nonzero, unwritten = int(stats[0]), int(stats[1]), int(stats[2]), stats[3], int(stats[4]), int(stats[5])
        assert unwritten == 0, (what, "%d elements that must be written still hold the sentinel" % unwritten)
        assert nans == 0, (what, "%d NaN among the elements that must be written" % nans)
        assert lost == 0, (what, "%d elements that must not be written lost their sentinel" % lost, torch.nonzero(spilled)[:4].tolist())
        assert bad == 0, (what, "%d elements outside the bound, worst err / tol %.3f at flat index %d" % (bad, worst, int(ratio.argmax())))
        assert nonzero == 0, (what, "%d elements that must be +0.0 hold other bits" % nonzero)
        return worst


def _run(ctx, what, refs, launch):
    """Fresh buffers of every output in `refs`, one launch, every buffer judged; -> (worst err / tol, the buffers)."""
    outs = {k: _Output(v) for k, v in refs.items()}
    bufs = {k: o.fresh() for k, o in outs.items()}
    try:
        launch(bufs)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "(%d)" % ERR_HIP in str(e) or "HIP error" in str(e):                   # a device fault: nothing else runs on this device
            pytest.exit("%s: %s" % (what, e), returncode=3)
        raise
    return max(outs[k].judge(bufs[k], what + (k,)) for k in outs), bufs


@contextlib.contextmanager
def _Deterministic(ctx, on):
    """radnet_set_deterministic for a block; the context's own setting is restored in the finally."""
    before = ctx.lib.radnet_get_deterministic(ctx.h)
    ctx.check(ctx.lib.radnet_set_deterministic(ctx.h, on), "set_deterministic")
    try:
        yield
    finally:
        ctx.check(ctx.lib.radnet_set_deterministic(ctx.h, before), "set_deterministic")


# ---------------------------------------------------------------------------------------------------------------- pooling, RoI crop
@pytest.mark.parametrize("i", range(len(E.MAXPOOL)), ids=[str(c) for c in E.MAXPOOL])
def test_maxpool(ctx, i):
    nb, h, w, c, k, s = E.MAXPOOL[i]
    x = _dev(E.maxpool_inputs(i)["x"])
    worst, _ = _run(ctx, ("maxpool", E.MAXPOOL[i]), E.ref_maxpool(E.maxpool_inputs(i)["x"], k, s),
                    lambda b: ctx.call("radnet_maxpool_fwd", x, b["y"], nb, h, w, c, k, s))
    assert worst == 0.0                                                           # bit-exact


@pytest.mark.parametrize("mi", range(len(E.ROI_MAPS)), ids=[str(c) for c in E.ROI_MAPS])
def test_roi_resize_fwd(ctx, mi):
    H, W, C = E.ROI_MAPS[mi]
    worst = 0.0
    for ps in E.ROI_FWD_PS:
        d = E.roi_inputs(mi, ps)
        fmap, rois = _dev(d["fmap"]), _dev(d["rois"])
        w, _ = _run(ctx, ("roi_resize_fwd", E.ROI_MAPS[mi], ps), E.ref_roi_fwd(d["fmap"], d["rois"], ps),
                    lambda b: ctx.call("radnet_roi_resize_fwd", fmap, H, W, C, rois, len(d["rois"]), ps, b["y"]))
        worst = max(worst, w)
    print("roi_resize_fwd %s: worst err / tol %.3f" % (E.ROI_MAPS[mi], worst))


@pytest.mark.parametrize("mi", range(len(E.ROI_MAPS)), ids=[str(c) for c in E.ROI_MAPS])
def test_roi_resize_bwd_ordered_and_atomic(ctx, mi):
    H, W, C = E.ROI_MAPS[mi]
    worst, launches = 0.0, 0
    for ps in E.roi_bwd_ps(mi):
        d = E.roi_inputs(mi, ps)
        dy, rois = _dev(d["dy"]), _dev(d["rois"])
        for det in (1, 0):
            ordered = bool(det) and ps <= 32                                      # above the mask width the entry takes the atomics kernel
            ref = E.ref_roi_bwd(d["dy"], H, W, d["rois"], ps, d["old"], ordered)
            assert not ref["dfmap"]["spilled"]
            with _Deterministic(ctx, det):
                w, _ = _run(ctx, ("roi_resize_bwd", E.ROI_MAPS[mi], ps, "ordered" if ordered else "atomic"), ref,
                            lambda b: ctx.call("radnet_roi_resize_bwd", dy, H, W, C, rois, len(d["rois"]), ps, b["dfmap"]))
            worst, launches = max(worst, w), launches + 1
    print("roi_resize_bwd %s: %d launches, worst err / tol %.3f" % (E.ROI_MAPS[mi], launches, worst))
    assert launches == 2 * len(E.roi_bwd_ps(mi))


@pytest.mark.parametrize("i", range(len(E.AVGPOOL)), ids=[str(c) for c in E.AVGPOOL])
def test_avgpool_fwd_and_bwd_relu(ctx, i):
    r, hw, c = E.AVGPOOL[i]
    d = E.avgpool_inputs(i)
    x, g = _dev(d["x"]), _dev(d["g"])
    worst, _ = _run(ctx, ("avgpool_fwd", E.AVGPOOL[i]), E.ref_avgpool_fwd(d["x"]), lambda b: ctx.call("radnet_avgpool_fwd", x, r, hw, c, b["y"]))
    exact, _ = _run(ctx, ("avgpool_bwd_relu", E.AVGPOOL[i]), E.ref_avgpool_bwd(d["g"], d["x"]),
                    lambda b: ctx.call("radnet_avgpool_bwd_relu", g, x, r, hw, c, b["dx"]))
    print("avgpool %s: worst err / tol %.3f" % (E.AVGPOOL[i], worst))
    assert exact == 0.0                                                           # one fp32 division per element: bit-exact


# ---------------------------------------------------------------------------------------------------------------- dense heads
@pytest.mark.parametrize("i", range(len(E.DENSE_FWD)), ids=[str(c) for c in E.DENSE_FWD])
def test_dense_heads_fwd(ctx, i):
    r, k, ldw, nc, nreg = E.DENSE_FWD[i]
    d = E.dense_fwd_inputs(i)
    feat, w, b = _dev(d["feat"]), _dev(d["w"]), _dev(d["b"])
    worst, _ = _run(ctx, ("dense_heads_fwd", E.DENSE_FWD[i]), E.ref_dense_fwd(d["feat"], d["w"], d["b"], nc, nreg),
                    lambda o: ctx.call("radnet_dense_heads_fwd", feat, r, k, w, ldw, b, nc, nreg, o["out_cls"], o["out_regr"]))
    print("dense_heads_fwd %s: worst err / tol %.3f" % (E.DENSE_FWD[i], worst))


@pytest.mark.parametrize("i", range(len(E.DENSE_BWD)), ids=[str(c) for c in E.DENSE_BWD])
def test_dense_heads_bwd(ctx, i):
    r, k, ldw, nout, acc = E.DENSE_BWD[i]
    d = E.dense_bwd_inputs(i)
    feat, dz, w = _dev(d["feat"]), _dev(d["dz"]), _dev(d["w"])
    worst, _ = _run(ctx, ("dense_heads_bwd", E.DENSE_BWD[i]), E.ref_dense_bwd(d["feat"], d["dz"], d["w"], ldw, nout, acc, d["dw0"], d["db0"]),
                    lambda o: ctx.call("radnet_dense_heads_bwd", feat, dz, r, k, w, ldw, nout, o["dw"], o["db"], o["dfeat"], acc))
    print("dense_heads_bwd %s: worst err / tol %.3f" % (E.DENSE_BWD[i], worst))


# ---------------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("i", range(len(E.RPN)), ids=[str(c) for c in E.RPN])
def test_rpn_loss_every_layout_mode_and_form(ctx, i):
    m, a, ld_pred, ld_dz = E.RPN[i]
    worst, launches = 0.0, 0
    for layout in E.RPN_LAYOUTS:
        d = E.rpn_inputs(i, layout)
        pred, y_cls, y_regr = _dev(d["pred"]), _dev(d["y_cls"]), _dev(d["y_regr"])
        for mode in (0, 1):
            ref = E.rpn_outputs(d["pred"], d["y_cls"], d["y_regr"], m, a, ld_dz, mode)
            for det in (1, 0):
                scratch = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")          # the entry zeroes it itself
                with _Deterministic(ctx, det):
                    w, _ = _run(ctx, ("rpn_loss", E.RPN[i], layout, "mode %d" % mode, "ordered" if det else "atomic"), ref,
                                lambda o: ctx.call("radnet_rpn_loss", pred, ld_pred, y_cls, y_regr, m, a, mode, o["dz"], ld_dz, o["losses"], scratch))
                worst, launches = max(worst, w), launches + 1
    print("rpn_loss %s: %d launches, worst err / tol %.3f" % (E.RPN[i], launches, worst))
    assert launches == 16


@pytest.mark.parametrize("i", range(len(E.DET)), ids=[str(c) for c in E.DET])
def test_det_loss_every_layout(ctx, i):
    r, nc, nreg = E.DET[i]
    worst = 0.0
    for layout in E.DET_LAYOUTS:
        d = E.det_inputs(i, layout)
        q, pregr, y1, y2 = (_dev(d[k]) for k in ("q", "pregr", "y1", "y2"))
        w, _ = _run(ctx, ("det_loss", E.DET[i], layout), E.ref_det(d["q"], d["pregr"], d["y1"], d["y2"]),
                    lambda o: ctx.call("radnet_det_loss", q, pregr, y1, y2, r, nc, nreg, o["dz"], o["losses"]))
        worst = max(worst, w)
    print("det_loss %s: worst err / tol %.3f" % (E.DET[i], worst))


# ---------------------------------------------------------------------------------------------------------------- head tail
@pytest.mark.parametrize("i", range(len(E.HEAD_TAIL)), ids=["-".join(str(v) for v in c) for c in E.HEAD_TAIL])
def test_head_tail_fwd_against_the_float64_chain(ctx, i):
    cs = E.HEAD_TAIL[i]
    d = E.head_tail_inputs(i)
    y5, w, b, y1, y2, live = (_dev(d[k]) for k in ("y5", "w", "b", "y1", "y2", "live"))
    scratch = torch.zeros(int(ctx.lib.radnet_head_tail_scratch_bytes(cs.R)), dtype=torch.uint8, device="cuda")
    ref = E.ref_head_tail(cs, d["y5"], d["w"], d["b"], d["y1"], d["y2"], d["live"])
    train = lambda o: ctx.call("radnet_head_tail_fwd", y5, cs.R, cs.hw, cs.c, w, cs.ldw, b, cs.nc, cs.nreg, o["feat"], o["p_cls"], o["p_regr"], y1, y2,
                               o["dz"], o["losses"], cs.groups, live, scratch)
    worst, first = _run(ctx, ("head_tail_fwd", tuple(cs), "first launch"), ref, train)
    w2, second = _run(ctx, ("head_tail_fwd", tuple(cs), "second launch"), ref, train)          # the arrival counters are back at zero
    for k in first:
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), (tuple(cs), k, "two launches on one scratch differ in bits")
    # the inference form: no targets, no dz, no losses
    infer = lambda o: ctx.call("radnet_head_tail_fwd", y5, cs.R, cs.hw, cs.c, w, cs.ldw, b, cs.nc, cs.nreg, o["feat"], o["p_cls"], o["p_regr"], None, None,
                               None, None, 1, None, scratch)
    w3, third = _run(ctx, ("head_tail_fwd", tuple(cs), "inference"), E.ref_head_tail(cs, d["y5"], d["w"], d["b"], None, None, None, targets=False), infer)
    for k in third:
        assert torch.equal(first[k].view(torch.int32), third[k].view(torch.int32)), (tuple(cs), k, "the inference form differs in bits")
    assert not bool(scratch[:4 * (1 + cs.R)].any()), "an arrival counter did not return to zero"
    print("head_tail_fwd %s: worst err / tol %.3f" % (tuple(cs), max(worst, w2, w3)))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusals(lib, h, z, o, sc):
    """entry -> (the prefix of its messages, [(what, the call)]): arguments the host checks refuse before anything is launched."""
    return {
        "radnet_maxpool_fwd": ("maxpool:", [
            ("s = 0", lambda: lib.radnet_maxpool_fwd(h, z, o, 1, 5, 5, 4, 3, 0)), ("k = 0", lambda: lib.radnet_maxpool_fwd(h, z, o, 1, 5, 5, 4, 0, 1)),
            ("c % 4", lambda: lib.radnet_maxpool_fwd(h, z, o, 1, 5, 5, 6, 3, 2)), ("h < k", lambda: lib.radnet_maxpool_fwd(h, z, o, 1, 2, 5, 4, 3, 2))]),
        "radnet_roi_resize_bwd": ("roi_resize_bwd:", [
            ("c % 4", lambda: lib.radnet_roi_resize_bwd(h, z, 5, 7, 6, z, 3, 2, o)), ("r = 0", lambda: lib.radnet_roi_resize_bwd(h, z, 5, 7, 4, z, 0, 2, o)),
            ("ps = 0", lambda: lib.radnet_roi_resize_bwd(h, z, 5, 7, 4, z, 3, 0, o))]),
        "radnet_avgpool_fwd": ("avgpool:", [
            ("r = 0", lambda: lib.radnet_avgpool_fwd(h, z, 0, 49, 4, o)), ("hw = 0", lambda: lib.radnet_avgpool_fwd(h, z, 2, 0, 4, o))]),
        "radnet_avgpool_bwd_relu": ("avgpool_bwd:", [
            ("r = 0", lambda: lib.radnet_avgpool_bwd_relu(h, z, z, 0, 49, 4, o)), ("hw = 0", lambda: lib.radnet_avgpool_bwd_relu(h, z, z, 2, 0, 4, o))]),
        "radnet_dense_heads_fwd": ("dense_heads:", [
            ("r = 0", lambda: lib.radnet_dense_heads_fwd(h, z, 0, 8, z, 32, z, 7, 24, o, o)), ("k = 0", lambda: lib.radnet_dense_heads_fwd(h, z, 2, 0, z, 32, z, 7, 24, o, o)),
            ("nc = 0", lambda: lib.radnet_dense_heads_fwd(h, z, 2, 8, z, 32, z, 0, 24, o, o)), ("ldw = 48", lambda: lib.radnet_dense_heads_fwd(h, z, 2, 8, z, 48, z, 7, 24, o, o))]),
        "radnet_dense_heads_bwd": ("dense_heads_bwd:", [
            ("ldw = 48", lambda: lib.radnet_dense_heads_bwd(h, z, z, 4, 8, z, 48, 31, o, o, o, 0)), ("nout > ldw", lambda: lib.radnet_dense_heads_bwd(h, z, z, 4, 8, z, 32, 33, o, o, o, 0)),
            ("r = 0", lambda: lib.radnet_dense_heads_bwd(h, z, z, 0, 8, z, 32, 31, o, o, o, 1)),
            ("R = 513, ldw = 32: more than 64 KiB of LDS", lambda: lib.radnet_dense_heads_bwd(h, z, z, 513, 8, z, 32, 31, o, o, o, 0))]),
        "radnet_rpn_loss": ("rpn_loss:", [
            ("m = 0", lambda: lib.radnet_rpn_loss(h, z, 64, z, z, 0, 12, 0, o, 64, o, o)), ("a = 0", lambda: lib.radnet_rpn_loss(h, z, 64, z, z, 7, 0, 0, o, 64, o, o)),
            ("ld_dz < 5a", lambda: lib.radnet_rpn_loss(h, z, 64, z, z, 7, 12, 1, o, 56, o, o))]),
        "radnet_det_loss": ("det_loss:", [
            ("r = 0", lambda: lib.radnet_det_loss(h, z, z, z, z, 0, 7, 24, o, o)), ("nc = 0", lambda: lib.radnet_det_loss(h, z, z, z, z, 3, 0, 24, o, o)),
            ("nreg < 0", lambda: lib.radnet_det_loss(h, z, z, z, z, 3, 7, -4, o, o))]),
        "radnet_head_tail_fwd": ("head_tail:", [
            ("r = 0", lambda: lib.radnet_head_tail_fwd(h, z, 0, 49, 2048, z, 32, z, 7, 24, o, o, o, z, z, o, o, 1, None, sc)),
            ("hw = 0", lambda: lib.radnet_head_tail_fwd(h, z, 6, 0, 2048, z, 32, z, 7, 24, o, o, o, z, z, o, o, 1, None, sc)),
            ("nc = 0", lambda: lib.radnet_head_tail_fwd(h, z, 6, 49, 2048, z, 32, z, 0, 24, o, o, o, z, z, o, o, 1, None, sc)),
            ("c = 36", lambda: lib.radnet_head_tail_fwd(h, z, 6, 49, 36, z, 32, z, 7, 24, o, o, o, z, z, o, o, 1, None, sc)),
            ("c = 2080", lambda: lib.radnet_head_tail_fwd(h, z, 6, 49, 2080, z, 32, z, 7, 24, o, o, o, z, z, o, o, 1, None, sc)),
            ("r % groups", lambda: lib.radnet_head_tail_fwd(h, z, 6, 49, 2048, z, 32, z, 7, 24, o, o, o, z, z, o, o, 4, None, sc)),
            ("ldw = 48", lambda: lib.radnet_head_tail_fwd(h, z, 6, 49, 2048, z, 48, z, 7, 24, o, o, o, z, z, o, o, 1, None, sc)),
            ("targets without dz", lambda: lib.radnet_head_tail_fwd(h, z, 6, 49, 2048, z, 32, z, 7, 24, o, o, o, z, z, None, o, 1, None, sc))]),
    }


ENTRIES = ("radnet_maxpool_fwd", "radnet_roi_resize_bwd", "radnet_avgpool_fwd", "radnet_avgpool_bwd_relu", "radnet_dense_heads_fwd",
           "radnet_dense_heads_bwd", "radnet_rpn_loss", "radnet_det_loss", "radnet_head_tail_fwd")


@pytest.mark.parametrize("entry", ENTRIES)
def test_refused_arguments_launch_nothing(ctx, entry):
    zeros = torch.zeros(1 << 16, device="cuda")
    out = torch.full((1 << 16,), S_INT, dtype=torch.int32, device="cuda")
    sc = torch.full((1 << 16,), S_INT, dtype=torch.int32, device="cuda")
    table = _refusals(ctx.lib, ctx.h, zeros.data_ptr(), out.data_ptr(), sc.data_ptr())
    assert set(table) == set(ENTRIES)
    prefix, calls = table[entry]
    for what, call in calls:
        rc = call()
        msg = ctx.lib.radnet_last_error(ctx.h)
        assert rc < 0, (entry, what, rc)
        assert msg and msg.decode().startswith(prefix), (entry, what, msg)
    torch.cuda.synchronize()
    assert bool((out == S_INT).all()) and bool((sc == S_INT).all()), (entry, "a refused call wrote to an output or to its scratch")
    test_maxpool(ctx, 0)                                                          # the context still works
