"""The classifier's backward in its deferred weight-gradient form (engine.head_update_deferred: all data gradients, then the weight
gradients of the ten stage-5 convs in one launch per tile shape with Adam #2 in the tile epilogue, the Adam tail, the Winograd filters)
against the paired launches + Adam #2 (RADNET_HEAD_DEFERRED_WGRAD=0): three train steps from the same weights, RNG seed and launch-shape
table give the same losses and the same head state BIT FOR BIT -- kernels, biases, dense heads, both moments, the Winograd filters U of
the three 3x3 convs and the folded shifts.  Ordered reductions make the two programs the same arithmetic in the same order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _batches(n):
    from radnet_hip import synth
    out = []
    for i in range(n):
        meta = synth.synthetic_gt(40 + i, n=6, src_w=1000, src_h=600, smin=60, smax=300)
        out.append([dict(img=synth.synthetic_panel(30 + i, 300, 500), bboxes=meta["bboxes"], width=1000, height=600)])
    return out


def _run(monkeypatch, switch, tune, batches, **ts_kw):
    from faster_rcnn.config import Config
    from oracle import dense
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.trainer import TrainStep
    monkeypatch.setenv("RADNET_HEAD_DEFERRED_WGRAD", switch)
    C = Config()
    C.img_size = 300
    eng = FasterRCNNEngine(C)
    if tune[0] is not None:
        eng.load_tuning(tune[0])                      # same launch shapes -> same summation order
    eng.set_weights(dense.init_params(seed=3))
    calls = {"deferred": 0, "adam_head": 0}
    upd, adam = eng.head_update_deferred, eng.adam

    def spy_upd(*a, **k):
        calls["deferred"] += 1
        return upd(*a, **k)

    def spy_adam(arena, *a, **k):
        calls["adam_head"] += arena is eng.head_arena
        return adam(arena, *a, **k)

    eng.head_update_deferred, eng.adam = spy_upd, spy_adam
    np.random.seed(64)
    ts = TrainStep(eng, **ts_kw)
    losses = []
    for b in batches:
        ts.step(b)
        losses.append(ts.losses())
    ts.flush()
    torch.cuda.synchronize()
    if tune[0] is None:
        import tempfile
        tune[0] = tempfile.mktemp(suffix=".txt")
        eng.save_tuning(tune[0])
    a = eng.head_arena
    state = dict(p=a.p.clone(), m=a.m.clone(), v=a.v.clone(), g=a.g.clone(), shift=eng.head_shift.clone(), t=a.t)
    for name in eng.INFERENCE_WINOGRAD_LAYERS:
        state["U/" + name] = eng.convs[name].wino_u.clone()
    return losses, state, eng.get_weights(), calls, eng.head_bias_off


TUNE = [None]      # one measured launch-shape table for every engine of this module


def test_three_steps_equal_the_paired_program_bit_for_bit(monkeypatch):
    tune = TUNE
    batches = _batches(3)
    l0, s0, w0, c0, _ = _run(monkeypatch, "0", tune, batches)
    l1, s1, w1, c1, bias_off = _run(monkeypatch, "1", tune, batches)
    assert c0 == {"deferred": 0, "adam_head": 3}, c0
    assert c1 == {"deferred": 3, "adam_head": 0}, c1          # the new program ran, in every step
    for i, (a, b) in enumerate(zip(l0, l1)):
        assert a["n_head"] == b["n_head"] == 1, (i, a, b)
        for k in ("rpn_cls", "rpn_regr", "det_cls", "det_regr", "det_acc"):
            assert a[k] == b[k], (i, k, a[k], b[k])
    assert s0["t"] == s1["t"] == 3
    assert any(k.startswith("U/") for k in s0)
    for k in s0:
        if k != "t":
            assert torch.equal(s0[k], s1[k]), (k, float((s0[k] - s1[k]).abs().max()))
    assert not s1["g"].any()                                    # the gradient never travelled through the arena (its tail is cleared by Adam)
    assert s1["m"][:bias_off].abs().max().item() > 0 and s1["v"][:bias_off].abs().max().item() > 0
    for name in w0:
        for k in w0[name]:
            assert np.array_equal(w0[name][k], w1[name][k]), (name, k)


def test_a_deferred_head_update_keeps_the_paired_program(monkeypatch):
    """Adam #2 applied later (TrainStep(defer_head_update=True)): the gradient must exist in the arena, so the old program runs."""
    _, s, _, calls, bias_off = _run(monkeypatch, "1", TUNE, _batches(1), defer_head_update=True)
    assert calls == {"deferred": 0, "adam_head": 1}, calls
    assert s["t"] == 1 and s["m"][:bias_off].abs().max().item() > 0
