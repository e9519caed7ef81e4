"""Every device buffer the engines derive from their trainable weights (folded shifts, Winograd filters, bf16 forward and dgrad images;
DESIGN.md 5, 'Derived copies of the trainable weights') audited by tests/derived_state.py after every path that changes the weights, in
eight engines at img_size = 300:

  fp32 (Adam #2 rewrites the classifier's Winograd filters), fp32-lazy (RADNET_NO_HEAD_TRAIN_WINOGRAD=1: they follow lazily, through
  sync_inference_filters), bf16, bf16-mixed, bf16-train, cont (ContEngine), cont-direct (its S34_WINOGRAD off) and vgg (VGG16Engine).

  1. set_weights, and set_weights again with other weights: clean, and bit for bit the buffers of a freshly built engine;
  2. ONE adam() / adam_s34() per arena with nothing behind it: what that launch claims (shifts when fused, U when wino, images when
     mixed -- read off adam()'s branches) is clean with no excuse; after the trainers' follow-up calls everything is; three more steps
     with zero_grad=False;
  3. adam(head_arena) WITHOUT a refresh, then set_weights / models.load_weights of other weights: the shifts fold the loaded biases;
  4. refresh_head_shift() twice after Adam and twice without: the flag that makes the first a no-op is never left set;
  5. head_forward / head_backward(defer_wgrad=True) / head_update_deferred on 8 RoIs of a 1 x 8 x 9 x 1024 map (both fp32 engines);
  6. one whole step of every trainer an engine supports on one 300 x 500 sample (TrainStep alone and with an announced batch,
     NativeTrainStep, ContTrainStep), audited as an inference entry point would find it;
  7. bf16-train: dgrad images created AFTER the first adam() enter the arena's registry (at most 16) and follow the next one; a forward
     image of an arena cannot be created late, adam_layers() makes them all;
  8. stepping one engine changes no record of another engine's audit.

Gradients are synthetic (arena.g.normal_(0, 1e-2)): a step moves every weight by about lr, 2e-5 or more, against bounds of 2^-23
relative.  The module-scoped engines are restored (weights, moments, gradients) behind every test.

What the audit found, on the engines as they were (one run of this module, the product fixes taken out; 17 of 61 cases failed):
  * sequence 3, every engine with folded shifts, through set_weights and through load_weights -- "fp32: adam(head_arena), no refresh,
    set_weights(P2): 10 of 26 derived buffers are stale or misplaced: [Record(layer='res5a_branch2a', kind='shift',
    worst=200286717.0, n_wrong=512, excused=False), Record(layer='res5a_branch2b', kind='shift', worst=349688088.9, n_wrong=512, ...":
    refresh_head_shift() consumed _head_shift_fresh whoever called it; set_weights() now calls refresh_head_shift(force=True);
  * sequences 1 and 3 on the VGG16 engine -- "set_weights(P2): 1 of 5 ...: [Record(layer='rpn_conv1', kind='wino_u',
    worst=2967669151805.8, n_wrong=9437180, ...": its set_weights() did not re-transform rpn_conv1's filter; it does now;
  * sequences 2 and 6 on cont-direct -- "one Adam launch of the s34/rpn arena: 10 of 42 ...: [Record(layer='res3a_branch2b',
    kind='wino_u', worst=38904947.3, n_wrong=589818, ...": set_weights() made transformed filters of the stage-3/4 3x3 convs that no
    program read and no adam_s34() rewrote; with S34_WINOGRAD off these layers now hold none (test 0 counts them).

Measured on one MI355X: the module takes 75 s, most of it the sixteen engines (eight under test, their eight fresh twins) and the float64
filter references on the host (1.1 s for rpn_conv1, 0.35 s for each 512 x 512 layer, recomputed only when that layer's weights changed);
the slowest case is test_adam_on_each_arena[fp32-head] with 3.4 s (3.2 s for [cont-head] in another run), test_weight_load[fp32] takes
3.1 s, test_deferred_head_update[fp32] 2.9 s, every whole step under 2.2 s."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import derived_state as D  # noqa: E402

KINDS = ("fp32", "fp32-lazy", "bf16", "bf16-mixed", "bf16-train", "cont", "cont-direct", "vgg")
TRAINABLE = tuple(k for k in KINDS if k != "bf16")
FP32 = ("fp32", "fp32-lazy")
H, W_ = 300, 500
_ENGINES, _FRESH, _PARAMS = {}, {}, {}


# ---------------------------------------------------------------------------------------------------------------- engines
def _cfg(kind):
    from faster_rcnn.config import Config
    C = Config()
    C.img_size = 300
    if kind == "vgg":
        C.network = "vgg16"
        C.anchor_box_scales = [128, 256, 512]
    return C


def params(kind, seed):
    """Weights of `kind`'s network: seed 3 / 4 (ResNet50), 5 / 6 (VGG16) for P / P2; made once."""
    net = "vgg" if kind == "vgg" else "resnet"
    if (net, seed) not in _PARAMS:
        from oracle import dense, vgg
        _PARAMS[net, seed] = vgg.init_params(seed=seed + 2, n_anchors=9) if net == "vgg" else dense.init_params(seed=seed)
    return _PARAMS[net, seed]


def _build(kind):
    from radnet_hip import make_engine
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.engine_cont import ContEngine
    with pytest.MonkeyPatch.context() as mp:              # the knobs are read at construction
        mp.delenv("RADNET_NO_HEAD_TRAIN_WINOGRAD", raising=False)
        if kind == "fp32-lazy":
            mp.setenv("RADNET_NO_HEAD_TRAIN_WINOGRAD", "1")
        if kind == "vgg":
            eng = make_engine(_cfg(kind))
        elif kind == "cont":
            eng = ContEngine(_cfg(kind))
        elif kind == "cont-direct":
            eng = type("ContEngineDirect", (ContEngine,), dict(S34_WINOGRAD=False))(_cfg(kind))     # the attribute, read wherever it is used
        else:
            eng = FasterRCNNEngine(_cfg(kind), precision="fp32" if kind in FP32 else kind)
    eng.set_weights(params(kind, 3))
    return eng


def _warm(kind, eng):
    """The plans of one 300 x 500 step and of an inference head: every buffer the programs read exists from here on."""
    bp = eng._plan_base(1, H, W_, 0)
    rp = eng._plan_rpn(bp["fh"], bp["fw"], bp["F"])
    eng._plan_head(8, bp["fh"], bp["fw"], bp["F"], training=False)
    if kind != "bf16":
        eng._plan_head(eng.C.n_rois, bp["fh"], bp["fw"], bp["F"])
    torch.cuda.synchronize()
    return bp, rp


def engine(kind):
    if kind not in _ENGINES:
        eng = _build(kind)
        _warm(kind, eng)
        assert eng.head_train_wino == (kind == "fp32")
        assert (eng.precision != "fp32") == kind.startswith("bf16")
        _ENGINES[kind] = eng
    return _ENGINES[kind]


def fresh(kind, seed):
    """A second engine of `kind`, built anew, holding the weights of `seed` and nothing any sequence did."""
    if kind not in _FRESH:
        _FRESH[kind] = _build(kind)
    _FRESH[kind].set_weights(params(kind, seed))
    return _FRESH[kind]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _ENGINES.clear(); _FRESH.clear(); _PARAMS.clear(); D._WINO_CACHE.clear()


def arenas(eng):
    """[(name, arena, step)]: every optimizer of the engine; step(zero_grad) is ONE Adam launch of it with whatever it folds in."""
    out = [("rpn", eng.rpn_arena, lambda z=True: eng.adam(eng.rpn_arena, zero_grad=z)),
           ("head", eng.head_arena, lambda z=True: eng.adam(eng.head_arena, zero_grad=z))]
    if hasattr(eng, "s34_arena"):
        out += [("s34/rpn", eng.s34_arena, lambda z=True: eng.adam_s34(0)), ("s34/cls", eng.s34_arena, lambda z=True: eng.adam_s34(1))]
    return out


def layers_of(eng, arena):
    lo = arena.p.data_ptr()
    return [n for n, c in eng.convs.items() if c.weight is not None and lo <= c.weight.data_ptr() < lo + 4 * arena.n]


def claimed(eng, name, arena):
    """The kinds of buffer ONE Adam launch of `arena` rewrites itself (engine.adam / engine_cont.adam_s34, branch by branch)."""
    kinds = []
    if name != "head" or eng.head_bias_len == 0 or (eng.head_bias_off % 4 == 0 and eng.head_bias_len % 4 == 0):
        kinds.append("shift")            # fused into the launch (head, s34), refreshed right behind it (s34 without U), or the bias itself
    if eng.precision == "fp32" and (name != "head" or eng.head_train_wino):
        kinds.append("wino_u")           # rpn_conv1 behind Adam #1, the classifier's and stages 3/4's in Adam's epilogue
    if eng.precision != "fp32":
        kinds += ["bf16_fwd", "bf16_dgrad"]
    return tuple(kinds)


def restore(kind, eng):
    torch.cuda.synchronize()
    eng.set_weights(params(kind, 3))
    for _, ar, _ in arenas(eng):
        ar.g.zero_(); ar.m.zero_(); ar.v.zero_(); ar.t = 0
        if hasattr(ar, "m2"):
            ar.m2.zero_(); ar.v2.zero_(); ar.t2 = 0
    eng.sync_inference_filters()
    torch.cuda.synchronize()


def clean(eng, what, **kw):
    rec = D.assert_clean(D.audit(eng, **kw), what)
    assert rec, what
    return rec


def no_excuse(rec, what):
    assert not any(r.excused for r in rec), (what, [r for r in rec if r.excused])
    return rec


def _sample(k=0):
    from radnet_hip import synth
    meta = synth.synthetic_gt(2 + k, n=6, src_w=1000, src_h=600, smin=60, smax=300)
    return dict(img=synth.synthetic_panel(1 + k, H, W_), bboxes=meta["bboxes"], width=1000, height=600)


# ---------------------------------------------------------------------------------------------------------------- 0. what is audited
@pytest.mark.parametrize("kind", KINDS)
def test_the_auditor_finds_the_buffers_of_this_engine(kind):
    eng = engine(kind)
    have = collections_count(D.derived_buffers(eng))
    names = list(eng.convs)
    if kind == "vgg":
        assert have == dict(shift=4, wino_u=1), have                        # rpn_conv1, rpn_heads, fc1, fc2: the bias itself; rpn_conv1's U
    elif kind.startswith("cont"):
        s34 = [n for n in names if n.startswith(("res3", "res4"))]
        assert have["shift"] == 2 + 10 + len(s34) and have["wino_u"] == (1 + 3 + 10 if kind == "cont" else 1 + 3), have
    elif kind in FP32:
        assert have == dict(shift=12, wino_u=1 + 10 + 3), have             # rpn_conv1, the frozen stage-3/4 3x3, the classifier's 3x3
    else:
        n8 = [n for n, c in eng.convs.items() if c.cin % 8 == 0]
        assert have["shift"] == 12 and "wino_u" not in have and have["bf16_fwd"] == len(n8) == len(names) - 1, have
        assert ("bf16_dgrad" in have) == (kind == "bf16-train"), have
    if kind != "vgg":                                                      # the convs' views tile the whole folded vector
        assert sum(eng.convs[n].cout for n in eng.head_conv_names) == eng.head_shift.numel() == eng.head_bias_len
        assert all(eng.convs[n].shift.data_ptr() == eng.head_shift.data_ptr() + 4 * (eng.head_arena.offsets[n + "/bias"][0] - eng.head_bias_off)
                   for n in eng.head_conv_names)
    if kind.startswith("cont"):
        assert sum(eng.convs[n].cout for n in eng.s34_names) == eng.s34_shift.numel()


def collections_count(bufs):
    out = {}
    for b in bufs:
        out[b.kind] = out.get(b.kind, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. weight load
@pytest.mark.parametrize("kind", KINDS)
def test_weight_load(kind):
    eng = engine(kind)
    try:
        eng.set_weights(params(kind, 3))
        no_excuse(clean(eng, "set_weights(P)", inference=True), kind)
        eng.set_weights(params(kind, 4))
        no_excuse(clean(eng, "set_weights(P2)"), kind)
        assert D.assert_same_as_fresh(eng, fresh(kind, 4)) == len(D.derived_buffers(eng))
    finally:
        restore(kind, eng)


# ---------------------------------------------------------------------------------------------------------------- 2. Adam, arena by arena
def _arena_names(kind):
    return ("rpn", "head") + (("s34/rpn", "s34/cls") if kind.startswith("cont") else ())


@pytest.mark.parametrize("kind,which", [(k, a) for k in TRAINABLE for a in _arena_names(k)])
def test_adam_on_each_arena(kind, which):
    eng = engine(kind)
    name, arena, step = [a for a in arenas(eng) if a[0] == which][0]
    mine = layers_of(eng, arena)
    try:
        what = "%s: one Adam launch of the %s arena" % (kind, name)
        arena.g.normal_(0, 1e-2)
        step()
        rec = no_excuse(clean(eng, what, kinds=claimed(eng, name, arena), layers=mine), what)
        assert {r.kind for r in rec} == set(claimed(eng, name, arena)) & {b.kind for b in D.derived_buffers(eng) if b.layer in mine}, what
        rec = clean(eng, what + ", every buffer")                    # the other arenas' buffers did not move, nor did they need to
        lazy = sorted(r.layer for r in rec if r.excused)
        assert lazy == (sorted(eng.INFERENCE_WINOGRAD_LAYERS) if (kind != "fp32" and eng.precision == "fp32" and name == "head" and kind != "vgg")
                        else []), (what, lazy)                        # fp32-lazy / cont: the classifier's U waits for the next inference pass
        eng.refresh_head_shift()                                     # the trainers' follow-up calls
        eng.sync_inference_filters()
        no_excuse(clean(eng, what + " + refresh_head_shift + sync_inference_filters"), what)
        what = "%s: three more Adam launches of the %s arena, zero_grad=False" % (kind, name)
        arena.g.normal_(0, 1e-2)
        for _ in range(3):
            step(False)
            if not arena.g.any():                                    # adam_s34 always clears
                arena.g.normal_(0, 1e-2)
        no_excuse(clean(eng, what, kinds=claimed(eng, name, arena), layers=mine), what)
        eng.refresh_head_shift()
        no_excuse(clean(eng, what + " + follow-up", inference=True), what)
    finally:
        restore(kind, eng)


# ---------------------------------------------------------------------------------------------------------------- 3. Adam, no refresh, then a load
def _model(eng, weights):
    """faster_rcnn.models' weight file front end around an engine that exists already."""
    from faster_rcnn import models as M
    s = M._Shared.__new__(M._Shared)
    s.C, s.eng, s.W, s._x_key, s._bp, s._f_host = eng.C, eng, copy.deepcopy(weights), None, None, None
    return M._ModelBase(s)


@pytest.mark.parametrize("kind,via", [(k, v) for k in TRAINABLE for v in ("set_weights", "load_weights")
                                      if (k, v) != ("vgg", "load_weights")])       # (VGG16 folds nothing: one load path is enough for 0.5 GB of fc1)
def test_adam_without_refresh_then_a_weight_load(kind, via, tmp_path):
    eng = engine(kind)
    try:
        if via == "load_weights":
            eng.set_weights(params(kind, 4))
            _model(eng, params(kind, 4)).save_weights(tmp_path / "p2")
            eng.set_weights(params(kind, 3))
        eng.head_arena.g.normal_(0, 1e-2)
        eng.adam(eng.head_arena)                                     # ... and no refresh_head_shift() behind it
        if via == "set_weights":
            eng.set_weights(params(kind, 4))
        else:
            _model(eng, params(kind, 3)).load_weights(tmp_path / "p2")
        no_excuse(clean(eng, "%s: adam(head_arena), no refresh, %s(P2)" % (kind, via)), kind)
        D.assert_same_as_fresh(eng, fresh(kind, 4))
    finally:
        restore(kind, eng)


# ---------------------------------------------------------------------------------------------------------------- 4. repeated refresh
@pytest.mark.parametrize("kind", TRAINABLE)
def test_repeated_refresh(kind):
    eng = engine(kind)
    try:
        eng.head_arena.g.normal_(0, 1e-2)
        eng.adam(eng.head_arena)
        for k in range(2):
            eng.refresh_head_shift()
            clean(eng, "%s: refresh_head_shift() #%d after Adam" % (kind, k + 1), kinds=("shift",))
        assert not eng._head_shift_fresh
        bias = eng.convs[eng.head_conv_names[0]].bias
        bias += 1e-3                                                 # written some other way: the next refresh must fold it
        for k in range(2):
            eng.refresh_head_shift()
            clean(eng, "%s: refresh_head_shift() #%d without Adam" % (kind, k + 1), kinds=("shift",))
        assert not eng._head_shift_fresh
    finally:
        restore(kind, eng)


# ---------------------------------------------------------------------------------------------------------------- 5. deferred head update
@pytest.mark.parametrize("kind", FP32)
def test_deferred_head_update(kind):
    eng = engine(kind)
    R = 8
    try:
        F = torch.relu(torch.randn(1, 8, 9, 1024, device="cuda", generator=torch.Generator("cuda").manual_seed(3)))
        hp = eng._plan_head(R, 8, 9, F)
        rs = np.random.RandomState(2)
        rois = np.stack([rs.randint(0, 5, R), rs.randint(0, 4, R), rs.randint(1, 4, R), rs.randint(1, 4, R)], 1).astype(np.float32)
        hp["rois"].copy_(torch.from_numpy(rois))
        hp["y1"].zero_(); hp["y2"].zero_()
        hp["y1"].view(R, -1)[:, 0] = 1
        eng.head_forward(hp, training=True, loss_out=eng.det_losses)
        eng.set_accumulate(hp["bwd"], False, prezeroed=True)
        assert eng.head_deferred_ok(hp)
        eng.head_backward(hp, accumulate=True, loss_out=eng.det_losses, defer_wgrad=True)
        before = eng.head_arena.p.clone()
        eng.head_update_deferred(hp)
        torch.cuda.synchronize()
        assert eng.head_arena.t == 1 and not torch.equal(before, eng.head_arena.p) and bool(torch.isfinite(eng.head_arena.p).all())
        what = "%s: head_update_deferred" % kind
        rec = clean(eng, what)
        assert sorted(r.layer for r in rec if r.excused) == ([] if eng.head_train_wino else sorted(eng.INFERENCE_WINOGRAD_LAYERS)), what
        no_excuse(clean(eng, what + ", inference", inference=True), what)
    finally:
        restore(kind, eng)


# ---------------------------------------------------------------------------------------------------------------- 6. whole steps
def _trainers(kind):
    if kind.startswith("cont"):
        return ("cont",)
    return ("pipelined", "announced") + (("native",) if kind in FP32 else ())


@pytest.mark.parametrize("kind,trainer", [(k, t) for k in TRAINABLE for t in _trainers(k)])
def test_one_whole_step(kind, trainer):
    eng = engine(kind)
    try:
        np.random.seed(64)
        before = eng.rpn_arena.p.clone()
        if trainer == "native":
            from radnet_hip.native import NativeTrainStep
            ts = NativeTrainStep(eng)
            ts.step(_sample())
            heads = [ts.losses()["n_head"]]
        elif trainer == "cont":
            from radnet_hip.trainer_cont import ContTrainStep
            ts = ContTrainStep(eng)
            ts.step([_sample()])
            heads = [ts.losses()["n_head"]]
        else:
            from radnet_hip.trainer import TrainStep
            ts = TrainStep(eng)
            b0, b1 = [_sample(0)], [_sample(1)]
            heads = []
            if trainer == "announced":
                ts.step(b0, upcoming=[b1])
                heads.append(ts.losses()["n_head"])
                ts.step(b1)
            else:
                ts.step(b0)
            heads.append(ts.losses()["n_head"])
            ts.flush()
        torch.cuda.synchronize()
        what = "%s: one step of the %s trainer (head batches %s)" % (kind, trainer, heads)
        assert not torch.equal(before, eng.rpn_arena.p), what
        if not any(heads):                                           # the early exit: the classifier's buffers stay as they were, coherent
            clean(eng, what + ", head buffers", layers=layers_of(eng, eng.head_arena))
        no_excuse(clean(eng, what, inference=True), what)
    finally:
        restore(kind, eng)


# ---------------------------------------------------------------------------------------------------------------- 7. images created late
def test_bf16_train_images_created_after_the_first_adam():
    eng = _build("bf16-train")
    assert not eng.bf16.fwd and not eng.bf16.dgrad and not eng.bf16.dgrad_arena
    for _, arena, step in arenas(eng):
        arena.g.normal_(0, 1e-2)
        step()
    # adam_layers() made the forward image of every conv of the arena: one of them created later cannot occur
    for _, arena, _ in arenas(eng):
        mine = [n for n in layers_of(eng, arena) if eng.convs[n].cin % 8 == 0]
        assert eng.bf16.adam[id(arena)].count == len(mine) and all(eng.convs[n].weight.data_ptr() in eng.bf16.fwd for n in mine)
    made = set(eng.bf16.fwd)
    assert not eng.bf16.dgrad
    no_excuse(clean(eng, "bf16-train: Adam before any plan"), "")
    _warm("bf16-train", eng)                                         # the backward programs create the dgrad images, and the frozen base its forward images
    assert eng.bf16.dgrad and set(eng.bf16.fwd) > made
    trainable = {eng.convs[n].weight.data_ptr() for _, a, _ in arenas(eng) for n in layers_of(eng, a)}
    assert not (set(eng.bf16.fwd) - made) & trainable
    for _, arena, _ in arenas(eng):
        reg = eng.bf16.dgrad_arena.get(id(arena))
        mine = {eng.convs[n].weight.data_ptr() for n in layers_of(eng, arena)}
        assert (reg.count if reg else 0) == len(mine & set(eng.bf16.dgrad)) <= 16
    no_excuse(clean(eng, "bf16-train: images created after Adam"), "")
    for name, arena, step in arenas(eng):
        arena.g.normal_(0, 1e-2)
        step()
        what = "bf16-train: Adam of the %s arena after its dgrad images were created" % name
        no_excuse(clean(eng, what, kinds=claimed(eng, name, arena), layers=layers_of(eng, arena)), what)
    no_excuse(clean(eng, "bf16-train: every buffer after the second Adam"), "")


# ---------------------------------------------------------------------------------------------------------------- 8. two engines
def test_two_engines_do_not_touch_each_other():
    a, b = engine("fp32"), engine("bf16-mixed")
    try:
        for mover, kind, other in ((a, "fp32", b), (b, "bf16-mixed", a)):
            before = D.audit(other)
            bits = [t.tensor.clone() for t in D.derived_buffers(other)]
            for name, arena, step in arenas(mover):
                arena.g.normal_(0, 1e-2)
                step()
            mover.refresh_head_shift()
            no_excuse(clean(mover, "%s stepped beside another engine" % kind, inference=True), kind)
            assert D.audit(other) == before
            assert all(torch.equal(x, t.tensor) for x, t in zip(bits, D.derived_buffers(other)))
            D.assert_clean(before)
    finally:
        restore("fp32", a)
        restore("bf16-mixed", b)
