"""bf16-mixed training mode (FasterRCNNEngine(precision="bf16-mixed")): bf16 forward convs, fp32 backward and Adam on fp32 masters.

  1. radnet_adam_step_bf16 is bit-identical to Adam followed by radnet_weights_to_bf16 (synthetic ragged layers, the real RPN and
     head arenas, t > 1, grad_scale != 1), keeps the K padding zero, and every rejected argument returns a negative code and
     leaves the buffers untouched;
  2. radnet_conv_fwd_bf16_split on every training-plan shape the split rule splits: within the per-conv bound, reproducible
     across runs and lanes, ksplit = 1 == radnet_conv_fwd_bf16 bit for bit;
  3. one training step against the oracle: within emulation-calibrated bounds of the fp32 oracle and clearly closer to the
     bf16-emulated oracle (tools/bf16_train_emulate.py's arithmetic, computed here on the same sample);
  4. pipelined == call-by-call, fresh engines agree; 5. images follow the masters; 6. end to end; 7. isolation; 8. errors."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _cfg(img_size=600):
    from faster_rcnn.config import Config
    C_ = Config()
    C_.img_size = img_size
    return C_


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def _sample(H, W, k=0):
    from radnet_hip import synth
    meta = synth.synthetic_gt(2 + k, n=5, src_w=2 * W, src_h=2 * H, smin=50, smax=min(H, W))
    return dict(img=synth.synthetic_panel(1 + k, H, W), bboxes=meta["bboxes"], width=2 * W, height=2 * H)


@pytest.fixture(scope="module")
def ctx():
    from radnet_hip import lib as L
    return L.Context(0)


# ------------------------------------------------------------------------------------------------------------ 1. Adam kernel
def _layers_arr(rows):
    from radnet_hip import lib as L
    arr = (L.AdamBf16 * max(len(rows), 1))()
    for k, (off, kk, n, ldw, wt, ldk) in enumerate(rows):
        arr[k].off, arr[k].k, arr[k].n, arr[k].ldw, arr[k].wt, arr[k].ldk = off, kk, n, ldw, wt.data_ptr(), ldk
    return arr


def _adam_both(ctx, state, rows, t, gs, bias=None):
    """(reference state, fused state) after one step from `state` (dict of device tensors; images under 'wt%d')."""
    ref = {k: v.clone() for k, v in state.items()}
    got = {k: v.clone() for k, v in state.items()}
    n = state["p"].numel()
    bo, bl = (bias if bias is not None else (0, 0))
    sh = [ref["scale"], ref["t0"], ref["shift"]] if bias is not None else [None, None, None]
    args = (C.c_int64(n), t, C.c_float(5e-5), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-7), C.c_float(gs), 1)
    if bias is not None:
        ctx.call("radnet_adam_step_affine", ref["p"], ref["g"], ref["m"], ref["v"], *args, C.c_int64(bo), C.c_int64(bl), *sh)
    else:
        ctx.call("radnet_adam_step", ref["p"], ref["g"], ref["m"], ref["v"], *args)
    for j, (off, kk, nn, ldw, ldk) in enumerate(rows):
        ctx.call("radnet_weights_to_bf16", ref["p"][off:], kk, nn, ldw, ref["wt%d" % j], ldk)
    arr = _layers_arr([(off, kk, nn, ldw, got["wt%d" % j], ldk) for j, (off, kk, nn, ldw, ldk) in enumerate(rows)])
    gsh = [got["scale"], got["t0"], got["shift"]] if bias is not None else [None, None, None]
    rc = ctx.lib.radnet_adam_step_bf16(ctx.h, got["p"].data_ptr(), got["g"].data_ptr(), got["m"].data_ptr(), got["v"].data_ptr(), *args,
                                       C.c_int64(bo), C.c_int64(bl), *[x.data_ptr() if x is not None else None for x in gsh], arr, len(rows))
    assert rc == 0, ctx.lib.radnet_last_error(ctx.h)
    torch.cuda.synchronize()
    return ref, got


def _assert_same(ref, got):
    for k in ref:
        assert torch.equal(ref[k].view(torch.int32) if ref[k].dtype == torch.float32 else ref[k],
                           got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k]), k


def _synthetic_state(rs, n, rows, bias_len=0):
    dev = "cuda"
    st = dict(p=torch.from_numpy(rs.randn(n).astype(np.float32) * 0.05).to(dev),
              g=torch.from_numpy(rs.randn(n).astype(np.float32) * 1e-3).to(dev),
              m=torch.from_numpy(rs.randn(n).astype(np.float32) * 1e-4).to(dev),
              v=torch.from_numpy(rs.rand(n).astype(np.float32) * 1e-6).to(dev))
    if bias_len:
        st.update(scale=torch.from_numpy(rs.uniform(0.5, 1.5, bias_len).astype(np.float32)).to(dev),
                  t0=torch.from_numpy(rs.randn(bias_len).astype(np.float32)).to(dev),
                  shift=torch.zeros(bias_len, dtype=torch.float32, device=dev))
    for j, (off, kk, nn, ldw, ldk) in enumerate(rows):
        st["wt%d" % j] = torch.from_numpy(rs.randint(-32768, 32767, (nn, ldk)).astype(np.int16)).to(dev)     # garbage: padding must become 0
    return st


# ragged: k % 32 != 0, n not a multiple of 64, n < ldw, ldk > k rounded up
RAGGED = [(0, 77, 100, 100, 96), (7700, 300, 60, 64, 304), (26900, 9, 8, 8, 40)]
RAGGED_N = 27000 + 256


def test_adam_bf16_bit_identical_synthetic(ctx):
    rs = np.random.RandomState(0)
    st = _synthetic_state(rs, RAGGED_N, RAGGED, bias_len=128)
    for t, gs in ((1, 1.0), (2, 0.5), (3, 0.25)):
        st["g"].copy_(torch.from_numpy(rs.randn(RAGGED_N).astype(np.float32) * 1e-3))
        ref, got = _adam_both(ctx, st, RAGGED, t, gs, bias=(27000, 128))
        _assert_same(ref, got)
        assert not got["g"].any(), "zero_grad"
        for j, (_, kk, _, _, ldk) in enumerate(RAGGED):
            assert not got["wt%d" % j][:, kk:].any(), "K padding must stay zero"
        st = got
    # shift == null: the plain step
    ref, got = _adam_both(ctx, st, RAGGED, 4, 1.0)
    _assert_same(ref, got)


def _engine(img_size=600, **kw):
    from radnet_hip import synth
    from radnet_hip.engine import FasterRCNNEngine
    eng = FasterRCNNEngine(_cfg(img_size), precision="bf16-mixed", **kw)
    eng.set_weights(synth.synthetic_weights(seed=3))
    return eng


@pytest.fixture(scope="module")
def mixed_eng():
    return _engine()


def test_adam_bf16_bit_identical_real_arenas(ctx, mixed_eng):
    eng = mixed_eng
    rs = np.random.RandomState(1)
    for arena, expect in ((eng.rpn_arena, 2), (eng.head_arena, 10)):
        reg = eng.bf16.adam_layers(arena)
        arr, n_l = reg.array, reg.count
        assert n_l == expect
        rows = [(arr[j].off, arr[j].k, arr[j].n, arr[j].ldw, arr[j].ldk) for j in range(n_l)]
        is_head = arena is eng.head_arena
        st = _synthetic_state(rs, arena.n, rows, bias_len=eng.head_bias_len if is_head else 0)
        st["p"].copy_(arena.p)
        for t, gs in ((1, 1.0), (5, 0.5)):
            ref, got = _adam_both(ctx, st, rows, t, gs, bias=(eng.head_bias_off, eng.head_bias_len) if is_head else None)
            _assert_same(ref, got)
            st = got


def test_adam_bf16_rejects_bad_arguments(ctx):
    rs = np.random.RandomState(2)
    st = _synthetic_state(rs, RAGGED_N, RAGGED, bias_len=128)
    before = {k: v.clone() for k, v in st.items()}
    wt = st["wt0"]
    bad = [
        [(RAGGED_N - 100, 77, 100, 100, wt, 96)],                     # outside the arena
        [(0, 77, 100, 100, wt, 96), (400, 9, 8, 8, st["wt2"], 40)],   # overlap
        [(26990, 9, 8, 8, st["wt2"], 40)],                            # overlaps the bias range [27000, 27128)
        [(0, 1, 8, 8, st["wt2"], 8)] * 17,                            # more than 16 layers
        [(2, 77, 100, 100, wt, 96)],                                  # offset not a multiple of 4
        [(0, 77, 100, 100, wt, 92)],                                  # ldk not a multiple of 8
        [(0, 77, 100, 98, wt, 96)],                                   # ldw < n and not a multiple of 4
        [(0, 77, 100, 100, wt, 64)],                                  # ldk < k
    ]
    args = (C.c_int64(RAGGED_N), 1, C.c_float(5e-5), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-7), C.c_float(1.0), 1)
    for rows in bad:
        arr = _layers_arr(rows)
        rc = ctx.lib.radnet_adam_step_bf16(ctx.h, st["p"].data_ptr(), st["g"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(), *args,
                                           C.c_int64(27000), C.c_int64(128), st["scale"].data_ptr(), st["t0"].data_ptr(), st["shift"].data_ptr(),
                                           arr, len(rows))
        assert rc < 0, rows
    # misaligned arena pointer
    rc = ctx.lib.radnet_adam_step_bf16(ctx.h, st["p"].data_ptr() + 4, st["g"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr(),
                                       C.c_int64(RAGGED_N - 4), *args[1:], C.c_int64(0), C.c_int64(0), None, None, None,
                                       _layers_arr([(0, 77, 100, 100, wt, 96)]), 1)
    assert rc < 0
    torch.cuda.synchronize()
    _assert_same(before, st)


# ------------------------------------------------------------------------------------------------------------ 2. split conv
def _training_split_shapes(nb=1):
    from radnet_hip import lib as L
    eng = _engine()
    bp = eng._plan_base(nb, 600, 1000)
    rp = eng._plan_rpn(bp["fh"], bp["fw"], bp["F"], nb=nb)
    hp = eng._plan_head(eng.C.n_rois * nb, bp["fh"], bp["fw"], bp["F"], training=True, groups=nb)
    out = set()
    for kind, d in bp["ops"] + rp["fwd"] + rp["refwd"] + hp["fwd"]:
        assert kind in ("conv_bf16", "maxpool") or (kind == "conv" and d.c == 4), kind
        if kind == "conv_bf16":
            M, N, K = d.nb * d.oh * d.ow, d.n, d.kh * d.kw * d.c
            s = int(L.load_library().radnet_conv_bf16_pick_split(M, N, K))
            if s > 1:
                out.add((d.nb, d.h, d.w_, d.c, d.kh, d.stride, d.pad_t, d.n, d.act, d.act_cols, s))
    return sorted(out)


def _im2col_rows(x, rows, oh, ow, kh, stride, pad):
    nb, h, w, c = x.shape
    img, r = rows // (oh * ow), rows % (oh * ow)
    oy, ox = r // ow, r % ow
    A = np.zeros((len(rows), kh, kh, c), np.float64)
    for ky in range(kh):
        for kx in range(kh):
            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
            ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)
            A[ok, ky, kx, :] = x[img[ok], iy[ok], ix[ok], :]
    return A.reshape(len(rows), -1)


def test_split_conv_every_split_training_shape():
    from radnet_hip import lib as L
    shapes = _training_split_shapes()
    assert shapes, "the split rule splits no training shape at 600x1000, batch 1"
    lanes = []
    for _ in range(2):
        st = torch.cuda.Stream()
        cx = L.Context(0, stream_handle=st.cuda_stream)
        ws = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
        cx.check(cx.lib.radnet_set_workspace(cx.h, ws.data_ptr(), ws.numel()), "set_workspace")
        lanes.append((cx, st, ws))
    for i, (nb, h, w, c, kh, stride, pad, n, act, act_cols, s) in enumerate(shapes):
        rs = np.random.RandomState(10 + i)
        oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kh) // stride + 1
        M, K = nb * oh * ow, kh * kh * c
        ldk = (K + 31) // 32 * 32
        x = rs.randn(nb, h, w, c).astype(np.float32)
        wgt = (rs.randn(K, n) / np.sqrt(K)).astype(np.float32)
        shift = rs.randn(n).astype(np.float32)
        xd, wd, hd = (torch.from_numpy(a).cuda() for a in (x, wgt, shift))
        wt = torch.empty(n, ldk, dtype=torch.int16, device="cuda")
        lanes[0][0].call("radnet_weights_to_bf16", wd, K, n, n, wt, ldk)
        torch.cuda.synchronize()

        def run(lane, ksplit, plain=False):
            cx, st, _ = lanes[lane]
            y = torch.full((M, n), float("nan"), dtype=torch.float32, device="cuda")
            d = L.ConvDesc()
            d.x, d.y, d.shift = xd.data_ptr(), y.data_ptr(), hd.data_ptr()
            d.nb, d.h, d.w_, d.c, d.oh, d.ow, d.kh, d.kw = nb, h, w, c, oh, ow, kh, kh
            d.stride, d.pad_t, d.pad_l, d.n, d.ldw, d.ldy, d.act, d.act_cols = stride, pad, pad, n, n, n, act, act_cols
            if plain:
                rc = cx.lib.radnet_conv_fwd_bf16(cx.h, C.byref(d), wt.data_ptr(), ldk)
            else:
                rc = cx.lib.radnet_conv_fwd_bf16_split(cx.h, C.byref(d), wt.data_ptr(), ldk, ksplit)
            cx.check(rc, "conv_fwd_bf16_split")
            st.synchronize()
            return y.cpu().numpy()

        y_s = run(0, s)
        assert np.array_equal(y_s.view(np.int32), run(0, s).view(np.int32)), "two runs differ"
        assert np.array_equal(y_s.view(np.int32), run(1, s).view(np.int32)), "two lanes differ"
        assert np.array_equal(run(0, 1).view(np.int32), run(0, 0, plain=True).view(np.int32)), "ksplit = 1 is not the one-pass launch"
        rows = np.unique(np.concatenate([rs.choice(M, min(M, 256), replace=False), np.arange(max(0, M - 4), M)]))
        A = _bf16_round(_im2col_rows(x, rows, oh, ow, kh, stride, pad))
        Wb = _bf16_round(wgt)
        dot, absdot = A @ Wb, np.abs(A) @ np.abs(Wb)
        pre = dot + shift
        ref = np.maximum(pre, 0) if act == 1 else pre.copy()
        if act == 2:                                         # sigmoid on the first act_cols columns (the RPN head)
            ref[:, :act_cols] = 1.0 / (1.0 + np.exp(-pre[:, :act_cols]))
        tol = 1e-5 * absdot + 1e-6 * (1.0 + np.abs(shift))
        err = np.abs(y_s[rows].astype(np.float64) - ref)
        assert np.isfinite(y_s).all()
        assert (err <= tol).all(), ((nb, h, w, c, kh, stride, n, s), float((err / tol).max()))


# ------------------------------------------------------------------------------------------------------------ 3. against the oracle
def _arena_grads(eng, arena):
    """Gradient arena in the oracle's {layer: {kernel}} layout (host copy)."""
    out = {}
    for name, c in eng.convs.items():
        if c.dweight is None or not (arena.g.data_ptr() <= c.dweight.data_ptr() < arena.g.data_ptr() + 4 * arena.n):
            continue
        g = c.dweight.detach().cpu().numpy()
        if name == "rpn_heads":
            out["rpn_out_class"] = g[:, :eng.A]
            out["rpn_out_regress"] = g[:, eng.A:5 * eng.A]
        else:
            out[name] = g[:, :c.cout]
    return out


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), 1e-30))


@pytest.mark.parametrize("H,W", [(240, 400), (600, 1000)])
def test_training_step_against_oracle(H, W, monkeypatch):
    import bf16_emulate as E
    from oracle import dense, step as ostep
    from radnet_hip import synth
    from radnet_hip.trainer import TrainStep
    Cc = _cfg(min(H, W))
    Wt = synth.synthetic_weights(seed=3)
    eng = _engine(min(H, W))
    grads = {}
    orig = eng.adam

    def adam(arena, *a, **k):                # the gradient arena before Adam zeroes it
        grads[id(arena)] = _arena_grads(eng, arena)
        return orig(arena, *a, **k)
    monkeypatch.setattr(eng, "adam", adam)
    s = _sample(H, W)
    np.random.seed(64)
    ts = TrainStep(eng)
    ts.capture = []
    ts.step([s])
    got = ts.losses()
    R = ts.capture[0]["R"]
    g_gpu = dict(grads[id(eng.rpn_arena)], **grads.get(id(eng.head_arena), {}))
    monkeypatch.setattr(dense, "conv2d", E.conv2d_torch)
    ref = {}
    try:
        for mode in ("fp32", "bf16"):
            E.MODE[0] = mode
            np.random.seed(64)
            det = {}
            L = ostep.OracleTrainer(Cc, copy.deepcopy(Wt)).step(s, detail=det, override_R=R)
            g = {k: v["kernel"].reshape(-1, v["kernel"].shape[-1]) for k, v in det["g_rpn"].items()}
            g.update({k: v["kernel"].reshape(-1, v["kernel"].shape[-1]) for k, v in (det.get("g_head") or {}).items() if not k.startswith("dense")})
            ref[mode] = (L, g)
    finally:
        E.MODE[0] = "fp32"
    (L32, g32), (L16, g16) = ref["fp32"], ref["bf16"]
    names = ("rpn_cls", "rpn_regr", "det_cls", "det_regr")
    for i, nm in enumerate(names):
        if L32[i] is None:
            continue
        emu = abs(L16[i] - L32[i])
        print("%-9s gpu %.7g  oracle fp32 %.7g  bf16-emulated %.7g" % (nm, got[nm], L32[i], L16[i]))
        assert abs(got[nm] - L32[i]) <= 3 * emu + 2e-3 * abs(L32[i]) + 1e-6, (nm, got[nm], L32[i], L16[i])
    to32, to16 = [], []
    for name in g32:
        emu = _rel(g32[name], g16[name])
        d32, d16 = _rel(g32[name], g_gpu[name]), _rel(g16[name], g_gpu[name])
        print("%-20s emulated %.3e  gpu-fp32 %.3e  gpu-bf16emu %.3e" % (name, emu, d32, d16))
        assert d32 <= 3 * emu + 1e-4, (name, d32, emu)
        to32.append(d32)
        to16.append(d16)
    # the mode really computes in bf16: layer by layer the gradients are closer to the bf16 emulation than to fp32 (measured: median
    # ratio 0.5-0.6; not near 0 -- the fp32 backward runs on activations whose bf16 rounding flips with the forward's summation
    # order).  The losses do not separate the two at the reduced panel (GPU-vs-oracle spread there ~ the bf16 effect, 2e-4).
    assert np.median(np.array(to16) / np.array(to32)) < 0.8, (to16, to32)


# ------------------------------------------------------------------------------------------------------------ 4. / 5. reproducibility, images
def _images_match(eng):
    for im in eng.bf16.fwd.values():
        c, ref = im.conv, torch.empty_like(im.wt)
        eng.ctx.call("radnet_weights_to_bf16", c.weight, c.kh * c.kh * c.cin, im.n, c.ldw, ref, im.ldk)
        torch.cuda.synchronize()
        assert torch.equal(ref, im.wt), c.name


def _run_steps(batches, prefetch, tune, defer=None):
    from radnet_hip import synth
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.trainer import TrainStep
    eng = FasterRCNNEngine(_cfg(300), precision="bf16-mixed")
    if tune[0] is not None:
        eng.load_tuning(tune[0])
    eng.set_weights(synth.synthetic_weights(seed=3))
    np.random.seed(64)
    ts = TrainStep(eng, defer_head_update=defer)
    ts.stack_base = False
    losses = []
    for k, b in enumerate(batches):
        ts.step(b, upcoming=batches[k + 1:k + 4] if prefetch else None)
        losses.append(ts.losses())
    ts.flush()
    torch.cuda.synchronize()
    if tune[0] is None:
        import tempfile
        tune[0] = tempfile.mktemp(suffix=".txt")
        eng.save_tuning(tune[0])
    images = {im.conv.name: im.wt.cpu().numpy().copy() for im in eng.bf16.fwd.values()}
    return eng, losses, eng.get_weights(), images


@pytest.mark.parametrize("per_batch", [1, 2])
def test_pipelined_equals_call_by_call_and_images_follow(per_batch):
    from radnet_hip import synth
    batches = []
    for i in range(4):
        b = []
        for j in range(per_batch):
            meta = synth.synthetic_gt(40 + 2 * i + j, n=6, src_w=1000, src_h=600, smin=60, smax=300)
            b.append(dict(img=synth.synthetic_panel(30 + 2 * i + j, 300, 500), bboxes=meta["bboxes"], width=1000, height=600))
        batches.append(b)
    tune = [None]
    e0, l0, w0, i0 = _run_steps(batches, False, tune)
    _images_match(e0)
    e1, l1, w1, i1 = _run_steps(batches, True, tune)
    _images_match(e1)
    e2, l2, w2, i2 = _run_steps(batches, False, tune)            # a fresh engine with the same table
    assert l0 == l1 == l2
    for k in w0:
        for kk in w0[k]:
            assert np.array_equal(w0[k][kk], w1[k][kk]) and np.array_equal(w0[k][kk], w2[k][kk]), k
    assert i0.keys() == i1.keys() == i2.keys()
    assert all(np.array_equal(i0[k], i1[k]) and np.array_equal(i0[k], i2[k]) for k in i0)
    assert all(np.isfinite(v) for l in l0 for v in l.values() if v is not None)
    # deferred head update (the data-parallel schedule) then flush(): images still follow their masters
    e3, _, _, _ = _run_steps(batches, True, tune, defer=True)
    _images_match(e3)
    # set_weights rewrites every image
    e3.set_weights(synth.synthetic_weights(seed=5))
    _images_match(e3)


# ------------------------------------------------------------------------------------------------------------ 6. end to end
AUG = ("use_horizontal_flips", "use_vertical_flips", "use_90_rotations", "use_rotations", "use_shear", "use_brightness", "use_noise")


def test_fit_validate_and_save_load(tmp_path):
    from faster_rcnn import data_feed, models as M
    from radnet_hip import fit as F, synth
    from radnet_hip.trainer import TrainStep
    C_ = _cfg(300)
    C_.tile_size, C_.tile_overlap, C_.balanced_classes = 300, 150, False
    for k in AUG:
        setattr(C_, k, False)
    m_rpn, m_cls, m_all, _, _ = M.build_models(C_, precision="bf16-mixed")
    eng = m_all._s.eng
    data, imgs = [], {}
    for i in range(2):
        meta = synth.synthetic_gt(50 + i, n=6, src_w=600, src_h=450, smin=60, smax=200)
        data.append(dict(filepath="img_%d.png" % i, width=600, height=450, bboxes=meta["bboxes"]))
        imgs["img_%d.png" % i] = synth.synthetic_panel(60 + i, 450, 600)
    class_count = {}
    for d in data:
        for b in d["bboxes"]:
            class_count[b["class"]] = class_count.get(b["class"], 0) + 1
    np.random.seed(3)
    feed = iter(data_feed.TileFeed(data, C_, class_count, lambda d, t: imgs[d["filepath"]], rng=np.random.RandomState(9)))
    ts = TrainStep(eng)
    record = tmp_path / "record.csv"
    val = [_sample(300, 500, k) for k in range(2)]
    rows, _ = F.fit(ts, feed, epochs=1, epoch_length=3, val_samples=val, weights_path=str(tmp_path / "w.h5"), record_path=str(record))
    assert record.exists() and rows
    losses = ts.read_loss_log() if hasattr(ts, "read_loss_log") else None
    assert losses is None or np.isfinite(losses).all()
    rec = ts.validate(val)
    assert all(np.isfinite(v) for k, v in rec.items() if isinstance(v, float))
    path = str(tmp_path / "mixed.h5")
    m_all.save_weights(path)
    _, _, a32, _, _ = M.build_models(_cfg(300))
    a32.load_weights(path, by_name=True)
    w_mixed, w32 = eng.get_weights(), a32._s.eng.get_weights()
    for k in w_mixed:
        for kk in w_mixed[k]:
            assert np.array_equal(w_mixed[k][kk], w32[k][kk]), k
    # and back into a bf16-mixed engine: the images are rewritten
    _, _, a16, _, _ = M.build_models(_cfg(300), precision="bf16-mixed")
    e16 = a16._s.eng
    e16.bf16.adam_layers(e16.rpn_arena)
    e16.bf16.adam_layers(e16.head_arena)                     # the trainable images exist before the load
    a16.load_weights(path, by_name=True)
    _images_match(a16._s.eng)


# ------------------------------------------------------------------------------------------------------------ 7. isolation
def test_fp32_and_bf16_unaffected_by_a_mixed_engine():
    from faster_rcnn import models as M
    from faster_rcnn.RADNet import RADNet
    from faster_rcnn.base_models import resnet50
    from radnet_hip import synth
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.trainer import TrainStep
    b = [[_sample(300, 500, k)] for k in range(2)]

    tune = [None]

    def fp32_steps():
        eng = FasterRCNNEngine(_cfg(300))
        if tune[0] is not None:
            eng.load_tuning(tune[0])              # same launch shapes -> same summation order
        eng.set_weights(synth.synthetic_weights(seed=3))
        np.random.seed(64)
        ts = TrainStep(eng)
        out = []
        for x in b:
            ts.step(x)
            out.append(ts.losses())
        ts.flush()
        if tune[0] is None:
            import tempfile
            tune[0] = tempfile.mktemp(suffix=".txt")
            eng.save_tuning(tune[0])
        return out, eng.get_weights()

    W = synth.synthetic_weights(seed=3)
    C2 = _cfg()
    _, _, _, r3, dt = M.build_models(C2, weights=copy.deepcopy(W), workload="predict", precision="bf16")
    net = RADNet(C2, r3, dt, resnet50.preprocess)
    tile = np.random.RandomState(21).randint(0, 256, (900, 900, 3)).astype(np.uint8)
    before_pred = net._detect(tile)
    l_a, w_a = fp32_steps()
    mixed = _engine(300)
    ts = TrainStep(mixed)
    ts.step(b[0])
    ts.flush()
    l_b, w_b = fp32_steps()
    assert l_a == l_b
    assert all(np.array_equal(w_a[k][kk], w_b[k][kk]) for k in w_a for kk in w_a[k])
    assert net._detect(tile) == before_pred
    # the bf16 inference engine's ops keep the one-pass launch
    from radnet_hip import lib as L
    eng16 = r3._s.eng
    bp = eng16._plan_base(1, 600, 600)
    arr = eng16._compile(bp["ops"])
    kinds = [arr[k].kind for k in range(len(bp["ops"]))]
    assert L.OP_CONV_FWD_BF16 in kinds
    assert all(arr[k].i[1] == 0 for k in range(len(bp["ops"])) if arr[k].kind == L.OP_CONV_FWD_BF16)


# ------------------------------------------------------------------------------------------------------------ 8. errors
def test_errors(mixed_eng):
    from faster_rcnn import models as M
    from radnet_hip.engine_cont import ContEngine
    from radnet_hip.native import NativeTrainStep
    with pytest.raises(NotImplementedError):
        NativeTrainStep(mixed_eng)
    with pytest.raises(NotImplementedError):
        ContEngine(_cfg(), precision="bf16-mixed")
    Cv = _cfg()
    Cv.network = "vgg16"
    with pytest.raises(NotImplementedError):
        M.build_models(Cv, precision="bf16-mixed")
