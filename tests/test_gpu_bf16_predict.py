"""bf16 inference mode of the ResNet50 predict path (FasterRCNNEngine(precision="bf16"), csrc/conv_bf16.hip):

  * radnet_weights_to_bf16 is bit-exact round-to-nearest-even (torch's CPU cast), transposed, zero K padding;
  * radnet_conv_fwd_bf16 on every conv shape of the bf16 predict plan (600x600 tile, 300 RoIs) plus ragged shapes, against a
    CPU fp64 reference on bf16-rounded operands -- with operands built so that the UNROUNDED product misses the bound (the test
    tells a bf16 kernel from an fp32 one);
  * network level against the fp32 engine, within bounds calibrated by tools/bf16_emulate.py (CPU emulation of the same
    arithmetic: F 4.9e-3, RPN 3.3e-3, classifier 2.3e-3 at 600x600 / 300 RoIs; bounds >= 3x those);
  * every path of the bf16 mode agrees bit for bit (device-resident / NumPy-facing, _detect_all / _detect, radnet_predict_tile /
    model calls, runs, engines), weights follow set_weights, fp32 results do not move when a bf16 engine exists;
  * errors: unknown precision, VGG16, training on a bf16 engine."""
import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from derived_state import fwd_image_bits  # noqa: E402  (the layout statement of the forward image, shared with the auditor)

# calibrated with tools/bf16_emulate.py ("bf16 inference mode"): measured x >= 3
BOUND_F_REL = 1.5e-2
BOUND_RPN = 1.0e-2
BOUND_CLS = 7.0e-3


def _cfg(img_size=600):
    from faster_rcnn.config import Config
    C_ = Config()
    C_.img_size = img_size
    return C_


def _tile(seed=4, size=2048):
    return np.random.RandomState(seed).randint(0, 256, (size, size, 3)).astype(np.uint8)


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


@pytest.fixture(scope="module")
def ctx():
    from radnet_hip import lib as L
    return L.Context(0)


# ------------------------------------------------------------------------------------------------------------ 1. cast
def test_weights_to_bf16_bit_exact_transposed_zero_padded(ctx):
    rs = np.random.RandomState(0)
    K, N, ldw, ldk = 77, 40, 48, 96
    w = (rs.randn(K, ldw) * 10.0 ** rs.uniform(-30, 30, (K, ldw))).astype(np.float32)
    bits = w.view(np.uint32)
    sign = rs.randint(0, 2, (K, ldw)).astype(np.uint32) << 31
    bits[0:8] = (rs.randint(0x3f80, 0x4f80, (8, ldw)).astype(np.uint32) << 16) | 0x8000 | sign[0:8]     # exact ties, even and odd
    bits[8:12] = rs.randint(1, 0x7fffff, (4, ldw)).astype(np.uint32) | sign[8:12]                       # subnormals
    bits[12:14] = (0x7f7f0000 + rs.randint(0, 0x10000, (2, ldw))).astype(np.uint32) | sign[12:14]       # near FLT_MAX (some -> inf)
    bits[14] = 0x00008000 | sign[14]                                                                     # smallest subnormal tie
    assert np.isfinite(w).all()
    wd = torch.from_numpy(w).cuda()
    wt = torch.full((N, ldk), 0x1234, dtype=torch.int16, device="cuda")
    ctx.call("radnet_weights_to_bf16", wd, K, N, ldw, wt, ldk)
    torch.cuda.synchronize()
    got = wt.cpu().numpy().view(np.uint16)
    ref = fwd_image_bits(w, N)
    assert np.array_equal(got[:, :K], ref)
    assert not got[:, K:].any(), "K padding must be zero"


# ------------------------------------------------------------------------------------------------------------ 2. conv parity
def _biased(rs, shape, scale=1.0):
    """Half the values in (1 + 2^-9, 1 + 2^-8) -- bf16 rounds every one of them DOWN -- the rest normal; scale: a power of two."""
    v = rs.uniform(1 + 2.0 ** -9, 1 + 2.0 ** -8, shape)
    return (np.where(rs.rand(*shape) < 0.5, v, rs.randn(*shape)) * scale).astype(np.float32)


def _plan_shapes():
    """Distinct conv shapes of the bf16 predict plan for a 600x600 tile and 300 RoIs."""
    from radnet_hip.engine import FasterRCNNEngine
    eng = FasterRCNNEngine(_cfg(), precision="bf16", workload="predict")
    bp = eng._plan_base(1, 600, 600)
    rp = eng._plan_rpn(bp["fh"], bp["fw"], bp["F"])
    hp = eng._plan_head(300, bp["fh"], bp["fw"], bp["F"], training=False)
    shapes = set()
    for kind, d in bp["ops"] + rp["fwd"] + hp["fwd"]:
        assert kind in ("conv_bf16", "maxpool") or (kind == "conv" and d.c == 4), kind
        if kind == "conv_bf16":
            shapes.add((d.nb, d.h, d.w_, d.c, d.kh, d.stride, d.pad_t, d.n, 2 if d.act == 2 else 1, d.act_cols))
    return sorted(shapes)


RAGGED = [(2, 13, 11, 24, 3, 2, 1, 100, 1, 0),      # ragged M and N, padding taps, stride 2
          (1, 9, 7, 8, 1, 1, 0, 33, 0, 0),          # C = 8, no activation
          (3, 5, 5, 40, 7, 1, 3, 70, 2, 20),        # 7x7, K = 1960 (K padding inside the last tile), sigmoid columns
          (1, 31, 29, 64, 3, 1, 1, 130, 1, 0)]


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


def _act(v, act, act_cols):
    if act == 1:
        return np.maximum(v, 0)
    if act == 2:
        v = v.copy()
        v[:, :act_cols] = 1.0 / (1.0 + np.exp(-v[:, :act_cols]))
    return v


def _check_shape(ctx, shape, seed):
    from radnet_hip import lib as L
    nb, h, w, c, kh, stride, pad, n, act, act_cols = shape
    rs = np.random.RandomState(seed)
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kh) // stride + 1
    M, K = nb * oh * ow, kh * kh * c
    ldw, ldk = n + 3, (K + 31) // 32 * 32 + 8
    x = _biased(rs, (nb, h, w, c))
    wgt = _biased(rs, (K, ldw), 2.0 ** -int(round(np.log2(np.sqrt(K)))))
    scale = rs.uniform(0.5, 1.5, n).astype(np.float32)
    shift = rs.randn(n).astype(np.float32)
    addend = rs.randn(M, n).astype(np.float32)
    xd, wd = torch.from_numpy(x).cuda(), torch.from_numpy(wgt).cuda()
    sd, hd, ad = torch.from_numpy(scale).cuda(), torch.from_numpy(shift).cuda(), torch.from_numpy(addend).cuda()
    y = torch.full((M, n), float("nan"), dtype=torch.float32, device="cuda")
    wt = torch.empty(n, ldk, dtype=torch.int16, device="cuda")
    ctx.call("radnet_weights_to_bf16", wd, K, n, ldw, wt, ldk)
    d = L.ConvDesc()
    d.x, d.w, d.y, d.scale, d.shift, d.addend = xd.data_ptr(), None, y.data_ptr(), sd.data_ptr(), hd.data_ptr(), ad.data_ptr()
    d.nb, d.h, d.w_, d.c, d.oh, d.ow = nb, h, w, c, oh, ow
    d.kh = d.kw = kh
    d.stride, d.pad_t, d.pad_l, d.n = stride, pad, pad, n
    d.ldw, d.ldy, d.ld_add, d.act, d.act_cols = ldw, n, n, act, act_cols
    ctx.check(ctx.lib.radnet_conv_fwd_bf16(ctx.h, C.byref(d), wt.data_ptr(), ldk), "radnet_conv_fwd_bf16")
    torch.cuda.synchronize()
    rows = np.unique(np.concatenate([rs.choice(M, min(M, 384), replace=False), np.arange(max(0, M - 8), M)]))
    yg = y.cpu().numpy()[rows].astype(np.float64)
    A = _im2col_rows(x, rows, oh, ow, kh, stride, pad)
    W = wgt[:, :n].astype(np.float64)
    Ab, Wb = _bf16_round(A), _bf16_round(W)
    dot_b, dot_u, absdot = Ab @ Wb, A @ W, np.abs(Ab) @ np.abs(Wb)
    tail = shift.astype(np.float64) + addend[rows].astype(np.float64)
    ref = _act(dot_b * scale + tail, act, act_cols)
    ref_u = _act(dot_u * scale + tail, act, act_cols)
    tol = 1e-5 * absdot * scale + 1e-6 * (1.0 + np.abs(tail))
    assert np.isfinite(yg).all(), shape
    err = np.abs(yg - ref)
    assert (err <= tol).all(), (shape, float((err / tol).max()))
    # the unrounded product is outside the bound: an fp32-operand kernel would fail this test
    assert (np.abs(ref_u - ref) > tol).any(), shape


def test_conv_bf16_parity_every_plan_shape(ctx):
    shapes = _plan_shapes()
    assert any(s[4] == 3 for s in shapes) and any(s[4] == 1 and s[5] == 2 for s in shapes) and any(s[8] == 2 for s in shapes)
    assert any(s[0] * s[1] * s[2] // s[5] ** 2 == 14700 for s in shapes), shapes          # the classifier convs at M = 300 x 49
    for i, s in enumerate(shapes):
        _check_shape(ctx, s, 100 + i)


@pytest.mark.parametrize("shape", RAGGED)
def test_conv_bf16_parity_ragged(ctx, shape):
    _check_shape(ctx, shape, 7)


def test_conv_bf16_deterministic(ctx):
    """Two launches of one problem give the same bits."""
    from radnet_hip import lib as L
    rs = np.random.RandomState(1)
    x = torch.from_numpy(rs.randn(2, 14, 14, 512).astype(np.float32)).cuda()
    w = torch.from_numpy(rs.randn(9 * 512, 256).astype(np.float32)).cuda()
    wt = torch.empty(256, 9 * 512, dtype=torch.int16, device="cuda")
    ctx.call("radnet_weights_to_bf16", w, 9 * 512, 256, 256, wt, 9 * 512)
    outs = []
    for _ in range(2):
        y = torch.empty(2 * 196, 256, dtype=torch.float32, device="cuda")
        d = L.ConvDesc()
        d.x, d.y = x.data_ptr(), y.data_ptr()
        d.nb, d.h, d.w_, d.c, d.oh, d.ow, d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.n = 2, 14, 14, 512, 14, 14, 3, 3, 1, 1, 1, 256
        d.ldw, d.ldy, d.act = 256, 256, 1
        ctx.check(ctx.lib.radnet_conv_fwd_bf16(ctx.h, C.byref(d), wt.data_ptr(), 9 * 512), "radnet_conv_fwd_bf16")
        outs.append(y.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------ network level
def _engine_outputs(eng, X, rois):
    """(F, RPN head matrix, classifier softmax) of one preprocessed input through the engine's programs, on given RoIs."""
    bp = eng.upload_preprocessed(X)
    eng.base_forward(bp)
    rp = eng.rpn_forward(bp)
    hp = eng._plan_head(rois.shape[0], bp["fh"], bp["fw"], bp["F"], training=False)
    hp["rois"].copy_(torch.from_numpy(rois))
    eng.head_forward(hp)
    torch.cuda.synchronize()
    return bp["F"].cpu().numpy().copy(), rp["pred"].cpu().numpy().copy(), hp["pcls"].cpu().numpy().copy()


@pytest.fixture(scope="module")
def nets():
    from faster_rcnn import models as M
    from faster_rcnn.RADNet import RADNet
    from faster_rcnn.base_models import resnet50
    from radnet_hip import synth
    W = synth.synthetic_weights(seed=3)
    out = {}
    for prec in ("fp32", "bf16"):
        C_ = _cfg()
        m_rpn, m_cls, m_all, m_rpn3, m_det = M.build_models(C_, weights=copy.deepcopy(W), workload="predict", precision=prec)
        out[prec] = dict(C=C_, rpn=m_rpn, cls=m_cls, rpn3=m_rpn3, det=m_det, eng=m_all._s.eng, net=RADNet(C_, m_rpn3, m_det, resnet50.preprocess))
    return out


def test_network_bf16_against_fp32_within_calibrated_bounds(nets):
    from faster_rcnn import rpn
    n32, n16 = nets["fp32"], nets["bf16"]
    X, _ = n32["net"].format_img(_tile())
    Y1, Y2, F32 = n32["rpn3"].predict(X)
    R = rpn.rpn_to_roi(Y1, Y2, n32["C"], overlap_thresh=0.7)[:300].astype(np.float32)
    R[:, 2] -= R[:, 0]
    R[:, 3] -= R[:, 1]
    A = n32["eng"].A
    F_a, pred_a, pc_a = _engine_outputs(n32["eng"], X, R)
    F_b, pred_b, pc_b = _engine_outputs(n16["eng"], X, R)
    rel = np.linalg.norm((F_b - F_a).astype(np.float64)) / np.linalg.norm(F_a.astype(np.float64))
    d_rpn = np.abs(pred_b[:, :A].astype(np.float64) - pred_a[:, :A]).max()
    d_cls = np.abs(pc_b.astype(np.float64) - pc_a).max()
    print("bf16 vs fp32: F rel %.3e, RPN %.3e, classifier %.3e" % (rel, d_rpn, d_cls))
    assert 0 < rel <= BOUND_F_REL
    assert d_rpn <= BOUND_RPN
    assert d_cls <= BOUND_CLS


# ------------------------------------------------------------------------------------------------------------ 4. paths agree
def test_bf16_paths_agree_bit_for_bit(nets):
    net = nets["bf16"]["net"]
    tiles = [_tile(40 + i) for i in range(3)]
    net.device_resident = True
    d_dev = net._detect(tiles[0])
    net.device_resident = False
    d_np = net._detect(tiles[0])
    net.device_resident = True
    assert d_dev == d_np
    one_by_one = [net._detect(t) for t in tiles]
    assert net._detect_all(tiles) == one_by_one
    assert net._detect(tiles[0]) == d_dev                       # second run of the same engine


def test_bf16_predict_tile_composed_equals_model_calls(nets):
    from faster_rcnn import rpn
    from faster_rcnn.base_models import resnet50
    from radnet_hip import native
    n16 = nets["bf16"]
    img = np.random.RandomState(11).randint(0, 256, (600, 640, 3)).astype(np.uint8)
    R, pc, pr = native.predict_tile(n16["eng"], torch.from_numpy(img).cuda(), 40)
    X = resnet50.preprocess(img[:, :, (2, 1, 0)].astype(np.float32)[None])
    Y1, Y2, F = n16["rpn3"].predict(X)
    R_ref = rpn.rpn_to_roi(Y1, Y2, n16["C"], overlap_thresh=0.7)
    assert np.array_equal(R, R_ref)
    rois = R_ref[:40].copy()
    rois[:, 2] -= rois[:, 0]
    rois[:, 3] -= rois[:, 1]
    pc_ref, pr_ref = n16["det"].predict([F, rois[None]])
    assert np.array_equal(pc, pc_ref[0]) and np.array_equal(pr, pr_ref[0])


def test_bf16_fresh_engines_agree_and_weights_follow(nets):
    from radnet_hip import synth
    from radnet_hip.engine import FasterRCNNEngine
    n16 = nets["bf16"]
    X, _ = n16["net"].format_img(_tile(9))
    rois = np.array([[2, 3, 10, 12], [0, 0, 37, 37], [20, 5, 7, 30]], np.float32)
    W3, W5 = synth.synthetic_weights(seed=3), synth.synthetic_weights(seed=5)
    e1 = FasterRCNNEngine(_cfg(), precision="bf16", workload="predict")
    e1.set_weights(W3)
    a = _engine_outputs(e1, X, rois)
    e2 = FasterRCNNEngine(_cfg(), precision="bf16", workload="predict")
    e2.set_weights(W3)
    b = _engine_outputs(e2, X, rois)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert all(np.array_equal(u, v) for u, v in zip(a, _engine_outputs(n16["eng"], X, rois)))
    # 5. set_weights(W5) on a used engine == a fresh engine built with W5
    e1.set_weights(W5)
    c = _engine_outputs(e1, X, rois)
    e3 = FasterRCNNEngine(_cfg(), precision="bf16", workload="predict")
    e3.set_weights(W5)
    d = _engine_outputs(e3, X, rois)
    assert all(np.array_equal(u, v) for u, v in zip(c, d))
    assert not np.array_equal(a[0], c[0])


def test_fp32_unaffected_by_a_bf16_engine():
    from faster_rcnn import models as M
    from faster_rcnn.RADNet import RADNet
    from faster_rcnn.base_models import resnet50
    from radnet_hip import synth
    W = synth.synthetic_weights(seed=3)
    C_ = _cfg()
    _, _, _, m_rpn3, m_det = M.build_models(C_, weights=copy.deepcopy(W), workload="predict")
    net = RADNet(C_, m_rpn3, m_det, resnet50.preprocess)
    tile = _tile(21)
    before = net._detect(tile)
    C2 = _cfg()
    _, _, _, b_rpn3, b_det = M.build_models(C2, weights=copy.deepcopy(W), workload="predict", precision="bf16")
    RADNet(C2, b_rpn3, b_det, resnet50.preprocess)._detect(tile)
    assert net._detect(tile) == before


# ------------------------------------------------------------------------------------------------------------ 7. errors
def test_precision_errors(nets):
    from faster_rcnn import models as M
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.trainer import TrainStep
    with pytest.raises(ValueError):
        FasterRCNNEngine(_cfg(), precision="fp16")
    with pytest.raises(ValueError):
        M.build_models(_cfg(), precision="fp16")
    Cv = _cfg()
    Cv.network = "vgg16"
    with pytest.raises(NotImplementedError):
        M.build_models(Cv, precision="bf16")
    n16 = nets["bf16"]
    X = np.zeros((1, 64, 64, 3), np.float32)
    with pytest.raises(RuntimeError, match="inference only"):
        n16["rpn"].train_on_batch(X, [None, None])
    with pytest.raises(RuntimeError, match="inference only"):
        n16["rpn"].test_on_batch(X, [None, None])
    with pytest.raises(RuntimeError, match="inference only"):
        n16["cls"].train_on_batch([X, np.zeros((1, 1, 4))], [None, None])
    with pytest.raises(RuntimeError, match="inference only"):
        TrainStep(n16["eng"])
    with pytest.raises(RuntimeError, match="inference only"):
        n16["eng"].adam(n16["eng"].rpn_arena)


# ------------------------------------------------------------------------------------------------------------ 8. end to end
def test_radnet_predict_bf16_two_tile_panel(nets):
    from faster_rcnn.RADNet import _spans
    net, C_ = nets["bf16"]["net"], nets["bf16"]["C"]
    panel = np.random.RandomState(12).randint(0, 256, (2000, 2400, 3)).astype(np.uint8)
    assert len(_spans(2000, C_.tile_size, C_.tile_overlap)) * len(_spans(2400, C_.tile_size, C_.tile_overlap)) == 2
    d1 = net.predict([panel])
    d2 = net.predict([panel])
    assert isinstance(d1, list)
    for det in d1:
        assert set(det) == {"class", "prob", "x1", "y1", "x2", "y2"}
    assert repr(d1) == repr(d2)
