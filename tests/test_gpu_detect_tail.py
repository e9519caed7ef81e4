"""The detection tail on the device (csrc/detect_tail.hip) against the host code it stands in for, on the SAME tensors:
RADNet._spp_chunks + _spp_decode + _per_class_nms (and, as a second opinion that needs no device, oracle.glue.spp_decode +
greedy_nms + real_coords).  Equal means: the same class keys in the same order, the same integer boxes in the same order,
probabilities equal as fp32 bits.

The host gets the RoIs as the int64 array the tile path hands it (np.float32 deltas times np.int64 sizes are fp64 products;
with float32 RoIs NumPy would multiply in fp32), the device the same integers as fp32.

Device exp() is within 1 ulp of libm's, so a value within 1 ulp of a half before round() could round differently: the
constructed cases stay away from halves by construction, the random cases assert a distance of 1e-9 from the host's own
pre-rounding values and drop the (very unlikely) draws inside that band -- at least 95 % of the draws must remain."""
import copy
import ctypes as C

import numpy as np
import pytest

from test_detect_tail_host import RATIOS, floor_divide_restated

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STD = (8.0, 8.0, 4.0, 4.0)


@pytest.fixture(scope="module")
def ctx():
    from radnet_hip import lib as L
    return L.Context(0)


@pytest.fixture(scope="module")
def net():
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    Cc = Config()
    assert list(Cc.classifier_regr_std) == list(STD) and Cc.n_rois == 20 and Cc.rpn_stride == 16
    return RADNet(Cc, None, None, None)


# ------------------------------------------------------------------------------------------------------------ helpers
def device_tail(ctx, p_cls, p_regr, rois, n, k, ratio, thr=0.7, nms=0.2, max_boxes=300):
    """radnet_detect_tail alone -> the raw int32 words on the host."""
    from radnet_hip import engine as E
    from radnet_hip import lib as L
    rows, nc = p_cls.shape
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p_cls.astype(np.float32), p_regr.astype(np.float32), rois.astype(np.float32))]
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    out = torch.full((int(ctx.lib.radnet_detect_tail_out_bytes(rows)) // 4,), -7, dtype=torch.int32, device="cuda")
    d = L.DetectTailDesc()
    d.p_cls, d.p_regr, d.rois, d.n = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n_dev.data_ptr()
    d.rows, d.nc, d.k, d.bg = rows, nc, k, nc - 1
    d.bbox_threshold = E.threshold_f32(thr)
    d.regr_std[:] = STD
    d.rpn_stride, d.nms_thresh, d.ratio, d.max_boxes = 16.0, nms, ratio, max_boxes
    d.out = out.data_ptr()
    ctx.check(ctx.lib.radnet_detect_tail(ctx.h, C.byref(d)), "radnet_detect_tail")
    return out.cpu().numpy()


def as_dict(net, words):
    from radnet_hip.engine import read_detections
    cls, boxes, probs = read_detections(words)
    out = {}
    for c, b, p in zip(cls.tolist(), boxes.tolist(), probs):
        real, pr = out.setdefault(net.class_mapping[c], ([], []))
        real.append(tuple(b))
        pr.append(p)
    return out


def padded_rois(net, R, rows):
    """The RoIs of the head plan: _spp_chunks' rows, then rows the tail must not look at."""
    chunks = net._spp_chunks(R)
    rois = np.concatenate(chunks, axis=1)[0].astype(np.float32) if chunks else np.zeros((0, 4), np.float32)
    return chunks, np.concatenate([rois, np.zeros((rows - rois.shape[0], 4), np.float32)])


def host_tail(net, p_cls, p_regr, R, ratio):
    """The yardstick: today's host path on the same tensors."""
    k = net.C.n_rois
    chunks = net._spp_chunks(R)
    outs = [(p_cls[None, i * k:(i + 1) * k], p_regr[None, i * k:(i + 1) * k]) for i in range(len(chunks))]
    return net._per_class_nms(*net._spp_decode(chunks, outs), ratio)


def oracle_tail(net, p_cls, p_regr, R, ratio):
    """Second opinion, NumPy only."""
    from oracle import glue
    k, at = net.C.n_rois, [0]

    def det(rois):
        i = at[0]
        at[0] += k
        return p_cls[None, i:i + k], p_regr[None, i:i + k]

    bb, pp = glue.spp_decode(R, det, net.C, net.bbox_threshold)
    out = {}
    for key in bb:
        nb, npr = glue.greedy_nms(np.array(bb[key]), np.array(pp[key]), 0.2, 300)
        out[key] = ([glue.real_coords(ratio, *nb[j]) for j in range(nb.shape[0])], [npr[j] for j in range(nb.shape[0])])
    return out


def same(a, b):
    assert list(a) == list(b), (list(a), list(b))
    for key in a:
        assert [tuple(int(v) for v in box) for box in a[key][0]] == [tuple(int(v) for v in box) for box in b[key][0]], key
        pa, pb = np.array(a[key][1], dtype=np.float32), np.array(b[key][1], dtype=np.float32)
        assert pa.dtype == np.float32 and np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), key


def half_distance(net, p_cls, p_regr, R, thr):
    """Smallest distance to a half of any value the host rounds (rpn.py:370-375), over the rows it decodes."""
    k = net.C.n_rois
    chunks = net._spp_chunks(R)
    rois = np.concatenate(chunks, axis=1)[0].astype(np.float64)
    m = rois.shape[0]
    best = np.argmax(p_cls[:m], axis=1)
    keep = ~(np.max(p_cls[:m], axis=1) < np.float32(thr)) & (best != p_cls.shape[1] - 1)
    dist = 1.0
    for i in np.nonzero(keep)[0]:
        t = [np.float64(p_regr[i, 4 * best[i] + q] / np.float32(STD[q])) for q in range(4)]
        x, y, w, h = rois[i]
        with np.errstate(all="ignore"):
            w1, h1 = np.exp(t[2]) * w, np.exp(t[3]) * h
            vals = np.array([t[0] * w + (x + w / 2.) - w1 / 2., t[1] * h + (y + h / 2.) - h1 / 2., w1, h1])
        vals = vals[np.isfinite(vals) & (np.abs(vals) < 1e15)]
        if len(vals):
            dist = min(dist, float(np.min(np.abs(np.abs(vals - np.floor(vals)) - 0.5))))
    return dist


def draw(seed, rows, n, nc=7, sharp=3.0, spread=0.15):
    """Benign tensors: every row a proper softmax, integer RoIs inside a 38 x 38 map, moderate deltas."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((rows, nc)) * sharp
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p_cls = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    p_regr = (rs.standard_normal((rows, 4 * (nc - 1))) * spread * np.tile(STD, nc - 1)).astype(np.float32)
    R = np.stack([rs.randint(0, 30, n), rs.randint(0, 30, n), rs.randint(2, 13, n), rs.randint(2, 13, n)], axis=1).astype(np.int64)
    return p_cls, p_regr, R


def check(ctx, net, p_cls, p_regr, R, rows, ratio=300 / 2048, thr=0.7, oracle=True, band=True):
    """Device == host (== oracle) for one case; returns the detections.  Rows past ceil(n/k)*k hold a box of zero size with
    score 1: looking at them would report a malformed box."""
    net.bbox_threshold = thr
    n, k = R.shape[0], net.C.n_rois
    chunks, rois = padded_rois(net, R, rows)
    m = len(chunks) * k
    p_cls, p_regr = p_cls.copy(), p_regr.copy()
    p_cls[m:] = 0.0
    p_cls[m:, 0] = 1.0
    if band:
        assert half_distance(net, p_cls, p_regr, R, thr) > 1e-9
    got = as_dict(net, device_tail(ctx, p_cls, p_regr, rois, n, k, ratio, thr))
    ref = host_tail(net, p_cls, p_regr, R, ratio)
    same(got, ref)
    if oracle:
        same(got, oracle_tail(net, p_cls, p_regr, R, ratio))
    return got


def one_hot(p_cls, i, c, s):
    """Row i: class c with score s, the rest spread evenly over the other classes (each below s)."""
    nc = p_cls.shape[1]
    p_cls[i] = np.float32((1.0 - float(s)) / (nc - 1))
    p_cls[i, c] = s


# ------------------------------------------------------------------------------------------------------------ 1. the kernel alone
def test_first_maximum_threshold_and_background(ctx, net):
    p_cls, p_regr, R = draw(1, 20, 20)
    s = np.float32(0.7)
    below, above = np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1))
    for i in range(20):
        one_hot(p_cls, i, 6, 0.9)                              # background: dropped
    one_hot(p_cls, 2, 1, below)
    one_hot(p_cls, 3, 1, s)                                    # np.float32(0.7) < 0.7 is False: kept
    one_hot(p_cls, 4, 1, above)
    p_cls[5] = [0.0, 0.0, 0.45, 0.0, 0.45, 0.1, 0.0]           # equal maxima: the first; below 0.7
    R[:, 0], R[:, 1] = np.arange(20) * 30, 0                   # boxes apart: nothing is suppressed
    got = check(ctx, net, p_cls, p_regr, R, 20)
    assert list(got) == [net.class_mapping[1]] and len(got[net.class_mapping[1]][0]) == 2
    assert sorted(np.array(got[net.class_mapping[1]][1]).view(np.uint32).tolist()) == sorted([s.view(np.uint32), above.view(np.uint32)])
    # threshold 0.4: row 5's first maximum (class 2, not 4) and rows 2-4 survive
    p_cls[6] = [0.0, 0.0, 0.0, 0.45, 0.0, 0.1, 0.45]           # equal with the background: class 3 comes first
    got = check(ctx, net, p_cls, p_regr, R, 20, thr=0.4)
    assert list(got) == [net.class_mapping[1], net.class_mapping[2], net.class_mapping[3]]
    # no surviving row at all
    for i in range(20):
        one_hot(p_cls, i, 0, 0.5)
    assert check(ctx, net, p_cls, p_regr, R, 20) == {}


@pytest.mark.parametrize("rows,n", [(20, 1), (20, 13), (40, 21), (300, 299), (300, 300), (300, 33), (1000, 987), (1000, 1000)])
@pytest.mark.parametrize("ratio", RATIOS)
def test_padding_rows_sizes_and_ratios(ctx, net, rows, n, ratio):
    """n not a multiple of k (the padding rows are copies of their chunk's first RoI but carry their OWN scores and deltas, and
    are decoded like the others), n = 1, n = rows, rows = 20 / 300 / 1000; resize ratios including 0.1, where Python's floor
    division is not floor(v / ratio)."""
    p_cls, p_regr, R = draw(100 + rows + n, rows, n)
    got = check(ctx, net, p_cls, p_regr, R, rows, ratio=ratio, thr=0.5)
    assert len(got) > 1 or n == 1
    if ratio == 0.1 and got:
        # the device restates the fmod-based division: the coordinates are those of the restatement, not of floor(v / ratio)
        net.bbox_threshold = 0.5
        k = net.C.n_rois
        chunks = net._spp_chunks(R)
        bb, pp = net._spp_decode(chunks, [(p_cls[None, i * k:(i + 1) * k], p_regr[None, i * k:(i + 1) * k]) for i in range(len(chunks))])
        allowed = {int(v) for key in bb for v in np.rint(floor_divide_restated(np.array(bb[key], dtype=np.float64).ravel(), 0.1))}
        assert all(v in allowed for key in got for box in got[key][0] for v in box)


def test_one_class_every_class_and_ties(ctx, net):
    # one class only
    p_cls, p_regr, R = draw(7, 300, 300)
    for i in range(300):
        one_hot(p_cls, i, 2, np.float32(0.71 + 0.001 * (i % 97)))
    got = check(ctx, net, p_cls, p_regr, R, 300)
    assert list(got) == [net.class_mapping[2]]
    # every class, in an order that is neither ascending nor descending: keys come in order of first surviving row
    order = [4, 0, 5, 2, 1, 3]
    for i in range(300):
        one_hot(p_cls, i, order[(i // 3) % 6] if i >= 2 else 6, np.float32(0.75 + 0.0005 * i))
    got = check(ctx, net, p_cls, p_regr, R, 300)
    assert list(got) == [net.class_mapping[c] for c in order]
    # equal scores within a class: "stable ascending, walk from the end" = the higher row first
    p_cls, p_regr, R = draw(8, 40, 40)
    p_regr[:] = 0.0                                            # boxes stay where the RoIs are
    for i in range(40):
        one_hot(p_cls, i, i % 2, np.float32(0.8))
        R[i] = (i // 2 % 5) * 3, (i // 10) * 9, 8, 8           # heavy overlaps inside each class
    got = check(ctx, net, p_cls, p_regr, R, 40, ratio=1.0)
    first = got[net.class_mapping[0]][0][0]
    assert first == (16 * R[38, 0], 16 * R[38, 1], 16 * (R[38, 0] + 8), 16 * (R[38, 1] + 8))      # row 38: the last row of class 0


def test_overflow_nan_and_degenerate_boxes(ctx, net):
    from radnet_hip.engine import read_detections
    p_cls, p_regr, R = draw(9, 20, 20)
    for i in range(20):
        one_hot(p_cls, i, 1, np.float32(0.9 - 0.01 * i))
        R[i] = 8 * (i % 10), 14 * (i // 10), 4, 5
    p_regr[3, 4 * 1 + 2] = 800.0 * 4.0                          # tw = 800: math.exp overflows -> the RoI itself
    p_regr[4, 4 * 1 + 0] = np.nan                               # NaN reaches round() -> the RoI itself
    p_regr[5, 4 * 1 + 3] = np.inf                               # exp(inf) = inf reaches round() -> the RoI itself
    p_regr[6, 4 * 1 + 2] = -np.inf                              # exp(-inf) = 0: no error, a width of 0 ... on row 6 only
    p_cls[6] = p_cls[0]
    one_hot(p_cls, 6, 6, 0.9)                                   # ... which is background here
    with np.errstate(all="ignore"):
        got = check(ctx, net, p_cls, p_regr, R, 20, ratio=1.0, thr=0.0, band=False)
    boxes = got[net.class_mapping[1]][0]
    for i in (3, 4, 5):
        x, y, w, h = (int(v) for v in R[i])
        assert (16 * x, 16 * y, 16 * (x + w), 16 * (y + h)) in boxes
    # a delta that rounds a width to 0: the reference asserts, the tail reports -1, the host side raises the same error
    p_cls, p_regr, R = draw(10, 20, 20)
    one_hot(p_cls, 11, 3, 0.95)
    R[11] = 5, 5, 1, 6
    p_regr[11, 4 * 3 + 2] = np.float32(np.log(0.3) * 4.0)       # w1 = 0.3 -> 0
    net.bbox_threshold = 0.7
    chunks, rois = padded_rois(net, R, 20)
    words = device_tail(ctx, p_cls, p_regr, rois, 20, 20, 1.0)
    assert words[0] == -1
    with pytest.raises(AssertionError):
        read_detections(words)
    with pytest.raises(AssertionError):
        host_tail(net, p_cls, p_regr, R, 1.0)


def test_random_cases(ctx, net):
    kept = drawn = with_boxes = 0
    for seed in range(300):
        rs = np.random.RandomState(5000 + seed)
        rows = (20, 300, 1000)[seed % 3]
        n = int(rs.randint(1, rows + 1))
        thr = (0.0, 0.5, 0.7)[seed // 3 % 3]
        ratio = RATIOS[seed % 4]
        p_cls, p_regr, R = draw(seed, rows, n, sharp=float(rs.uniform(1.0, 4.0)), spread=float(rs.uniform(0.02, 0.2)))
        drawn += 1
        m = (n + 19) // 20 * 20
        if half_distance(net, p_cls[:m], p_regr[:m], R, thr) <= 1e-9:
            continue
        kept += 1
        try:
            net.bbox_threshold = thr
            ref = host_tail(net, p_cls, p_regr, R, ratio)
        except AssertionError:                                  # a width rounded to 0 somewhere: both sides must say so
            chunks, rois = padded_rois(net, R, rows)
            assert device_tail(ctx, p_cls, p_regr, rois, n, 20, ratio, thr)[0] == -1
            continue
        got = check(ctx, net, p_cls, p_regr, R, rows, ratio=ratio, thr=thr, oracle=seed % 10 == 0)
        with_boxes += bool(got)
    assert kept >= 0.95 * drawn and with_boxes >= drawn // 3, (kept, with_boxes, drawn)


# ------------------------------------------------------------------------------------------------------------ 2. RoI builder
@pytest.mark.parametrize("n", [1, 19, 20, 21, 299, 300])
def test_rois_from_proposals_equals_spp_chunks(ctx, net, n):
    rs = np.random.RandomState(n)
    R = np.zeros((1024, 4), dtype=np.int64)
    R[:, :2] = rs.randint(0, 30, (1024, 2))
    R[:, 2:] = R[:, :2] + rs.randint(1, 12, (1024, 2))
    Rd = torch.from_numpy(R).cuda()
    nd = torch.tensor([n], dtype=torch.int32, device="cuda")
    xywh = R[:n].copy()
    xywh[:, 2] -= xywh[:, 0]
    xywh[:, 3] -= xywh[:, 1]
    want = np.concatenate(net._spp_chunks(xywh), axis=1)[0].astype(np.float32)
    for rows in (want.shape[0], 320):
        out = torch.full((rows, 4), -1.0, dtype=torch.float32, device="cuda")
        ctx.call("radnet_rois_from_proposals", Rd, nd, 1024, 20, rows, out)
        got = out.cpu().numpy()
        assert np.array_equal(got[:want.shape[0]], want)
        assert np.array_equal(got[want.shape[0]:], np.broadcast_to(want[0], (rows - want.shape[0], 4)))


# ------------------------------------------------------------------------------------------------------------ 3. end to end
def _models(network="resnet50", precision="fp32"):
    from faster_rcnn import models as M
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    Cc = Config()
    Cc.img_size = 300
    if network == "vgg16":
        from faster_rcnn.base_models import vgg16 as base
        Cc.network = "vgg16"
        Cc.anchor_box_scales = [128, 256, 512]
        ms = M.build_models(Cc, workload="predict")
    else:
        from faster_rcnn.base_models import resnet50 as base
        from oracle import dense
        kw = {} if precision == "fp32" else dict(precision=precision)
        ms = M.build_models(Cc, weights=copy.deepcopy(dense.init_params(seed=3)), workload="predict", **kw)
    return Cc, ms, RADNet(Cc, ms[3], ms[4], base.preprocess)


@pytest.fixture(scope="module")
def fp32_net():
    return _models()


def _tile(seed, shape):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def _end_to_end(rnet, shapes, tiles):
    assert rnet.device_resident and rnet._tail_on_device() == rnet.device_tail
    n_boxes = 0
    for thr in (0.0, 0.7):
        rnet.bbox_threshold = thr
        for shape in shapes:
            tile = _tile(sum(shape), shape)
            rnet.device_tail = True
            assert rnet._tail_on_device()
            a = rnet._detect(tile)
            rnet.device_tail = False
            same(a, rnet._detect(tile))
            n_boxes += sum(len(v[0]) for v in a.values()) if thr == 0.0 else 0
    assert n_boxes > 0
    rnet.bbox_threshold = 0.0
    rnet.device_tail = True
    piped = rnet._detect_all(tiles)
    one = [rnet._detect(t) for t in tiles]
    rnet.device_tail = False
    host = rnet._detect_all(tiles)
    assert len(piped) == len(tiles) == len(host)
    for a, b, c in zip(piped, one, host):
        same(a, b)
        same(a, c)
    dets = []
    for flag in (True, False):
        rnet.device_tail = flag
        dets.append(rnet.predict([tiles[0]]))
    assert len(dets[0]) == len(dets[1]) and len(dets[0]) > 0
    for a, b in zip(*dets):
        assert list(a) == list(b) and all(np.array_equal(a[key], b[key]) and type(a[key]) is type(b[key]) for key in a)


def test_detect_paths_equal_host_tail_fp32(fp32_net):
    Cc, ms, rnet = fp32_net
    shapes = ((2048, 2048, 3), (300, 300, 3), (700, 1100, 3))
    tiles = [_tile(70 + i, sh) for i, sh in enumerate(((640, 640, 3), (640, 640, 3), (300, 420, 3), (640, 640, 3), (2048, 2048, 3)))]
    _end_to_end(rnet, shapes, tiles)


def test_detect_paths_equal_host_tail_bf16():
    Cc, ms, rnet = _models(precision="bf16")
    _end_to_end(rnet, ((300, 300, 3), (700, 1100, 3)), [_tile(80 + i, sh) for i, sh in enumerate(((640, 640, 3), (300, 420, 3), (640, 640, 3)))])


def test_detect_paths_equal_host_tail_vgg16():
    Cc, ms, rnet = _models(network="vgg16")
    _end_to_end(rnet, ((300, 300, 3), (700, 1100, 3)), [_tile(90 + i, sh) for i, sh in enumerate(((640, 640, 3), (300, 420, 3), (640, 640, 3)))])


# ------------------------------------------------------------------------------------------------------------ 4. the C entry point
def test_predict_tile_detect_equals_predict_tile_plus_host_decode(fp32_net):
    from radnet_hip import native
    Cc, ms, rnet = fp32_net
    eng = ms[2]._s.eng
    k = Cc.n_rois
    rnet.device_tail = True
    for seed, ratio, thr in ((3, 300 / 2048, 0.0), (4, 0.1, 0.0), (5, 600 / 700, 0.7)):
        img = torch.from_numpy(_tile(seed, (300, 300, 3))).cuda()
        R, pc, pr = native.predict_tile(eng, img, 300)
        n = R.shape[0]
        m = (n + k - 1) // k * k
        assert 0 < n <= 300 and pc.shape == (300, eng.nc)
        cls, boxes, probs = native.predict_tile_detect(eng, img, ratio, bbox_threshold=thr)
        hp = eng._plan_head(300, eng.feat_len(300), eng.feat_len(300), eng._plan_base(1, 300, 300, 0)["F"], training=False)
        pc2, pr2 = hp["pcls"].cpu().numpy(), hp["pregr"].cpu().numpy()
        # the rows that are proposals: the same bits from both entry points; a padding row: the bits of its chunk's first row
        # (radnet_predict_tile pads with row 0 instead, so its own padding rows are not the reference's)
        src = np.array([i if i < n else i // k * k for i in range(m)])
        assert np.array_equal(pc2[:n].view(np.uint32), pc[:n].view(np.uint32)) and np.array_equal(pr2[:n].view(np.uint32), pr[:n].view(np.uint32))
        assert np.array_equal(pc2[:m].view(np.uint32), pc[src].view(np.uint32)) and np.array_equal(pr2[:m].view(np.uint32), pr[src].view(np.uint32))
        xywh = R.copy()
        xywh[:, 2] -= xywh[:, 0]
        xywh[:, 3] -= xywh[:, 1]
        rnet.bbox_threshold = thr
        ref = host_tail(rnet, pc[src], pr[src], xywh, ratio)
        got = {}
        for c, b, p in zip(cls.tolist(), boxes.tolist(), probs):
            real, prb = got.setdefault(rnet.class_mapping[c], ([], []))
            real.append(tuple(b))
            prb.append(p)
        same(got, ref)
        assert thr > 0.0 or len(got) > 0


# ------------------------------------------------------------------------------------------------------------ 5. the schedule
def test_tile_loop_enqueues_the_next_classifier_pass_before_it_collects(fp32_net):
    Cc, ms, rnet = fp32_net

    class Recorder:
        accepts_any_roi_count = True

        def __init__(self, inner):
            self._inner, self.log, self._ids = inner, [], {}

        def __getattr__(self, name):
            return getattr(self._inner, name)

        def detect_launch(self, *a, **kw):
            h = self._inner.detect_launch(*a, **kw)
            j = len(self._ids)
            self._ids[id(h)] = j
            self._keep = getattr(self, "_keep", []) + [h]
            self.log.append(("launch", j))
            return h

        def detect_finish(self, h):
            self.log.append(("finish", self._ids[id(h)]))
            return self._inner.detect_finish(h)

    rec = Recorder(ms[4])
    from faster_rcnn.RADNet import RADNet
    from faster_rcnn.base_models import resnet50
    net2 = RADNet(Cc, ms[3], rec, resnet50.preprocess)
    net2.bbox_threshold = 0.0
    net2.device_tail = True
    tiles = [_tile(70 + i, sh) for i, sh in enumerate(((640, 640, 3), (640, 640, 3), (300, 420, 3), (640, 640, 3)))]
    out = net2._detect_all(tiles)
    assert len(out) == 4
    at = {ev: i for i, ev in enumerate(rec.log)}
    assert sorted(at) == sorted([(w, j) for w in ("launch", "finish") for j in range(4)])
    for j in range(3):
        assert at[("launch", j + 1)] < at[("finish", j)], rec.log
    assert [j for w, j in rec.log if w == "finish"] == [0, 1, 2, 3]
