"""The merge of a scan on the device (csrc/scan_tail.hip) on an MI355X: radnet_final_nms and radnet_scan_merge through their C
entries against the NumPy model of scan_tail_cases.py (which test_scan_tail_host.py holds against RADNet.final_nms and the merge
lines of predict), bit for bit over whole buffers prefilled with a sentinel; RADNet.final_nms_device against RADNet.final_nms; and
predict with scan_tail on against predict with it off, end to end on the small engine-backed net of test_gpu_detect_tail.py."""
import ctypes as C

import numpy as np
import pytest

import scan_tail_cases as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FINAL_CASES = S.final_nms_cases()
MERGE_CASES = S.scan_merge_cases()
BOX_SENTINEL, PROB_SENTINEL = -77, np.float32(-5.5)


@pytest.fixture(scope="module")
def ctx():
    from radnet_hip import lib as L
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    return L.Context(0)


# ---- radnet_final_nms --------------------------------------------------------------------------------------------------------------
def device_final_nms(ctx, groups, obj_avg_threshold, obj_confidence_threshold, n_obj_avg):
    """radnet_final_nms on a batch -> (out_boxes [cap][4], out_probs [cap], count [g], status [g], offsets), whole buffers."""
    from radnet_hip import lib as L
    from radnet_hip.engine import confidence_f32
    offsets = np.concatenate([[0], np.cumsum([len(p) for _, p in groups])]).astype(np.int32)
    cap, ng = int(offsets[-1]), len(groups)
    boxes = np.concatenate([np.asarray(b, np.int64).reshape(-1, 4) for b, _ in groups] + [np.zeros((0, 4), np.int64)])
    probs = np.concatenate([np.asarray(p, np.float32) for _, p in groups] + [np.zeros(0, np.float32)])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bd, pd, od = dev(boxes if cap else np.zeros((1, 4), np.int64)), dev(probs if cap else np.zeros(1, np.float32)), dev(offsets)
    ob = torch.full((max(cap, 1), 4), BOX_SENTINEL, dtype=torch.int64, device="cuda")
    op = torch.full((max(cap, 1),), float(PROB_SENTINEL), dtype=torch.float32, device="cuda")
    oc = torch.full((ng,), -9, dtype=torch.int32, device="cuda")
    os_ = torch.full((ng,), -9, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(ctx.lib.radnet_final_nms_ws_bytes(cap, ng)), dtype=torch.uint8, device="cuda")
    d = L.FinalNmsDesc()
    d.boxes, d.probs, d.offsets, d.n_groups, d.capacity = bd.data_ptr(), pd.data_ptr(), od.data_ptr(), ng, cap
    d.obj_avg_threshold, d.obj_confidence_threshold, d.n_obj_avg = obj_avg_threshold, confidence_f32(obj_confidence_threshold), n_obj_avg
    d.out_boxes, d.out_probs, d.out_count, d.out_status, d.ws = ob.data_ptr(), op.data_ptr(), oc.data_ptr(), os_.data_ptr(), ws.data_ptr()
    ctx.check(ctx.lib.radnet_final_nms(ctx.h, C.byref(d)), "radnet_final_nms")
    torch.cuda.synchronize()
    return ob.cpu().numpy()[:cap], op.cpu().numpy()[:cap], oc.cpu().numpy(), os_.cpu().numpy(), offsets


def check_final_nms(ctx, names, kw):
    groups = [FINAL_CASES[n][:2] for n in names]
    ob, op, oc, os_, offsets = device_final_nms(ctx, groups, **kw)
    want_b, want_p = np.full_like(ob, BOX_SENTINEL), np.full_like(op, PROB_SENTINEL)
    for g, (name, (boxes, probs)) in enumerate(zip(names, groups)):
        status, mb, mp = S.final_nms_model(boxes, probs, **kw)
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        assert os_[g] == status, (name, os_[g], status)
        if status < 0:                                   # the group's other outputs are unspecified
            want_b[lo:hi], want_p[lo:hi] = ob[lo:hi], op[lo:hi]
            continue
        assert oc[g] == len(mp), (name, oc[g], len(mp))
        want_b[lo:lo + len(mp)], want_p[lo:lo + len(mp)] = mb, mp
    assert np.array_equal(ob, want_b), names
    assert op.tobytes() == want_p.tobytes(), names


@pytest.mark.parametrize("name", sorted(FINAL_CASES))
def test_final_nms_cases(ctx, name):
    check_final_nms(ctx, [name], S.case_args(FINAL_CASES[name])[2])


def test_final_nms_batch_of_mixed_groups(ctx):
    check_final_nms(ctx, list(S.FINAL_NMS_BATCH), dict(S.DEFAULTS))
    check_final_nms(ctx, [], dict(S.DEFAULTS))           # no group: nothing launched, nothing written


def test_final_nms_argument_checks(ctx):
    from radnet_hip import lib as L
    d = L.FinalNmsDesc()
    d.n_groups, d.capacity, d.n_obj_avg = 1, 4, 5        # null pointers
    assert ctx.lib.radnet_final_nms(ctx.h, C.byref(d)) != 0
    d.n_groups, d.n_obj_avg = 0, 0
    assert ctx.lib.radnet_final_nms(ctx.h, C.byref(d)) != 0
    d.n_obj_avg, d.capacity = 5, -1
    assert ctx.lib.radnet_final_nms(ctx.h, C.byref(d)) != 0
    d.capacity = 0
    assert ctx.lib.radnet_final_nms(ctx.h, C.byref(d)) == 0


def test_final_nms_device_equals_final_nms(ctx):
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    net = RADNet(Config(), None, None, None)
    for name in ("one", "tie_disjoint", "below_6", "just_above", "mean_half_even", "sum_137", "scatter_1025", "golden_c1", "golden_c2", "n_obj_avg_2_conf_half"):
        boxes, probs, kw = S.case_args(FINAL_CASES[name])
        hb, hp = net.final_nms(boxes, probs, **kw)
        db, dp = net.final_nms_device(boxes, probs, **kw)
        assert db.dtype == hb.dtype and dp.dtype == hp.dtype == np.float32 and np.array_equal(db, hb) and dp.tobytes() == hp.tobytes(), name
    assert net.final_nms_device(np.zeros((0, 4), np.int64), np.zeros(0, np.float32)) == []
    with pytest.raises(AssertionError):
        net.final_nms_device(*FINAL_CASES["malformed_x"][:2])
    with pytest.raises(TypeError):
        net.final_nms_device(FINAL_CASES["one"][0].astype(np.float64), FINAL_CASES["one"][1])
    with pytest.raises(TypeError):
        net.final_nms_device(FINAL_CASES["one"][0], FINAL_CASES["one"][1].astype(np.float64))
    import warnings
    with warnings.catch_warnings():                      # the host's own answer to the empty cluster
        warnings.simplefilter("ignore")
        hb, hp = net.final_nms(*FINAL_CASES["exactly_threshold"][:2])
        db, dp = net.final_nms_device(*FINAL_CASES["exactly_threshold"][:2])
    assert np.array_equal(db, hb) and dp.tobytes() == hp.tobytes()


# ---- radnet_scan_merge -----------------------------------------------------------------------------------------------------------------
def device_scan_merge(ctx, pool, tiles, slot_rows, nc, nms_thresh=0.4, max_boxes=300, check=True, **fn):
    from radnet_hip import lib as L
    from radnet_hip.engine import SCAN_TILE, confidence_f32
    fn = dict(S.DEFAULTS, **fn)
    table = np.array([tuple(t) for t in tiles], SCAN_TILE).reshape(-1)
    rc, n_images, bad, msg = L.scan_merge_check(table, len(pool), slot_rows)
    assert rc == 0 or not check, msg
    n_images = max(n_images, 1)
    pd = torch.from_numpy(pool.copy()).cuda()
    td = torch.from_numpy(table.view(np.int32).copy()).cuda()
    out = torch.full((int(ctx.lib.radnet_scan_merge_out_bytes(nc, max_boxes)) // 4,), S.SENTINEL, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(ctx.lib.radnet_scan_merge_ws_bytes(len(table), slot_rows, n_images, nc, max_boxes)), dtype=torch.uint8, device="cuda")
    d = L.ScanMergeDesc()
    d.pool, d.pool_words, d.slot_rows = pd.data_ptr(), len(pool), slot_rows
    d.tiles_host, d.tiles_dev, d.n_tiles, d.nc = table.ctypes.data, td.data_ptr(), len(table), nc
    d.obj_avg_threshold, d.obj_confidence_threshold, d.n_obj_avg = fn["obj_avg_threshold"], confidence_f32(fn["obj_confidence_threshold"]), fn["n_obj_avg"]
    d.nms_thresh, d.max_boxes, d.out, d.ws = nms_thresh, max_boxes, out.data_ptr(), ws.data_ptr()
    ctx.check(ctx.lib.radnet_scan_merge(ctx.h, C.byref(d)), "radnet_scan_merge")
    torch.cuda.synchronize()
    assert np.array_equal(pd.cpu().numpy(), pool)        # the pool is read only
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(MERGE_CASES))
def test_scan_merge_cases(ctx, name):
    pool, tiles, kw = S.build_scan_case(MERGE_CASES[name])
    got, want = device_scan_merge(ctx, pool, tiles, **kw), S.scan_merge_model(pool, tiles, **kw)
    assert got.shape == want.shape and (got[0], got[1]) == (want[0], want[1]), (name, got[:2], want[:2])
    assert np.array_equal(got, want), name


def test_scan_merge_larger_groups_and_a_small_cap(ctx):
    """Groups beyond one workgroup's threads and beyond the LDS sort, through the whole merge; then max_boxes = 7."""
    recs, tiles = [], []
    for t, name in enumerate(("scatter_1025", "scatter_2049", "scatter_1025")):
        b, p = FINAL_CASES[name][:2]
        cls = np.where(np.arange(len(p)) % 3 == 0, 2, 0) if t < 2 else np.full(len(p), 2)
        order = np.argsort(-cls, kind="stable") if t == 0 else np.argsort(cls, kind="stable")
        recs.append([(int(cls[i]), int(b[i, 0]), int(b[i, 1]), int(b[i, 2]), int(b[i, 3]), p[i]) for i in order])
        tiles.append((17 * t, 5 * t, min(t, 1)))
    pool, slots = S.make_pool(recs, 2049)
    rows = [(s, ox, oy, im) for s, (ox, oy, im) in zip(slots, tiles)]
    for max_boxes in (300, 7):
        got = device_scan_merge(ctx, pool, rows, 2049, 3, max_boxes=max_boxes)
        want = S.scan_merge_model(pool, rows, 2049, 3, max_boxes=max_boxes)
        assert want[1] == 0 and want[0] > max_boxes and (max_boxes > 7 or want[0] == 14) and np.array_equal(got, want), max_boxes


def test_scan_merge_refuses_what_the_check_refuses(ctx):
    from radnet_hip import lib as L
    pool, tiles, kw = S.build_scan_case(MERGE_CASES["class_in_later_tile"])
    for bad in ([tiles[0], tiles[0]], [tiles[1], (tiles[0][0], 0, 0, -1)], [(len(pool), 0, 0, 0)], [(1, 0, 0, 0)]):
        with pytest.raises(L.RadnetError):               # overlapping slots, a decreasing image index, out of range, unaligned
            device_scan_merge(ctx, pool, bad, check=False, **kw)
    d = L.ScanMergeDesc()
    d.nc, d.max_boxes, d.n_obj_avg = 2, 300, 5
    assert ctx.lib.radnet_scan_merge(ctx.h, C.byref(d)) != 0                     # null out / ws


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_net():
    from test_gpu_detect_tail import _models, _tile
    Cc, ms, rnet = _models()
    Cc.tile_size, Cc.tile_overlap, Cc.include_full_img = 400, 250, True
    rnet.bbox_threshold = 0.0
    rnet.device_tail, rnet.device_resident, rnet.scan_tail = True, True, False
    images = [_tile(61, (700, 900, 3)), _tile(62, (640, 420, 3))]
    want = rnet.predict(images)                          # the host merge: computed once, never changed
    assert len(want) > 0
    return Cc, ms, rnet, images, want


def same_dets(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for key in x:
            assert type(x[key]) is type(y[key]), (key, type(x[key]), type(y[key]))
            assert np.array_equal(x[key], y[key]), (key, x[key], y[key])
        assert np.float32(x["prob"]).tobytes() == np.float32(y["prob"]).tobytes()


def test_predict_with_scan_tail_equals_predict_without(scan_net, monkeypatch):
    Cc, ms, rnet, images, want = scan_net
    collected = []
    collect = rnet._tail_collect
    monkeypatch.setattr(rnet, "_tail_collect", lambda h: collected.append(1) or collect(h))
    n_tiles = 9 + 1 + 4 + 1                              # 700 x 900 and 640 x 420 under 400 / 250 tiles, each with its full image
    assert rnet.scan_tail is False and not rnet._scan_tail_on()
    same_dets(rnet.predict(images), want)                # the default: the host merge, every tile's records collected in the loop
    assert len(collected) == n_tiles
    try:
        rnet.scan_tail = True
        assert rnet._scan_tail_on()
        del collected[:]
        same_dets(rnet.predict(images), want)            # from host arrays
        pool = rnet._scan_pool[1]
        same_dets(rnet.predict(images), want)            # a second call: the same pool
        assert rnet._scan_pool[1] is pool and pool.numel() == n_tiles * S.slot_words(300)
        dev_images = [torch.from_numpy(im).cuda() for im in images]
        same_dets(rnet.predict(dev_images), want)        # from device images
        dd = rnet.predict_device(dev_images)
        assert dd.records.is_cuda and dd.status == 0 and len(dd) == len(want)
        same_dets(dd.to_host(), want)
        same_dets(rnet.predict_device(images).to_host(), want)
        assert collected == []                           # nothing collected in the tile loop
        same_dets(rnet.predict(images[:1]), rnet_default(rnet, images[:1]))
    finally:
        rnet.scan_tail = False


def rnet_default(rnet, images):
    saved, rnet.scan_tail = rnet.scan_tail, False
    try:
        return rnet.predict(images)
    finally:
        rnet.scan_tail = saved


def test_negative_status_takes_the_host_merge(scan_net, monkeypatch):
    """A merge that reports a failure (forced here: the words of an empty-cluster status) sends predict to the pool and the host."""
    Cc, ms, rnet, images, want = scan_net
    eng = rnet._engine()
    merge = eng.scan_merge

    def failing(*a, **kw):
        out = merge(*a, **kw)
        out[:2] = torch.tensor([0, S.SM_EMPTY], dtype=torch.int32, device=out.device)
        return out
    monkeypatch.setattr(eng, "scan_merge", failing)
    try:
        rnet.scan_tail = True
        same_dets(rnet.predict(images), want)
    finally:
        rnet.scan_tail = False
