"""Host side of the device merge of a scan (csrc/scan_tail.hip), no GPU needed:

  * the NumPy model of scan_tail_cases.py -- what the GPU tests hold the kernels against -- equals RADNet.final_nms and the merge
    lines of RADNet.predict (_merge_image, _merge_final) on every case, and the golden file of the reference's final_nms;
  * its restatement of NumPy's fp32 sum equals np.mean itself;
  * every mutant of the model is caught by some case: the case tables can tell the mistakes apart;
  * with the device work stubbed, predict with scan_tail = True builds the same list as the default path, and takes the host merge
    on a negative status."""
import contextlib
import warnings

import numpy as np
import pytest

import scan_tail_cases as S

FINAL_CASES = S.final_nms_cases()
MERGE_CASES = S.scan_merge_cases()


def radnet():
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    return RADNet(Config(), None, None, None)


def test_fp32_sum_restatement_is_np_mean_s():
    rs = np.random.RandomState(0)
    for n in list(range(1, 301)) + [399, 1000, 1025, 4099, 20000]:
        for scale in (1.0, 1e-3):
            a = (rs.uniform(0.5, 1.0, n) * scale).astype(np.float32)
            assert S.mean_f32(a).tobytes() == a.mean().tobytes() and isinstance(a.mean(), np.float32), n
            assert np.float32(np.float32(0) + S.np_sum_f32(a)).tobytes() == a.sum().tobytes(), n
    z = np.full(9, -0.0, np.float32)
    assert S.mean_f32(z).tobytes() == z.mean().tobytes() and S.mean_f32(z[:3]).tobytes() == z[:3].mean().tobytes()
    # ... and it is not the running sum, which is why the kernel restates it
    a = rs.uniform(0.8, 1.0, 300).astype(np.float32)
    assert sum(S.mean_f32(a[:n], "sequential_sum").tobytes() != a[:n].mean().tobytes() for n in range(1, 301)) > 50


@pytest.mark.parametrize("name", sorted(FINAL_CASES))
def test_model_equals_final_nms(name):
    boxes, probs, kw = S.case_args(FINAL_CASES[name])
    status, mb, mp = S.final_nms_model(boxes, probs, **kw)
    net = radnet()
    if len(boxes) == 0:
        assert status == 0 and len(mb) == 0 and net.final_nms(boxes, probs, **kw) == []
        return
    if status == S.FN_MALFORMED:
        with pytest.raises(AssertionError):
            net.final_nms(boxes, probs, **kw)
        return
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hb, hp = net.final_nms(boxes, probs, **kw)
    if status == S.FN_EMPTY:                             # the host takes the mean of an empty slice
        assert np.any(np.isnan(hp))
        return
    assert status == 0 and hp.dtype == np.float32 and hb.dtype.kind == "i"
    assert np.array_equal(hb, mb) and hp.tobytes() == mp.tobytes()


def test_case_tables_hold_what_they_are_for():
    st = {name: S.final_nms_model(*S.case_args(c)[:2], **S.case_args(c)[2])[0] for name, c in FINAL_CASES.items()}
    assert st["exactly_threshold"] == S.FN_EMPTY and st["malformed_x"] == st["malformed_y"] == S.FN_MALFORMED
    assert all(v == 0 for k, v in st.items() if k not in ("exactly_threshold", "malformed_x", "malformed_y") and not k.startswith("golden_"))
    k = lambda name: len(S.final_nms_model(*S.case_args(FINAL_CASES[name])[:2], **S.case_args(FINAL_CASES[name])[2])[1])
    assert k("overlap_fifth") == 2 and k("overlap_below_fifth") == 2 and k("overlap_above_fifth") == 1
    assert k("scatter_1025") > 200 and k("scatter_2049") > 300 and len(FINAL_CASES["scatter_1025"][1]) == 1025 and len(FINAL_CASES["scatter_2049"][1]) == 2049
    for m in (7, 8, 9, 16, 17, 128, 129, 136, 137, 300):
        assert k("sum_%d" % m) == 1 and len(FINAL_CASES["sum_%d" % m][1]) == m
    assert any(name.startswith("golden_") for name in FINAL_CASES)
    want = {"zero_record_tiles": 0, "slot_count_minus_one": S.SM_BAD_SLOT, "x1_equals_x2": S.SM_MALFORMED, "empty_cluster": S.SM_EMPTY,
            "coordinate_out_of_range": S.SM_RANGE, "nms_box_collapses": S.SM_NMS_BOX, "max_boxes_cap": 0, "slots_not_ascending": 0}
    for name, status in want.items():
        pool, tiles, kw = S.build_scan_case(MERGE_CASES[name])
        out = S.scan_merge_model(pool, tiles, **kw)
        assert out[1] == status and (status == 0 or out[0] == 0), name
        assert np.all(out[S.HEADER + S.RECORD * max(0, int(out[0])):] == S.SENTINEL) and np.all(out[2:S.HEADER] == S.SENTINEL)
    pool, tiles, kw = S.build_scan_case(MERGE_CASES["max_boxes_cap"])
    assert S.scan_merge_model(pool, tiles, **kw)[0] == 300
    pool, tiles, kw = S.build_scan_case(MERGE_CASES["cluster_over_four_tiles"])
    assert S.scan_merge_model(pool, tiles, **kw)[0] == 2
    pool, tiles, kw = S.build_scan_case(MERGE_CASES["cross_image_suppression"])
    assert S.scan_merge_model(pool, tiles, **kw)[0] == 3
    pool, tiles, kw = S.build_scan_case(MERGE_CASES["class_nms_2049"])                      # 2049 candidates of one class, the cap reached
    out = S.scan_merge_model(pool, tiles, **kw)
    assert sum(len(r) for r in MERGE_CASES["class_nms_2049"]["records"]) == 2049 and (out[0], out[1]) == (300, 0)


def test_model_equals_the_golden_final_nms():
    g = np.load(S.GOLDEN)
    for i in range(int(g["n_cases"])):
        boxes, p64 = g["c%d_boxes" % i], g["c%d_probs" % i]
        p32 = p64.astype(np.float32)
        status, mb, mp = S.final_nms_model(boxes, p32)
        if status != 0:                                  # the cast put a prob ON the fp32 threshold: the case the device hands back
            assert status == S.FN_EMPTY and np.any(p32 == np.float32(0.8)) and not np.any(p64 == 0.8)
            continue
        # the reference ran on fp64 probs: the same clusters wherever the cast neither ties two probs nor moves one across 0.8
        if len(np.unique(p32)) == len(np.unique(p64)) and np.array_equal(p32 > np.float32(0.8), p64 > 0.8) and np.array_equal(p32 < np.float32(0.8), p64 < 0.8):
            assert np.array_equal(mb, g["c%d_out_boxes" % i])
            # an fp32 mean of at most len(p32) terms against the fp64 one: (n + 1) roundings of 2^-24 relative at most
            assert np.all(np.abs(mp.astype(np.float64) - g["c%d_out_probs" % i]) <= (len(p32) + 1) * 2.0 ** -24 * g["c%d_out_probs" % i])


# ---- the merge lines of predict ------------------------------------------------------------------------------------------------------
def host_merge(net, pool, tiles, slot_rows, monkeypatch):
    """RADNet's own host merge (the lines predict runs) on the records of a pool; the device NMS restated by the oracle."""
    from faster_rcnn import rpn
    from oracle import glue
    from radnet_hip.engine import read_detections
    monkeypatch.setattr(rpn, "non_max_suppression_fast", lambda b, p, overlap_thresh=0.9, max_boxes=300: glue.greedy_nms(b, p, overlap_thresh, max_boxes))
    sw = S.slot_words(slot_rows)
    all_boxes, all_probs = {}, {}
    images = sorted(set(t[3] for t in tiles))
    for im in images:
        mine = [t for t in tiles if t[3] == im]
        dets = [net._det_from_records(*read_detections(pool[s:s + sw])) for (s, _, _, _) in mine]
        net._merge_image(dets, [(ox, oy) for (_, ox, oy, _) in mine], all_boxes, all_probs)
    return net._merge_final(all_boxes, all_probs)


def records_as_dicts(net, words):
    from radnet_hip.engine import read_scan_records
    status, cls, boxes, probs = read_scan_records(words)
    assert status == 0
    return [{'class': net.class_mapping[c], 'prob': p, 'x1': b[0], 'y1': b[1], 'x2': b[2], 'y2': b[3]} for c, b, p in zip(cls.tolist(), boxes.astype(np.int64), probs)]


def same_dets(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for key in x:
            assert type(x[key]) is type(y[key]) and (x[key] == y[key] if key == "class" else np.array_equal(x[key], y[key])), (key, x, y)
        assert np.float32(x["prob"]).tobytes() == np.float32(y["prob"]).tobytes()


# (the empty cluster: the host's mean of an empty slice is a box of INT64_MIN, on which its NMS then asserts)
HOST_RAISES = {"slot_count_minus_one", "x1_equals_x2", "nms_box_collapses", "empty_cluster"}
NO_HOST_FORM = {"slot_count_too_large", "class_out_of_range", "coordinate_out_of_range"}      # the device's own refusals


@pytest.mark.parametrize("name", sorted(MERGE_CASES))
def test_model_equals_the_merge_lines_of_predict(name, monkeypatch):
    case = MERGE_CASES[name]
    pool, tiles, kw = S.build_scan_case(case)
    out = S.scan_merge_model(pool, tiles, **kw)
    if name in NO_HOST_FORM:
        assert out[1] < 0 and out[0] == 0
        return
    net = radnet()
    net.class_mapping = {c: "class%d" % c for c in range(case["nc"])}
    if "fn" in case:                                     # the merge lines of predict have fixed parameters
        fn = net.final_nms
        monkeypatch.setattr(net, "final_nms", lambda b, p, **k: fn(b, p, **dict(k, **case["fn"])))
    if name in HOST_RAISES:
        assert out[1] < 0
        with pytest.raises(AssertionError), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            host_merge(net, pool, tiles, case["slot_rows"], monkeypatch)
        return
    host = host_merge(net, pool, tiles, case["slot_rows"], monkeypatch)
    same_dets(records_as_dicts(net, out), host)


# ---- the mutants ---------------------------------------------------------------------------------------------------------------------
def caught_by(mutant):
    hits = []
    for name, c in FINAL_CASES.items():
        b, p, kw = S.case_args(c)
        good, bad = S.final_nms_model(b, p, **kw), S.final_nms_model(b, p, mutant=mutant, **kw)
        if good[0] != bad[0] or (good[0] == 0 and not (np.array_equal(good[1], bad[1]) and good[2].tobytes() == bad[2].tobytes())):
            hits.append(name)
    for name, c in MERGE_CASES.items():
        pool, tiles, kw = S.build_scan_case(c)
        if not np.array_equal(S.scan_merge_model(pool, tiles, **kw), S.scan_merge_model(pool, tiles, mutant=mutant, **kw)):
            hits.append(name)
    return hits


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_every_mutant_is_caught(mutant):
    assert len(S.MUTANTS) >= 6
    assert caught_by(mutant), mutant


# ---- predict with the device work stubbed ------------------------------------------------------------------------------------------
class StubEvent:
    def synchronize(self):
        pass


class StubEngine:
    """What RADNet._scan_pass asks of the engine, on the host: the pool is a CPU tensor, scan_merge is the NumPy model."""
    main_stream, ctx, nc = None, None, 6

    def __init__(self, force_status=None):
        self.force_status, self.merges, self.pools = force_status, 0, 0

    @contextlib.contextmanager
    def lane(self, name):
        yield

    def mark(self):
        return StubEvent()

    def after(self, ev):
        pass

    def scan_pool(self, n_tiles, rows):
        import torch
        self.pools += 1
        return torch.full((n_tiles * S.slot_words(rows),), S.SENTINEL, dtype=torch.int32), S.slot_words(rows)

    def scan_table(self, tiles):
        return [tuple(int(v) for v in t) for t in tiles], None

    def scan_merge(self, pool, rows, table, nms_thresh=0.4, max_boxes=300, **fn):
        import torch
        self.merges += 1
        out = S.scan_merge_model(pool.numpy(), table[0], rows, self.nc, nms_thresh, max_boxes, **fn)
        if self.force_status is not None:
            out[:] = S.SENTINEL
            out[0], out[1] = 0, self.force_status
        return torch.from_numpy(out)


class StubModels:
    """model_rpn and model_detector in one: tile j's records are drawn from its bytes, so both paths see the same ones."""
    accepts_any_roi_count = True

    def __init__(self, eng):
        import types
        self._s = types.SimpleNamespace(eng=eng)
        self.collected = 0

    def propose_device(self, *a, **k):
        raise AssertionError("not on this path")

    def propose_launch(self, img_dev, overlap_thresh=0.7, slot=0):
        return (img_dev, None, None)

    def count_launch(self, h):
        return (h, StubEvent())

    @staticmethod
    def count_finish(counted):
        return 40

    def _words(self, tile, rows):
        rs = np.random.RandomState(int(tile.sum()) % 100000)
        n = int(rs.randint(0, 30))
        cls = np.sort(rs.randint(0, 5, n))
        centres = rs.randint(0, 120, (5, 2))
        recs = [(int(c), int(centres[i % 5, 0] + rs.randint(-4, 5)), int(centres[i % 5, 1] + rs.randint(-4, 5))) for i, c in enumerate(cls)]
        recs = [(c, x, y, x + int(rs.randint(30, 40)), y + int(rs.randint(30, 40)), np.float32(rs.uniform(0.7, 1.0))) for c, x, y in recs]
        return S.make_pool([recs], rows)[0]

    def detect_launch(self, bp, R_dev, Rn_dev, n, ratio, k, bbox_threshold, nms_thresh=0.2, max_boxes=300, out=None):
        import torch
        words = self._words(R_dev, 300)
        if out is not None:
            out[:len(words)] = torch.from_numpy(words)
            return None, StubEvent()
        return words, StubEvent()

    def detect_finish(self, handle):
        from radnet_hip.engine import read_detections
        self.collected += 1
        return read_detections(handle[0])


def stub_net(monkeypatch, force_status=None):
    import faster_rcnn.RADNet as R
    from faster_rcnn import rpn
    from faster_rcnn.config import Config
    from oracle import glue
    monkeypatch.setattr(rpn, "non_max_suppression_fast", lambda b, p, overlap_thresh=0.9, max_boxes=300: glue.greedy_nms(b, p, overlap_thresh, max_boxes))
    monkeypatch.setattr(R, "resize_cubic", lambda img, new_w, new_h, **kw: img)          # the "device image" of a tile: the tile
    Cc = Config()
    Cc.img_size, Cc.tile_size, Cc.tile_overlap, Cc.include_full_img = 160, 160, 80, True
    eng = StubEngine(force_status)
    m = StubModels(eng)
    net = R.RADNet(Cc, m, m, None)
    net.class_mapping = {c: "class%d" % c for c in range(6)}
    return net, eng, m


@pytest.mark.parametrize("force_status", [None, S.SM_EMPTY, S.SM_BAD_SLOT])
def test_predict_with_the_device_work_stubbed(monkeypatch, force_status):
    net, eng, m = stub_net(monkeypatch, force_status)
    images = [np.random.RandomState(4 + i).randint(0, 256, (240, 320 - 80 * i, 3)).astype(np.uint8) for i in range(2)]
    assert net.scan_tail is False and not net._scan_tail_on() and net._tail_on_device()
    default = net.predict(images)
    n_tiles = m.collected
    assert len(default) > 3 and n_tiles == 2 * 3 + 1 + 2 * 2 + 1 and eng.merges == 0      # _tail_collect once per tile, no device merge
    net.scan_tail = True
    assert net._scan_tail_on()
    for again in range(2):                               # the second call uses the pool of the first
        same_dets(net.predict(images), default)
    assert m.collected == n_tiles and eng.merges == 2 and eng.pools == 1                   # nothing collected in the tile loop
    dd = net.predict_device(images)
    assert eng.pools == 2 and len(dd) == len(default) and dd.status == (force_status or 0)
    same_dets(dd.to_host(), default)
    assert net.scan_tail is True
    net.set_distributed(enabled=True)                    # no process group: not sharded, the device merge stays
    assert net._scan_tail_on()
    net.device_tail = False
    assert not net._scan_tail_on()


def test_duck_typed_models_ignore_scan_tail():
    net = radnet()
    net.scan_tail = True
    assert not net._scan_tail_on()
    with pytest.raises(TypeError):
        net.predict_device([np.zeros((10, 10, 3), np.uint8)])


def test_confidence_threshold_in_fp32():
    from radnet_hip.engine import confidence_f32
    assert confidence_f32(0.8) == float(np.float32(0.8)) and confidence_f32(np.float32(0.8)) == float(np.float32(0.8)) and confidence_f32(0.5) == 0.5
    assert confidence_f32(np.float64(0.5)) == 0.5
    with pytest.raises(ValueError):
        confidence_f32(np.float64(0.8))
