"""Device-free checks of tests/proposal_edge_cases.py, the case tables and expected buffers of tests/test_gpu_proposal_edges.py:

  * every case reaches the branch it names, asserted from the tally the oracle's own decisions give;
  * the NumPy models of the kernels' schemes -- the 64-candidate chunk scan, the band select with its 4096-key cap, the visiting-order
    best-anchor key with the ordered fallback, the RoI labelling -- equal the oracle on every case;
  * every named mutant of a model or of the oracle differs from the oracle on at least one case: the tables have teeth;
  * no expected value equals the sentinel, and the judgement itself has teeth;
  * the tables build in a few seconds."""
import time

import numpy as np
import pytest

import proposal_edge_cases as E

F = np.float32


def _ids(cases):
    return [c["name"] for c in cases]


# ---------------------------------------------------------------------------------------------------------------- reach
def test_tables_build_in_a_few_seconds():
    t0 = time.perf_counter()
    for c in E.nms_cases():
        E.nms_expected(c)
    for i in range(len(E.rpn_cases())):
        E.rpn_expected(i)
    for i in range(len(E.anchor_cases())):
        E.anchor_expected(i)
        E.anchor_pack_expected(i)
    for i in range(len(E.roi_cases())):
        E.roi_expected(i)
    for k in range(len(E.PACK_CASES)):
        E.pack_expected(k)
    dt = time.perf_counter() - t0
    print("tables: %.1f s" % dt)
    assert dt < 15.0


def test_the_tables_hold_the_cases_the_suite_is_there_for():
    names = {c["name"] for c in E.nms_cases()}
    for n in E.NMS_SIZES:
        for mb in {1, 63, 64, 65, min(n, 1024), 1024}:
            assert "disjoint_n%d_max%d" % (n, mb) in names
    assert {c["branch"] for c in E.nms_cases()} == set(E.NMS_REACH)
    shapes = {(c["rows"], c["cols"], c["A"], c["ld"]) for c in E.rpn_cases()}
    assert shapes >= {(1, 2, 1, 5), (2, 1, 1, 8), (3, 5, 12, 60), (3, 5, 12, 64), (7, 9, 32, 160), (16, 16, 1, 5), (1, 257, 1, 5), (63, 65, 1, 5),
                      (64, 64, 1, 5), (17, 241, 1, 5), (19, 647, 1, 5)}
    assert 19 * 647 == 3 * 4096 + 5 and {c["mb"] for c in E.rpn_cases()} >= {1, 64, 1024}
    assert {c["scores"] for c in E.rpn_cases()} == {"distinct", "tie", "two_levels", "zeros", "denormal"}
    assert any(c["use_regr"] == 0 for c in E.rpn_cases()) and {c["branch"] for c in E.rpn_cases()} == set(E.RPN_REACH)
    assert {(m.fw, m.fh) for m in E.ANCHOR_MAPS} == {(1, 1), (1, 7), (7, 1), (5, 3), (16, 16), (13, 20)}
    assert {c["branch"] for c in E.anchor_cases()} == set(E.ANCHOR_REACH) == set(E.GT_KINDS)
    assert {(c["n"], c["g"]) for c in E.roi_cases()} == {(n, g) for n in (1, 255, 256, 257) for g in (0, 1, 40)}
    assert {c["branch"] for c in E.roi_cases()} == set(E.ROI_REACH)
    assert E.PACK_CASES == [(r, nc) for r in (1, 4, 33) for nc in (2, 7, 21)]


@pytest.mark.parametrize("case", E.nms_cases(), ids=_ids(E.nms_cases()))
def test_nms_case_reaches_its_branch_and_the_chunk_scan_equals_the_oracle(case):
    t = E.nms_tally(case["boxes"], case["probs"], case["thr"], case["mb"])
    assert E.NMS_REACH[case["branch"]](t), (case["branch"], t)
    exp = E.nms_expected(case)
    count = int(exp["out_count"].buf[0])
    if t["malformed"]:
        assert count == -1 and (exp["out_idx"].buf == E.sentinel(np.int32, 1)[0]).all()
        return
    assert count == t["picks"]
    picks = E.model_nms(case["boxes"], case["probs"], case["thr"], case["mb"])
    assert np.array_equal(picks, exp["out_idx"].buf[:count])
    assert (exp["out_idx"].buf[count:] == E.sentinel(np.int32, 1)[0]).all()
    assert np.array_equal(E.model_nms(case["boxes"], case["probs"], case["thr"], case["mb"], "matrix_no_lane_restriction"), picks)
    if count:                                                       # the indices stand for what the oracle itself returns
        rb, rp = E.glue.greedy_nms(case["boxes"], case["probs"], case["thr"], case["mb"])
        assert np.array_equal(case["boxes"][picks].astype("int"), rb) and np.array_equal(case["probs"][picks].view(np.uint32), rp.view(np.uint32))


def test_the_disjoint_scores_never_rank_an_index_at_its_own_place():
    for c in E.nms_cases():
        if c["name"].startswith("disjoint") and len(c["probs"]) > 1:
            assert (E.stable_desc(c["probs"]) != np.arange(len(c["probs"]))).all(), c["name"]


@pytest.mark.parametrize("i", range(len(E.rpn_cases())), ids=_ids(E.rpn_cases()))
def test_rpn_case_reaches_its_branch_and_both_path_models_equal_the_oracle(i):
    cs = E.rpn_cases()[i]
    t = E.rpn_tally(i)
    assert E.RPN_REACH[cs["branch"]](t), (cs["branch"], {k: v for k, v in t.items() if k != "scan_slots"})
    exp = E.rpn_expected(i)
    count = int(exp["out_count"].buf[0])
    assert count == t["picks"] and count <= cs["mb"]
    for path in ("full_sort", "select"):
        b, p = E.rpn_model_outputs(i, path)
        assert len(b) == count, path
        assert np.array_equal(b.reshape(-1), exp["out_boxes"].buf[:4 * count]), path
        assert np.array_equal(p.view(np.uint32), exp["out_probs"].buf[:count].view(np.uint32)), path


def test_the_planted_deltas_are_marked_from_the_float64_decode():
    by = {c["name"]: i for i, c in enumerate(E.rpn_cases())}
    count = lambda name: E.rpn_tally(by[name])["nonfinite"]
    assert [count("plant_" + k) for k in ("nan_tx", "nan_th", "pinf_tw", "overflow_tw", "overflow_th")] == [3] * 5
    assert [count("plant_" + k) for k in ("ninf_tw", "pinf_tx", "ninf_ty")] == [0] * 3       # width 1, or a degenerate box: the oracle's result stands
    assert 12 <= count("plant_mixed") <= 15                         # a planted box that is degenerate on its other axis is dropped by the decode itself
    # the planted anchors hold the best scores, and without the removal the reference asserts
    i = by["plant_pinf_tw"]
    boxes, probs, keep, bad = E.rpn_decoded(i)
    assert set(np.argsort(probs)[::-1][:3]) == set(np.nonzero(bad)[0])
    with pytest.raises(AssertionError):
        E.glue.greedy_nms(boxes, probs, 0.7, 64)


@pytest.mark.parametrize("i", range(len(E.anchor_cases())), ids=_ids(E.anchor_cases()))
def test_anchor_case_reaches_its_branch_and_the_key_model_equals_the_oracle(i):
    cs = E.anchor_cases()[i]
    t = E.anchor_tally(i)
    assert E.ANCHOR_REACH[cs["branch"]](t), (cs["branch"], t)
    d, m = E.anchor_dense(i), E.model_anchor_targets(i)
    for k in ("valid", "overlap", "regr", "best_anchor", "n_for_gt"):
        assert np.array_equal(m[k], d[k]), k


def test_the_anchor_maps_put_edges_on_and_one_pixel_beyond_the_image():
    t = [E.anchor_tally(next(i for i, c in enumerate(E.anchor_cases()) if c["map"] is m)) for m in E.ANCHOR_MAPS]
    assert all(x["edge_on_zero"] and x["edge_on_rw"] for x in t[:4]) and t[4]["one_beyond"] and t[5]["one_beyond"] and t[7]["one_beyond"]
    assert t[4]["inside"] == 4 * 2 and t[5]["inside"] == 3 * 1 and t[3]["inside"] == 15
    assert t[6]["anchors"] == 256 and t[6]["blocks"] == 1 and t[7]["anchors"] == 13 * 20 * 12 and 0 < t[7]["inside"] < t[7]["anchors"]
    for i, cs in enumerate(E.anchor_cases()):
        m = cs["map"]
        total = m.fw * m.fh * 8 * len(m.scales) * len(m.ratios)
        assert total % 256 != 0 or (m.fw, m.fh) == (16, 16)


@pytest.mark.parametrize("i", range(len(E.roi_cases())), ids=_ids(E.roi_cases()))
def test_roi_case_reaches_its_branch_and_the_row_model_equals_the_oracle(i):
    cs, d = E.roi_cases()[i], E.roi_inputs(i)
    t = E.roi_tally(i)
    assert E.ROI_REACH[cs["branch"]](t), (cs["branch"], t)
    r, m = E.roi_rows(i), E.model_roi_targets(d["rois"], d["gt"], d["gt_cls"], E._roi_config())
    for k in ("keep", "cls", "box", "t", "iou"):
        assert np.array_equal(m[k], r[k]), k
    exp = E.roi_expected(i)
    live = t["live"]
    s64, s32 = E.sentinel(np.float64, 1)[0], E.sentinel(np.int32, 1)[0]
    assert (exp["keep"].buf[live:cs["n"]] == 0).all() and (exp["cls"].buf[live:cs["n"]] == -1).all()
    assert (exp["iou"].buf[live:].view(np.uint64) == s64.view(np.uint64)).all() and (exp["box"].buf[4 * live:] == s32).all()


@pytest.mark.parametrize("k", range(len(E.PACK_CASES)), ids=[str(c) for c in E.PACK_CASES])
def test_pack_case_selects_repeats_out_of_order_and_background_rows(k):
    d = E.pack_inputs(k)
    sel, r = d["sel"], d["r"]
    assert len(sel) == r and (d["cls"][sel] >= 0).all()
    if r >= 4:
        assert len(set(sel.tolist())) < r and (np.diff(sel) < 0).any() and (d["cls"][sel] == d["bg"]).any() and (d["cls"][sel] != d["bg"]).any()
    exp = E.pack_expected(k)
    nreg = 4 * (d["nc"] - 1)
    y2 = exp["y2"].buf[:r * 2 * nreg].reshape(r, 2 * nreg)
    assert np.array_equal(y2[:, :nreg].sum(1), np.where(d["cls"][sel] == d["bg"], 0.0, 4.0))
    for j, s in enumerate(sel):                                     # the packed row is the kernel's own formula on the per-row arrays
        on = d["cls"][s] != d["bg"]
        ref = np.zeros(nreg, F)
        if on:
            ref[4 * d["cls"][s]:4 * d["cls"][s] + 4] = d["t"][s].astype(F)
        assert np.array_equal(y2[j, nreg:], ref)


# ---------------------------------------------------------------------------------------------------------------- teeth
def _nms_differs(mutant):
    hits = []
    for c in E.nms_cases():
        exp = E.nms_expected(c)
        count = int(exp["out_count"].buf[0])
        if count < 0:
            continue
        if not np.array_equal(E.model_nms(c["boxes"], c["probs"], c["thr"], c["mb"], mutant), exp["out_idx"].buf[:count]):
            hits.append(c["name"])
    return hits


def _rpn_differs(mutant, path):
    hits = []
    for i, cs in enumerate(E.rpn_cases()):
        exp = E.rpn_expected(i)
        count = int(exp["out_count"].buf[0])
        b, p = E.rpn_model_outputs(i, path, mutant)
        if len(b) != count or not np.array_equal(b.reshape(-1), exp["out_boxes"].buf[:4 * count]) or not np.array_equal(
                p.view(np.uint32), exp["out_probs"].buf[:count].view(np.uint32)):
            hits.append(cs["name"])
    return hits


def _anchor_differs(mutant):
    hits = []
    for i, cs in enumerate(E.anchor_cases()):
        d, m = E.anchor_dense(i), E.model_anchor_targets(i, mutant)
        if not all(np.array_equal(m[k], d[k]) for k in ("valid", "overlap", "regr", "best_anchor")):
            hits.append(cs["name"])
    return hits


def _roi_differs(mutant):
    hits = []
    for i, cs in enumerate(E.roi_cases()):
        if cs["n_dev"] is not None:
            continue
        d, r = E.roi_inputs(i), E.roi_rows(i)
        m = E.model_roi_targets(d["rois"], d["gt"], d["gt_cls"], E._roi_config(), mutant)
        if not all(np.array_equal(m[k], r[k]) for k in ("keep", "cls", "box", "t", "iou")):
            hits.append(cs["name"])
    return hits


MUTANT_HOMES = {         # mutant -> (where it is looked for, the case that exists for it)
    "ties_lower_index_first": (lambda m: _nms_differs(m), "ties_all_equal"),
    "suppress_ge": (lambda m: _nms_differs(m), "thr_eq_q_0"),
    "one_pick_too_many": (lambda m: _nms_differs(m), "disjoint_n65_max63"),
    "pick_slot_skipped": (lambda m: _nms_differs(m), "pick_slots"),
    "matrix_lane_lt_j": (lambda m: _nms_differs(m), "chain_200"),
    "alive_not_trimmed": (lambda m: _nms_differs(m), "disjoint_n65_max1024"),
    "band_cut_drops_tie": (lambda m: _rpn_differs(m, "select"), "single_tie_12293"),
    "last_best_anchor": (lambda m: _anchor_differs(m), "5x3_a1_rw80_s16_between_x"),
    "best_anchor_fp64": (lambda m: _anchor_differs(m), "5x3_a1_rw80_s16_fp32_tie"),
    "fallback_reverse_order": (lambda m: _anchor_differs(m), "5x3_a1_rw80_s16_two_onto_one"),
    "last_gt_wins_tie": (lambda m: _roi_differs(m), "n257_g40_ndev_null"),
    "round_half_away": (lambda m: _roi_differs(m), "n257_g40_ndev_null"),
}


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_every_mutant_differs_from_the_oracle_on_the_case_named_for_it(mutant):
    assert set(MUTANT_HOMES) == set(E.MUTANTS)
    find, home = MUTANT_HOMES[mutant]
    hits = find(mutant)
    print("%s: caught by %d cases" % (mutant, len(hits)))
    assert home in hits, (mutant, hits[:8])


def test_the_scan_mutants_are_caught_on_the_rpn_tables_too():
    assert _rpn_differs("ties_lower_index_first", "full_sort") and _rpn_differs("alive_not_trimmed", "select")
    assert _rpn_differs("one_pick_too_many", "select") and _rpn_differs("suppress_ge", "full_sort") == _rpn_differs("suppress_ge", "select")


def test_the_literal_matrix_mutant_is_equivalent():
    """Bits at and below row j are already clear when the serial resolve reaches row j, so dropping `lane > j` changes no pick."""
    assert E.EQUIVALENT_MUTANTS == ("matrix_no_lane_restriction",)
    assert not _nms_differs("matrix_no_lane_restriction") and not _rpn_differs("matrix_no_lane_restriction", "select")


def test_signed_zero_scores_tie_in_the_reference_and_an_ordering_of_the_bits_would_differ():
    c = next(c for c in E.nms_cases() if c["name"] == "ties_signed_zero")
    exp = E.nms_expected(c)
    count = int(exp["out_count"].buf[0])
    u = c["probs"].view(np.uint32).astype(np.uint64)
    raw = np.where(u & 0x80000000 != 0, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)          # -0.0 ranked below +0.0
    order = np.argsort((raw << np.uint64(32)) | np.arange(len(u), dtype=np.uint64))[::-1]
    cs = E.ChunkScan(c["boxes"], c["thr"], c["mb"])
    cs.feed(order)
    assert not np.array_equal(np.asarray(cs.picks), exp["out_idx"].buf[:count])


def test_no_expected_value_is_a_sentinel_and_the_judgement_has_teeth():
    for i in range(len(E.anchor_cases())):
        for k, o in E.anchor_pack_expected(i)[1].items():
            assert not (o.buf[:-E.TAIL].view(np.uint32) == E.sentinel(F, 1).view(np.uint32)[0]).any()
        e = E.anchor_expected(i)
        assert not (e["regr"].buf[:-E.TAIL].view(np.uint64) == E.sentinel(np.float64, 1).view(np.uint64)[0]).any()
        assert (e["valid"].buf[:-E.TAIL] <= 1).all()
    exp = E.roi_expected(next(i for i, c in enumerate(E.roi_cases()) if c["name"] == "n257_g40_ndev_null"))["t"]
    assert E.judge("t", exp.buf.copy(), exp) == []
    got = exp.buf.copy()
    j = int(np.nonzero(exp.loose & (exp.buf != 0))[0][0])
    got[j] = np.nextafter(got[j], np.inf)
    assert E.judge("t", got, exp) == []                              # 1 ulp on a log component
    got[j] = exp.buf[j] * (1 + 2.0 ** -50)
    assert E.judge("t", got, exp)
    got = exp.buf.copy()
    j = int(np.nonzero(exp.buf[:1028:4] != 0)[0][0]) * 4
    got[j] = np.nextafter(got[j], np.inf)
    assert E.judge("t", got, exp)                                    # tx is bit for bit
    got = exp.buf.copy()
    got[-1] = 0.0
    assert E.judge("t", got, exp)                                    # the tail
