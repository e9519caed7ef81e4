"""Device-free checks of tests/head_edge_cases.py, the case tables and float64 references of tests/test_gpu_head_edges.py:

  * every case lies inside the contract of its entry point, and the tables reach the paths they are there for;
  * the references agree with oracle/dense.py where it has the operation, at one shared shape each;
  * no decision (smooth-L1 branch, clip, ReLU, argmax) of any case is borderline between fp32 and float64;
  * honest fp32 arithmetic of the + - * / operations stays inside their bounds, the bit-exact ones are bit-exact;
  * the bounds have teeth: every mutant lies outside the bound of the case named for it."""
import numpy as np
import pytest

import head_edge_cases as E
from oracle import dense

F = np.float32


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) / max(float(np.abs(b).max()), 1e-300)


def _inner(res):
    """The tensor of a full buffer, without its tail."""
    return res["buf"][:-E.TAIL].reshape(res["shape"])


# ---------------------------------------------------------------------------------------------------------------- contracts, reach
def test_every_case_lies_inside_its_entry_s_contract():
    assert all(E.maxpool_contract(*cs) for cs in E.MAXPOOL)
    for mi, (H, W, C) in enumerate(E.ROI_MAPS):
        for ps in set(E.ROI_FWD_PS) | set(E.roi_bwd_ps(mi)):
            assert E.roi_contract(H, W, C, E.roi_inputs(mi, ps)["rois"], ps), (mi, ps)
    assert all(E.avgpool_contract(*cs) for cs in E.AVGPOOL)
    assert all(E.dense_contract(*cs) for cs in E.DENSE_FWD)
    assert all(E.dense_bwd_contract(*cs) for cs in E.DENSE_BWD)
    assert all(E.rpn_contract(*cs) for cs in E.RPN)
    assert all(E.det_contract(*cs) for cs in E.DET)
    assert all(E.head_tail_contract(cs) for cs in E.HEAD_TAIL)
    # what lies outside: the arguments the entries refuse on the host
    assert not E.maxpool_contract(1, 5, 5, 4, 3, 0) and not E.maxpool_contract(1, 5, 5, 4, 0, 1) and not E.maxpool_contract(1, 2, 5, 4, 3, 1)
    assert not E.dense_bwd_contract(513, 8, 32, 31, 0) and not E.dense_bwd_contract(4, 8, 48, 31, 0) and not E.dense_bwd_contract(4, 8, 32, 33, 0)
    assert not E.head_tail_contract(E.HeadTail(6, 49, 36, 32, 7, 24, 1, None)) and not E.head_tail_contract(E.HeadTail(6, 49, 2080, 32, 7, 24, 1, None))
    assert not E.head_tail_contract(E.HeadTail(6, 49, 2048, 32, 7, 24, 4, None)) and not E.head_tail_contract(E.HeadTail(6, 49, 2048, 48, 7, 24, 1, None))


def test_tables_reach_the_paths_they_name():
    assert E.MAXPOOL[:6] == [(1, 3, 3, 4, 3, 2), (1, 2, 3, 4, 1, 1), (2, 7, 9, 4, 3, 2), (1, 8, 10, 8, 3, 2), (3, 5, 6, 12, 2, 2), (1, 21, 30, 68, 3, 2)]
    assert all((E.maxpool_inputs(i)["x"] < 0).all() for i in E.MAXPOOL_NEGATIVE) and E.MAXPOOL_NEGATIVE
    assert E.ROI_MAPS == [(5, 7, 4), (6, 5, 12), (9, 11, 260), (4, 4, 1028)]
    launch_threads = lambda c: 256 if c // 4 >= 256 else (c // 4 + 63) // 64 * 64
    assert [launch_threads(c) for _, _, c in E.ROI_MAPS] == [64, 64, 128, 256] and 1028 // 4 > 256
    assert set(E.ROI_FWD_PS) == {1, 2, 7, 14} and set(E.roi_bwd_ps(0)) == {1, 2, 7, 32, 33} and all(set(E.roi_bwd_ps(i)) == {1, 2, 7} for i in (1, 2, 3))
    for H, W, _ in E.ROI_MAPS:
        rois = E.roi_list(H, W)
        g = [E._geom(r, H, W) for r in rois]
        assert g[0] == (0, 0, W, H) and [q[2:] for q in g[1:5]] == [(1, 1)] * 4 and {q[:2] for q in g[1:5]} == {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}
        assert g[5][2] == 0 and g[6][3] == 0 and g[7] == (W - 2, H - 2, 2, 2) and g[8][2] == 0 and g[8][0] == W
        assert g[9] == (1, 0, 2, 3) and E._geom(rois[9], H, W, "roi_round") != g[9]
        assert g[10] == g[11] and (rois[10] == rois[11]).all() and g[12][0] < g[10][0] + g[10][2] and g[12][1] < g[10][1] + g[10][3]
        assert (rois >= 0).all()
    assert E.AVGPOOL == [(1, 1, 4), (1, 49, 4), (3, 2, 8), (5, 49, 260), (2, 64, 12), (2, 100, 36)]
    assert E.DENSE_FWD == [(1, 4, 32, 2, 4), (3, 100, 32, 7, 24), (2, 300, 32, 1, 4), (5, 256, 64, 13, 48), (1, 257, 64, 16, 48), (2, 4096, 64, 21, 40)]
    assert 80.0 in E.DENSE_FWD_SPREAD.values()
    b = E.DENSE_BWD
    assert {c[0] for c in b} >= {1, 20, 33, 64, 512} and {c[1] for c in b} >= {4, 9, 100, 2048} and {c[4] for c in b} == {0, 1}
    assert {c[2:4] for c in b} >= {(32, 31), (32, 32), (64, 37), (64, 64)} and (512, 8, 32, 31, 0) in b and 512 * 32 * 4 == 64 * 1024
    assert E.RPN == [(1, 1, 5, 5), (3, 2, 10, 12), (7, 12, 64, 64), (50, 9, 45, 64), (300, 12, 64, 80)]
    assert E.DET == [(1, 2, 4), (3, 7, 24), (20, 7, 24), (64, 13, 48), (257, 7, 24)]
    h = E.HEAD_TAIL
    assert {c.c for c in h} == {32, 96, 2048} and {c.hw for c in h} == {1, 3, 16, 49, 64, 65, 100} and {c.ldw for c in h} == {32, 64}
    assert {(c.R, c.groups) for c in h} >= {(1, 1), (6, 1), (6, 2), (6, 6), (40, 2)}
    assert any(c.idle is None for c in h) and any(c.idle == 0 for c in h) and any(c.idle == c.groups - 1 and c.groups > 1 for c in h)
    assert any(c.nc + c.nreg == c.ldw for c in h)
    # layouts of the loss inputs
    for i, (m, a, _, _) in enumerate(E.RPN):
        d = {lay: E.rpn_inputs(i, lay) for lay in E.RPN_LAYOUTS}
        assert d["none_valid"]["y_cls"][:, :a].sum() == 0 and d["all_valid"]["y_cls"][:, :a].all()
        assert d["no_positive"]["y_cls"][:, :a].sum() > 0 and d["no_positive"]["y_cls"][:, a:].sum() == 0 and d["no_positive"]["y_regr"][:, :4 * a].sum() == 0
        assert (d["general"]["pred"][:, 5 * a:] == E.PAD).all()
        if m * a >= 6:
            p, valid = d["all_valid"]["pred"][:, :a], d["all_valid"]["y_cls"][:, :a]
            assert ((p == 0) & (valid > 0)).any() and ((p == 1) & (valid > 0)).any()
            x = np.abs(d["general"]["y_regr"][:, 4 * a:] - d["general"]["pred"][:, a:5 * a])
            assert (x == 0).any() and ((x > 0) & (x < 1)).any() and (x > 1).any()
    for i, (r, nc, nreg) in enumerate(E.DET):
        d = E.det_inputs(i, "general")
        assert (E.det_inputs(i, "all_background")["y2"][:, :nreg] == 0).all()
        if r >= 3:
            q = d["q"]
            assert (q[0] == 0).any() and abs(float(q[1].sum()) - 1) > 0.2 and q[r - 1, 0] == q[r - 1, 1] == q[r - 1].max() and d["y1"][r - 1, 1] == 1
    for i, cs in enumerate(E.HEAD_TAIL):
        d = E.head_tail_inputs(i)
        assert (d["w"][:, cs.nc + cs.nreg:] == E.PAD).all() and (d["b"][cs.nc + cs.nreg:] == E.PAD).all() and (d["y5"] >= 0).all() and (d["y5"] == 0).any()


# ---------------------------------------------------------------------------------------------------------------- the oracle
def test_references_agree_with_the_oracle_at_shared_shapes():
    rs = np.random.RandomState(5)
    x = rs.standard_normal((2, 7, 9, 4))
    assert np.array_equal(_inner(E.ref_maxpool(x, 3, 2)["y"]), dense.maxpool_3x3_s2(x))
    assert np.array_equal(_inner(E.ref_maxpool(x, 2, 2)["y"]), dense.maxpool_2x2_s2(x))
    H, W, C = E.ROI_MAPS[1]
    d = E.roi_inputs(1, 7)
    f64 = d["fmap"].astype(np.float64)
    full = np.array([min(E._geom(r, H, W)[2:]) > 0 for r in d["rois"]])                  # the oracle's forward takes no empty crop
    assert _rel(_inner(E.ref_roi_fwd(d["fmap"], d["rois"], 7)["y"])[full], dense.roi_crop_resize(f64[None], d["rois"][full], 7)) <= 1e-14
    assert (_inner(E.ref_roi_fwd(d["fmap"], d["rois"], 7)["y"])[~full] == 0).all() and (~full).sum() == 3
    zero_old = np.zeros((H, W, C), F)
    got = _inner(E.ref_roi_bwd(d["dy"], H, W, d["rois"], 7, zero_old, True)["dfmap"])
    assert _rel(got, dense.roi_crop_resize_bwd((1, H, W, C), d["rois"], 7, d["dy"].astype(np.float64))[0]) <= 1e-14
    z = rs.standard_normal((5, 13)) * 3
    assert _rel(E.softmax(z), dense.softmax(z)) <= 1e-15
    # RPN losses at (7, 12, 64, 64): the oracle takes [1][H][W][..] maps and float64 clip bounds; no prediction of this layout is clipped
    m, a, ld_pred, ld_dz = E.RPN[2]
    di = E.rpn_inputs(2, "no_positive")
    p, reg = di["pred"][:, :a].astype(np.float64), di["pred"][:, a:5 * a].astype(np.float64)
    for mode in (0, 1):
        dz, losses = E.ref_rpn(di["pred"], di["y_cls"], di["y_regr"], m, a, ld_dz, mode)
        lc, dp = dense.rpn_loss_cls(di["y_cls"].astype(np.float64)[None, None], p[None, None], a, mode == 0)
        lr, dr = dense.smooth_l1_masked(di["y_regr"].astype(np.float64)[None, None], reg[None, None], 4 * a)
        assert abs(losses[0] - lc) <= 1e-6 * abs(lc) and abs(losses[1] - lr) <= 1e-12          # mode 0: the oracle's logit of the label is fp32
        assert _rel(dz[:, :a], (dp * p * (1 - p))[0, 0]) <= 1e-6 and np.abs(dz[:, a:5 * a] - dr[0, 0]).max() <= 1e-15
    di = E.rpn_inputs(2, "all_valid")
    x = di["pred"][:, :a]
    keep = (x > 0) & (x < 1)                                                               # where nothing is clipped
    dz, _ = E.ref_rpn(di["pred"], di["y_cls"], di["y_regr"], m, a, ld_dz, 1)
    pp = di["pred"][:, :a].astype(np.float64)
    _, dp = dense.rpn_loss_cls(di["y_cls"].astype(np.float64)[None, None], pp[None, None], a, False)
    assert np.abs(dz[:, :a] - (dp * pp * (1 - pp))[0, 0])[keep].max() <= 1e-12
    _, dr = dense.smooth_l1_masked(di["y_regr"].astype(np.float64)[None, None], di["pred"][:, a:5 * a].astype(np.float64)[None, None], 4 * a)
    assert np.abs(dz[:, a:5 * a] - dr[0, 0]).max() <= 1e-15
    # detector losses at (20, 7, 24), all background rows aside: generic rows, nothing clipped
    r, nc, nreg = E.DET[2]
    di = E.det_inputs(2, "all_background")
    rows = slice(0, r)
    dz, losses = E.det_rows(di["q"][rows], di["pregr"][rows], di["y1"][rows], di["y2"][rows])
    q64 = di["q"].astype(np.float64)
    lc, dq = dense.class_loss_cls(di["y1"].astype(np.float64)[None], q64[None])
    lr, dr = dense.smooth_l1_masked(di["y2"].astype(np.float64)[None], di["pregr"].astype(np.float64)[None], nreg)
    assert abs(losses[0] - lc) <= 1e-12 * abs(lc) and abs(losses[1] - lr) <= 1e-15
    assert _rel(dz[:, :nc], q64 * (dq[0] - (dq[0] * q64).sum(-1, keepdims=True))) <= 1e-12 and np.abs(dz[:, nc:] - dr[0]).max() <= 1e-15
    dg = E.det_inputs(2, "general")
    dzg, lg = E.det_rows(dg["q"], dg["pregr"], dg["y1"], dg["y2"])
    assert abs(lg[2] - dense.categorical_accuracy(dg["y1"][None], dg["q"][None])) <= 1e-15
    _, drg = dense.smooth_l1_masked(dg["y2"].astype(np.float64)[None], dg["pregr"].astype(np.float64)[None], nreg)
    assert np.abs(dzg[:, nc:] - drg[0]).max() <= 1e-15 and np.abs(drg).max() > 0


def test_head_tail_reference_is_the_chain_of_the_separate_references():
    for i, cs in enumerate(E.HEAD_TAIL):
        d = E.head_tail_inputs(i)
        ref = E.ref_head_tail(cs, d["y5"], d["w"], d["b"], d["y1"], d["y2"], d["live"])
        feat = _inner(E.ref_avgpool_fwd(d["y5"])["y"])
        assert np.array_equal(_inner(ref["feat"]), feat)
        rg = cs.R // cs.groups
        for g in range(cs.groups):
            rows = slice(g * rg, (g + 1) * rg)
            if cs.idle == g:
                assert (_inner(ref["dz"])[rows] == 0).all() and np.isnan(_inner(ref["losses"])[g]).all() and ref["dz"]["zero"][:-E.TAIL].reshape(cs.R, -1)[rows].all()
                continue
            one = E.ref_det(_inner(ref["p_cls"])[rows], _inner(ref["p_regr"])[rows], d["y1"][rows], d["y2"][rows])
            assert np.array_equal(_inner(one["dz"]), _inner(ref["dz"])[rows]) and np.array_equal(_inner(one["losses"]), _inner(ref["losses"])[g])
        inf = E.ref_head_tail(cs, d["y5"], d["w"], d["b"], None, None, None, targets=False)
        assert set(inf) == {"feat", "p_cls", "p_regr"} and np.array_equal(inf["p_cls"]["buf"], ref["p_cls"]["buf"], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- margins
def test_no_decision_of_any_case_is_borderline():
    for i in range(len(E.AVGPOOL)):
        assert E.borderline_act(E.avgpool_inputs(i)["x"]) == 0
    for i, (m, a, _, _) in enumerate(E.RPN):
        for lay in E.RPN_LAYOUTS:
            d = E.rpn_inputs(i, lay)
            assert E.borderline_prob(d["pred"][:, :a]) == 0 and E.borderline_prob(d["y_cls"][:, a:]) == 0, (i, lay)
            assert E.borderline_l1(d["y_regr"][:, 4 * a:], d["pred"][:, a:5 * a]) == 0, (i, lay)
    for i, (r, nc, nreg) in enumerate(E.DET):
        for lay in E.DET_LAYOUTS:
            d = E.det_inputs(i, lay)
            q = d["q"].astype(np.float64)
            assert E.borderline_prob(q / q.sum(-1, keepdims=True)) == 0 and E.borderline_prob((d["q"] / d["q"].sum(-1, keepdims=True, dtype=F)).astype(F)) == 0, (i, lay)
            assert E.borderline_argmax(d["q"]) == 0 and E.borderline_argmax(d["y1"]) == 0, (i, lay)
            assert E.borderline_l1(d["y2"][:, nreg:], d["pregr"]) == 0, (i, lay)
    for i, cs in enumerate(E.HEAD_TAIL):
        d = E.head_tail_inputs(i)
        _, _, z, tz, q = E.head_forward(d["y5"], d["w"], d["b"], cs.nc, cs.nreg)
        assert E.borderline_prob(q) == 0 and E.borderline_argmax(q) == 0 and E.borderline_argmax(d["y1"]) == 0, i
        assert E.borderline_l1(d["y2"][:, cs.nreg:], z[:, cs.nc:].astype(F)) == 0, i
        assert tz.max() + E.MARGIN < E.L1_GAP and E.borderline_act(d["y5"]) == 0          # the device's own p_regr moves no decision


# ---------------------------------------------------------------------------------------------------------------- fp32 stays inside
def _inside(ref, got):
    ins = ref["inside"][:-E.TAIL]
    err = np.abs(np.asarray(got, np.float64).ravel() - ref["buf"][:-E.TAIL])[ins]
    tol = ref["tol"][:-E.TAIL][ins]
    return float((err / np.maximum(tol, 1e-300)).max()) if (err > 0).any() else 0.0


def test_honest_fp32_arithmetic_stays_inside_the_counted_bounds():
    worst = {}
    for mi, (H, W, C) in enumerate(E.ROI_MAPS):
        for ps in (2, 7):
            d = E.roi_inputs(mi, ps)
            ref = E.ref_roi_fwd(d["fmap"], d["rois"], ps)["y"]
            em = E.ref_roi_fwd(d["fmap"], d["rois"], ps, dt=F)["y"]
            assert em["buf"].dtype == np.float64 and E.ref_roi_fwd(d["fmap"][:, :, :4], d["rois"][:1], 1, dt=F)["y"]["shape"] == (1, 1, 1, 4)
            worst["roi_fwd"] = max(worst.get("roi_fwd", 0), _inside(ref, em["buf"][:-E.TAIL]))
            for ordered in (True, False):
                ref = E.ref_roi_bwd(d["dy"], H, W, d["rois"], ps, d["old"], ordered)["dfmap"]
                em = E.ref_roi_bwd(d["dy"], H, W, d["rois"], ps, d["old"], ordered, dt=F)["dfmap"]
                worst["roi_bwd"] = max(worst.get("roi_bwd", 0), _inside(ref, em["buf"][:-E.TAIL]))
    for i in range(len(E.AVGPOOL)):
        x = E.avgpool_inputs(i)["x"]
        s = np.zeros(x[:, 0].shape, F)
        for p in range(x.shape[1]):
            s = s + x[:, p]
        worst["avgpool"] = max(worst.get("avgpool", 0), _inside(E.ref_avgpool_fwd(x)["y"], s / F(x.shape[1])))
    for i, (r, k, ldw, nc, nreg) in enumerate(E.DENSE_FWD):
        d = E.dense_fwd_inputs(i)
        z = d["feat"] @ d["w"][:, nc:nc + nreg] + d["b"][nc:nc + nreg]
        assert z.dtype == F
        worst["dense"] = max(worst.get("dense", 0), _inside(E.ref_dense_fwd(d["feat"], d["w"], d["b"], nc, nreg)["out_regr"], z))
    for i, (r, k, ldw, nout, acc) in enumerate(E.DENSE_BWD):
        d = E.dense_bwd_inputs(i)
        ref = E.ref_dense_bwd(d["feat"], d["dz"], d["w"], ldw, nout, acc, d["dw0"], d["db0"])
        dw = np.zeros((k, ldw), F)
        dw[:, :nout] = d["feat"].T @ d["dz"]
        worst["dw"] = max(worst.get("dw", 0), _inside(ref["dw"], dw + d["dw0"] if acc else dw))
        worst["dfeat"] = max(worst.get("dfeat", 0), _inside(ref["dfeat"], d["dz"] @ d["w"][:, :nout].T))
    print("worst fp32 err / tol:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v < 1.0 for v in worst.values()), worst


def test_avgpool_bwd_reference_is_one_fp32_division():
    for i, (r, hw, c) in enumerate(E.AVGPOOL):
        d = E.avgpool_inputs(i)
        ref = E.ref_avgpool_bwd(d["g"], d["x"])["dx"]
        got = _inner(ref)
        live = d["x"] > 0
        assert np.array_equal(got.astype(F).astype(np.float64), got) and (ref["tol"] == 0).all()
        assert np.array_equal(got[live], np.broadcast_to((d["g"] / F(hw))[:, None, :], got.shape)[live].astype(np.float64)) and (got[~live] == 0).all()
        assert (ref["zero"][:-E.TAIL].reshape(got.shape) == ~live).all() and (~live).any()


# ---------------------------------------------------------------------------------------------------------------- teeth
def _outside(ref, mu):
    """Whether a mutant's outputs leave the reference's bounds: an element off by more than tol (or NaN, or never written), an element
    written that must keep the sentinel, a non-zero where the contract says +0.0, or a write behind the tensor."""
    for name in ref:
        r, m = ref[name], mu[name]
        ins = r["inside"]
        if (~(np.abs(m["buf"][ins] - r["buf"][ins]) <= r["tol"][ins])).any() or (~np.isnan(m["buf"][~ins])).any():
            return True
        if (m["buf"][r["zero"]] != 0).any() or m.get("spilled"):
            return True
    return False


def _maxpool(i, mut=None):
    return E.ref_maxpool(E.maxpool_inputs(i)["x"], *E.MAXPOOL[i][4:], mut=mut)


def _roi_fwd(mi, ps, mut=None):
    d = E.roi_inputs(mi, ps)
    return E.ref_roi_fwd(d["fmap"], d["rois"], ps, mut)


def _roi_bwd(mi, ps, ordered, mut=None):
    d = E.roi_inputs(mi, ps)
    return E.ref_roi_bwd(d["dy"], E.ROI_MAPS[mi][0], E.ROI_MAPS[mi][1], d["rois"], ps, d["old"], ordered, mut)


def _avg_fwd(i, mut=None):
    return E.ref_avgpool_fwd(E.avgpool_inputs(i)["x"], mut)


def _avg_bwd(i, mut=None):
    return E.ref_avgpool_bwd(E.avgpool_inputs(i)["g"], E.avgpool_inputs(i)["x"], mut)


def _dense_fwd(i, mut=None):
    d = E.dense_fwd_inputs(i)
    return E.ref_dense_fwd(d["feat"], d["w"], d["b"], *E.DENSE_FWD[i][3:], mut=mut)


def _dense_bwd(i, mut=None):
    d = E.dense_bwd_inputs(i)
    return E.ref_dense_bwd(d["feat"], d["dz"], d["w"], *E.DENSE_BWD[i][2:], d["dw0"], d["db0"], mut)


def _rpn(i, lay, mode, mut=None):
    d = E.rpn_inputs(i, lay)
    m, a, _, ld_dz = E.RPN[i]
    return E.rpn_outputs(d["pred"], d["y_cls"], d["y_regr"], m, a, ld_dz, mode, mut)


def _det(i, lay, mut=None):
    d = E.det_inputs(i, lay)
    return E.ref_det(d["q"], d["pregr"], d["y1"], d["y2"], mut)


def _tail(i, mut=None):
    d = E.head_tail_inputs(i)
    return E.ref_head_tail(E.HEAD_TAIL[i], d["y5"], d["w"], d["b"], d["y1"], d["y2"], d["live"], True, mut)


# mutant -> [(what the case is, the reference of that case as a function of the mutant)]: EVERY listed case must catch it
CAUGHT_BY = {
    "pool_init_zero": [("maxpool (1,3,3,4,3,2), all inputs negative", lambda m: _maxpool(0, m))],
    "pool_drop_last": [("maxpool (2,7,9,4,3,2)", lambda m: _maxpool(2, m))],
    "roi_round": [("roi_resize fwd (5,7,4) ps 7", lambda m: _roi_fwd(0, 7, m)), ("roi_resize bwd (5,7,4) ps 7", lambda m: _roi_bwd(0, 7, True, m))],
    "roi_no_clamp": [("roi_resize fwd (5,7,4) ps 2", lambda m: _roi_fwd(0, 2, m)), ("roi_resize bwd (6,5,12) ps 2", lambda m: _roi_bwd(1, 2, False, m))],
    "roi_hi_unclamped": [("roi_resize fwd (5,7,4) ps 7", lambda m: _roi_fwd(0, 7, m)), ("roi_resize bwd (4,4,1028) ps 7", lambda m: _roi_bwd(3, 7, True, m))],
    "roi_dedup": [("roi_resize bwd (5,7,4) ps 2", lambda m: _roi_bwd(0, 2, True, m)), ("roi_resize bwd (5,7,4) ps 33", lambda m: _roi_bwd(0, 33, False, m))],
    "avg_div49": [("avgpool fwd (3,2,8)", lambda m: _avg_fwd(2, m)), ("avgpool bwd (2,100,36)", lambda m: _avg_bwd(5, m)),
                  ("head_tail hw 16", lambda m: _tail(2, m))],
    "tail_drop_64": [("head_tail hw 65", lambda m: _tail(5, m)), ("head_tail hw 100", lambda m: _tail(6, m))],
    "no_bias": [("dense_heads fwd (3,100,32,7,24)", lambda m: _dense_fwd(1, m)), ("head_tail (1,1,32,32,2,4)", lambda m: _tail(0, m))],
    "softmax_no_max": [("dense_heads fwd (5,256,64,13,48), biases +-100", lambda m: _dense_fwd(3, m))],
    "acc_ignored": [("dense_heads bwd (20,9,32,32,1)", lambda m: _dense_bwd(1, m)), ("roi_resize bwd (6,5,12) ps 1", lambda m: _roi_bwd(1, 1, True, m))],
    "pad_read": [("rpn_loss (7,12,64,64)", lambda m: _rpn(2, "general", 0, m)), ("dense_heads fwd (1,4,32,2,4)", lambda m: _dense_fwd(0, m))],
    "rpn_no_eps": [("rpn_loss (1,1,5,5) all valid", lambda m: _rpn(0, "all_valid", 1, m)), ("rpn_loss (3,2,10,12)", lambda m: _rpn(1, "general", 0, m))],
    "l1_threshold": [("rpn_loss (50,9,45,64)", lambda m: _rpn(3, "general", 0, m)), ("det_loss (20,7,24)", lambda m: _det(2, "general", m))],
    "det_batch_norm": [("head_tail (6,64,32,32,7,24) in 2 groups", lambda m: _tail(4, m))],
    "idle_live": [("head_tail (6,16,32,64,13,48), first group idle", lambda m: _tail(2, m)), ("head_tail, last group idle", lambda m: _tail(3, m))],
    "acc_last_max": [("det_loss (20,7,24), tie with the label on the second maximum", lambda m: _det(2, "general", m))],
}


@pytest.mark.parametrize("mut", E.MUTANTS)
def test_every_mutant_leaves_the_bound_of_its_named_case(mut):
    assert set(CAUGHT_BY) == set(E.MUTANTS)
    for what, run in CAUGHT_BY[mut]:
        ref = run(None)
        assert not _outside(ref, run(None)), ("the reference itself", what)
        assert _outside(ref, run(mut)), (mut, "is not caught by", what)
