"""Device-free checks of tests/fp32_edge_cases.py, the case table and references of tests/test_gpu_fp32_edges.py:

  * the references are right: they equal oracle.dense.conv2d / conv2d_bwd in float64 to 1e-12 of the largest value, and the cases
    with asymmetric padding or kh != kw also equal an explicit loop over pixels and taps written here;
  * the table respects the launchers' constraints, its comments' tile counts are true, every forced split exists;
  * the bound has teeth: every mutant of the reference that applies to a case (a pitch misread, swapped padding, a dropped tap, ...)
    differs from the true reference by more than 4 * tol somewhere, and no case is left without one."""
import numpy as np
import pytest

import fp32_edge_cases as F
from oracle import dense

ALL = [(name, side) for name, cs in F.CASES.items() for side in F.sides(cs)]


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max()) <= 1e-12 * max(float(np.abs(b).max()), 1e-300)


def _g(name):
    d = F.inputs(name)
    return (d["dy"] * d["gscale"][None, :] if d["gscale"] is not None else d["dy"]).astype(np.float64)


def _raw(name, side, mode=0):
    """The sums before the epilogue, recovered from the reference's output where the epilogue is invertible."""
    cs, d, r = F.CASES[name], F.inputs(name), F.compute(name, side, mode)
    if side == "fwd":
        return (r["pre"] - d["shift"].astype(np.float64) - d["addend"].astype(np.float64)) / d["scale"].astype(np.float64)
    if side == "dgrad":
        out = r["out"] - (d["dx_add"].astype(np.float64) if d["dx_add"] is not None else 0.0)
        return out, (d["dx_mask"] > 0 if d["dx_mask"] is not None else np.ones(out.shape, bool))
    return r["out"] - (d["dw0"].astype(np.float64) if mode == 1 else 0.0)


@pytest.mark.parametrize("name,side", ALL)
def test_reference_equals_the_oracle(name, side):
    cs, d, g = F.CASES[name], F.inputs(name), F.geometry(F.CASES[name], side)
    w4 = d["w"].astype(np.float64).reshape(cs.kh, cs.kw, cs.c, cs.n)
    scale = max(1.0, float(np.abs(F.compute(name, side)["out"]).max()))
    if side == "fwd":
        y = dense.conv2d(d["x"].astype(np.float64), w4, None, cs.stride, cs.pad)
        assert y.shape == (cs.nb, g["oh"], g["ow"], cs.n)
        got = _raw(name, side)
        assert np.abs(got - y.reshape(g["M"], cs.n)).max() <= 1e-12 * scale
        return
    gm = _g(name).reshape(cs.nb, g["oh"], g["ow"], cs.n)
    x = d["x"].astype(np.float64) if side == "wgrad" else np.zeros((cs.nb, cs.h, cs.w, cs.c))
    dx, dw, db = dense.conv2d_bwd(x, w4, gm, cs.stride, cs.pad, need_dx=side == "dgrad")
    if side == "dgrad":
        got, keep = _raw(name, side)
        assert dx.shape == (cs.nb, cs.h, cs.w, cs.c)
        assert np.abs(np.where(keep, got - dx.reshape(g["P"], cs.c), 0.0)).max() <= 1e-12 * scale
        assert (F.compute(name, side)["out"][~keep] == 0).all()
    else:
        for mode in cs.opts["modes"]:
            assert _close(_raw(name, side, mode), dw.reshape(g["K"], cs.n))
            r = F.compute(name, side, mode)
            assert _close(r["db"] - (d["db0"].astype(np.float64) if mode == 1 else 0.0), db)


def _loop_conv(x, w4, stride, pt, pl, oh, ow):
    """y[b][oy][ox][:] = sum over taps inside the image of x[b][iy][ix][:] @ w[ky][kx] -- one pixel and one tap at a time."""
    nb, h, w, _ = x.shape
    kh, kw, _, n = w4.shape
    y = np.zeros((nb, oh, ow, n))
    for b in range(nb):
        for oy in range(oh):
            for ox in range(ow):
                for ky in range(kh):
                    for kx in range(kw):
                        iy, ix = oy * stride - pt + ky, ox * stride - pl + kx
                        if 0 <= iy < h and 0 <= ix < w:
                            y[b, oy, ox] += x[b, iy, ix] @ w4[ky, kx]
    return y


def _loop_dgrad(gm, w4, pt, pl, h, w):
    """Stride 1: every output pixel scatters g[b][oy][ox][:] @ w[ky][kx]^T to the input pixel its tap read."""
    nb, oh, ow, _ = gm.shape
    kh, kw, c, _ = w4.shape
    dx = np.zeros((nb, h, w, c))
    for b in range(nb):
        for oy in range(oh):
            for ox in range(ow):
                for ky in range(kh):
                    for kx in range(kw):
                        iy, ix = oy - pt + ky, ox - pl + kx
                        if 0 <= iy < h and 0 <= ix < w:
                            dx[b, iy, ix] += w4[ky, kx] @ gm[b, oy, ox]
    return dx


def _loop_wgrad(x, gm, kh, kw, stride, pt, pl):
    nb, h, w, c = x.shape
    _, oh, ow, n = gm.shape
    dw = np.zeros((kh, kw, c, n))
    for b in range(nb):
        for oy in range(oh):
            for ox in range(ow):
                for ky in range(kh):
                    for kx in range(kw):
                        iy, ix = oy * stride - pt + ky, ox * stride - pl + kx
                        if 0 <= iy < h and 0 <= ix < w:
                            dw[ky, kx] += np.outer(x[b, iy, ix], gm[b, oy, ox])
    return dw


ODD_GEOMETRY = [(n, s) for n, s in ALL if F.CASES[n].kh != F.CASES[n].kw or len(set(F.CASES[n].pad)) > 1]


@pytest.mark.parametrize("name,side", ODD_GEOMETRY)
def test_asymmetric_and_non_square_cases_equal_an_explicit_loop(name, side):
    cs, d, g = F.CASES[name], F.inputs(name), F.geometry(F.CASES[name], side)
    w4 = d["w"].astype(np.float64).reshape(cs.kh, cs.kw, cs.c, cs.n)
    pt, pl = cs.pad[:2]
    if side == "fwd":
        assert _close(_raw(name, side), _loop_conv(d["x"].astype(np.float64), w4, cs.stride, pt, pl, g["oh"], g["ow"]).reshape(g["M"], cs.n))
    elif side == "dgrad":
        got, keep = _raw(name, side)
        want = _loop_dgrad(_g(name).reshape(cs.nb, g["oh"], g["ow"], cs.n), w4, pt, pl, cs.h, cs.w).reshape(g["P"], cs.c)
        assert np.abs(np.where(keep, got - want, 0.0)).max() <= 1e-12 * max(1.0, float(np.abs(want).max()))
    else:
        want = _loop_wgrad(d["x"].astype(np.float64), _g(name).reshape(cs.nb, g["oh"], g["ow"], cs.n), cs.kh, cs.kw, cs.stride, pt, pl)
        assert _close(_raw(name, side, cs.opts["modes"][0]) if cs.opts["modes"][0] != 1 else _raw(name, side, 1), want.reshape(g["K"], cs.n))


def test_odd_geometry_list_is_what_the_table_says():
    names = {n for n, _ in ODD_GEOMETRY}
    assert {"f_s2_pad_br", "f_pad_t_ne_l", "f_1x3", "f_3x1", "d_pad_t_ne_l", "d_1x3", "d_3x1", "w_pad_br", "w_1x3", "w_3x1_s2"} <= names


def test_general_gather_is_the_shared_im2col():
    """The gather the mutants are built from is, unmutated, the im2col / col2im_gather of tests/bf16_edge_cases.py."""
    for name in ("f_s2_pad_br", "f_1x3", "f_stem", "w_3x1_s2"):
        cs, d, g = F.CASES[name], F.inputs(name), F.geometry(F.CASES[name])
        A = F.gather(d["x"], cs.nb, cs.h, cs.w, g["oh"], g["ow"], cs.kh, cs.kw, cs.stride, cs.pad[0], cs.pad[1])
        assert np.array_equal(A.reshape(g["M"], -1), F.im2col(d["x"], cs))
    for name in ("d_pad_t_ne_l", "d_1x3", "d_valid_3x3"):
        cs, g = F.CASES[name], F.geometry(F.CASES[name])
        gm = _g(name)
        A = F.gather(gm.reshape(cs.nb, g["oh"], g["ow"], cs.n), cs.nb, g["oh"], g["ow"], cs.h, cs.w, cs.kh, cs.kw, 1, cs.kh - 1 - cs.pad[0],
                     cs.kw - 1 - cs.pad[1])
        assert np.array_equal(A[:, ::-1, ::-1, :].reshape(g["P"], -1), F.col2im_gather(gm, cs))


def test_g_is_one_fp32_multiply():
    d = F.inputs("d_same_3x3_all")
    g32 = d["dy"] * d["gscale"][None, :]
    assert g32.dtype == np.float32
    assert not np.array_equal(g32.astype(np.float64), d["dy"].astype(np.float64) * d["gscale"].astype(np.float64)[None, :])


# ---------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("name", list(F.CASES))
def test_case_respects_the_launchers_and_its_comment(name):
    cs, p = F.CASES[name], F.pitches(F.CASES[name])
    for side in F.sides(cs):
        g = F.geometry(cs, side)
        for key, want in cs.expect.items():
            if key != "nrt" or side == F.sides(cs)[0]:
                assert g[key] == want, (name, key, g[key])
        if side == "fwd":
            assert (cs.c % 32 == 0 or cs.c == 4) and cs.n % 4 == 0 and (cs.kh * cs.kw <= 32 or cs.c == 4)
            assert p["ldw"] % 4 == 0 and p["ldw"] > cs.n and p["ldy"] > cs.n and p["ld_add"] > cs.n
            assert len({p["ldw"], p["ldy"], p["ld_add"]}) == 3
            assert (g["oh"] - 1) * cs.stride - cs.pad[0] < cs.h and (g["ow"] - 1) * cs.stride - cs.pad[1] < cs.w
        elif side == "dgrad":
            assert cs.stride == 1 and cs.n % 32 == 0 and cs.c % 4 == 0 and p["ld_dy"] == cs.n and cs.kh * cs.kw <= 32
            assert p["ldw"] % 4 == 0 and len({cs.c, p["ld_dx"], p["ld_dx_add"], p["ld_dx_mask"]}) == 4 and p["ld_dx"] > cs.c
            assert cs.kh - 1 - cs.pad[0] >= 0 and cs.kw - 1 - cs.pad[1] >= 0
        else:
            assert cs.c % 64 == 0 and cs.n % 4 == 0 and p["ld_dy"] % 4 == 0 and p["ldw"] % 4 == 0 and p["ldw"] > cs.n
            assert cs.kind == "bwd" or p["ld_dy"] > cs.n
        if name not in F.ODD_PITCH:
            assert all(v % 4 == 0 for v in p.values()), p
        # every forced split satisfies the launchers' condition (forward / dgrad: nk / s >= 1; wgrad: a 32-row tile per split)
        for s in cs.splits:
            assert g["nrt"] // s >= 1, (name, side, s, g["nrt"])
        if side == "wgrad":
            shapes, left = F.wgrad_shapes(cs)
            assert {s for _, _, s in shapes} >= set(cs.splits) | {1}
            assert any(bmk == 128 for bmk, _, _ in shapes) == (cs.c % 128 == 0)
        else:
            shapes, left = F.igemm_shapes(cs, side)
            n_tiles = 8 if cs.c == 4 and side == "fwd" else 10              # 4 tiles x {4, 8} waves + the two 32-row tiles (not the stem)
            assert len(shapes) == n_tiles * (2 + 2 * len(cs.splits)) and left == (10 - n_tiles) * (2 + 2 * len(cs.splits))


def test_table_reaches_every_edge_the_issue_names():
    C = F.CASES
    g = {n: F.geometry(cs) for n, cs in C.items()}
    assert g["f_ragged_mn"]["M"] == 2 * 64 + 7 and C["f_ragged_mn"].n == 64 + 4 and g["f_ragged_mn"]["nrt"] == 1
    assert g["f_same_3x3_two_images"]["M"] // 2 % 64 != 0                      # the image boundary lies inside a tile
    assert g["f_deep_k"]["M"] < 64 and C["f_deep_k"].splits == (2, 3, 33) and C["d_deep"].splits == (2, 3, 99)
    assert g["w_deep_m"]["M"] == 33 * 32 + 29 and C["w_deep_m"].splits == (2, 3, 8)
    assert g["d_valid_3x3"]["oh"] == 5 and C["d_valid_3x3"].kh - 1 - C["d_valid_3x3"].pad[0] == 2
    assert C["f_5x5"].kh * C["f_5x5"].kw == 25 and C["f_stem"].c == 4
    assert (np.abs(F.inputs("f_stem")["x"][..., 3]) > 0).all()                 # the fourth channel is NOT zero
    assert F.pitches(C["f_col_block"])["ldy"] == 2 * C["f_col_block"].n
    opts = {(bool(c.opts.get("dx_add")), bool(c.opts.get("dx_mask"))) for c in C.values() if c.kind == "dgrad"}
    assert opts == {(True, True), (False, False), (True, False), (False, True)}
    assert any(c.kind == "wgrad" and c.c % 128 == 0 for c in C.values())
    assert {m for c in C.values() if c.kind == "wgrad" and c.opts.get("db") for m in c.opts["modes"]} == {0, 1, 2}
    for name in F.ODD_PITCH:
        assert any(v % 4 for v in F.pitches(C[name]).values())


# ---------------------------------------------------------------------------------------------------------------- teeth
def _caught(m, r, key="out", tol="tol"):
    return bool((~np.isfinite(m[key]) | (np.abs(m[key] - r[key]) > 4 * r[tol])).any())


@pytest.mark.parametrize("name,side", ALL)
def test_every_applicable_mutant_is_outside_four_times_the_bound(name, side):
    cs = F.CASES[name]
    modes = cs.opts.get("modes", (0,)) if side == "wgrad" else (0,)
    applied, not_applicable = [], []
    for mut in F.MUTANTS:
        hit = [mode for mode in modes if F.applies(mut, cs, side, mode)]
        if not hit:
            not_applicable.append(mut)
            continue
        for mode in hit:
            r, m = F.compute(name, side, mode), F.mutant(name, side, mode, mut)
            assert np.isfinite(r["out"]).all() and (r["tol"] >= 0).all() and r["out"].shape == r["tol"].shape == m["out"].shape
            if mut == "db_without_gscale":
                assert _caught(m, r, "db", "db_tol"), (name, side, mode, mut)
            else:
                assert _caught(m, r), (name, side, mode, mut, float(np.nanmax(np.abs(m["out"] - r["out"]) / np.maximum(r["tol"], 1e-300))))
        applied.append(mut)
    print("%s/%s: caught %s; not applicable: %s" % (name, side, ", ".join(applied), ", ".join(not_applicable)))
    assert "drop_last_k_tile" in applied and len(applied) >= 2, (name, side, applied)
    assert sorted(applied + not_applicable) == sorted(F.MUTANTS)


def test_every_mutant_applies_somewhere():
    for mut in F.MUTANTS:
        assert any(F.applies(mut, cs, side, mode) for cs in F.CASES.values() for side in F.sides(cs) for mode in cs.opts.get("modes", (0,))), mut


def test_bound_is_the_stated_formula():
    """tol = (K_red + 8) * 2^-24 * (absdot * |scale| + |shift| + |addend|), sigmoid columns a quarter of it plus the slack."""
    name = "f_s2_pad_br"
    cs, d, r, g = F.CASES[name], F.inputs(name), F.compute(name), F.geometry(F.CASES[name])
    base = (g["K"] + 8) * 2.0 ** -24 * (r["absdot"] * np.abs(d["scale"].astype(np.float64)) + np.abs(d["shift"].astype(np.float64))
                                         + np.abs(d["addend"].astype(np.float64)))
    ac = cs.opts["act_cols"]
    assert np.array_equal(r["tol"][:, ac:], base[:, ac:]) and np.allclose(r["tol"][:, :ac], 0.25 * base[:, :ac] + F.SIGMOID_SLACK, rtol=1e-15)
    assert ((r["out"][:, :ac] > 0) & (r["out"][:, :ac] < 1)).all()
    r = F.compute("w_ragged_db", "wgrad", 1)
    d = F.inputs("w_ragged_db")
    assert np.array_equal(r["tol"], (135 + 8) * 2.0 ** -24 * (r["absdot"] + np.abs(d["dw0"].astype(np.float64))))
    assert r["db_tol"].shape == (68,) and (r["db_tol"] > 0).all()
