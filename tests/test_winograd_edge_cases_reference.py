"""Device-free checks of tests/winograd_edge_cases.py, the case table and per-stage references of tests/test_gpu_winograd_edges.py:

  * the stages compose: in float64, filter -> input -> per-position products -> output equals oracle.dense.conv2d, and input -> dy ->
    reduction over tiles -> filter_grad equals oracle.dense.conv2d_bwd's dw, to 1e-12 of the largest value, every case, both forms;
  * the bound is wide enough for honest fp32: an emulation of every stage in the kernels' association and one as plain matrix products
    stay inside it; on the integer-valued inputs the emulation of the exact stages equals float64 bit for bit;
  * the bound has teeth: every mutant that applies to a case lies outside 4 * tol somewhere (or writes outside the rows), every mutant
    that does not apply changes nothing, and every mutant applies somewhere;
  * the table's tile / unit / workgroup counts are true and it reaches every edge the suite is about."""
import numpy as np
import pytest

import winograd_edge_cases as W
from oracle import dense

ALL = [(name, form) for name in W.CASES for form in W.FORMS]
RUNS = [(name, form, stage, var) for name, form in ALL for stage in W.STAGES for var in W.variants(stage)]


def _rel(a, b):
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-300)


@pytest.mark.parametrize("name,form", ALL)
def test_stages_compose_to_the_convolution_and_its_weight_gradient(name, form):
    cs, d = W.CASES[name], W.inputs(name, form)
    g = W.geometry(cs, form)
    w4, x = d["w"].astype(np.float64).reshape(3, 3, cs.c, cs.n), d["x"].astype(np.float64)
    take = lambda r: r["buf"][r["inside"]].reshape(r["shape"])
    u = take(W.stage_filter(d["w"], cs.c, cs.n, cs.n, form))
    v = take(W.stage_input(d["x"], form))
    assert u.shape == (g["P"], cs.c, cs.n) and v.shape == (g["P"], g["T"], cs.c)
    m = W.ref_gemm(v, u)
    m = m["buf"][m["inside"]].reshape(m["shape"])
    y = W.stage_output(m, cs.nb, cs.h, cs.w, cs.n, cs.n, form)
    y = y["buf"].reshape(y["shape"])[:-1]
    assert _rel(y, dense.conv2d(x, w4, None, 1, (1, 1, 1, 1)).reshape(g["rows"], cs.n)) <= 1e-12
    # gradient: g = fl32(dy * gscale), as the dy stage states it
    gm = (d["dy"] * d["gscale"][None, :]).astype(np.float64)
    dz = take(W.stage_dy(d["dy"], cs.nb, cs.h, cs.w, cs.n, cs.n, form, d["gscale"]))
    du = W.ref_wgrad(v, dz)
    du = du["buf"][du["inside"]].reshape(du["shape"])
    dw = W.stage_filter_grad(du, cs.c, cs.n, cs.n, form)
    dw = dw["buf"].reshape(dw["shape"])[:-1]
    _, dw_ref, _ = dense.conv2d_bwd(x, np.zeros_like(w4), gm.reshape(cs.nb, cs.h, cs.w, cs.n), 1, (1, 1, 1, 1), need_dx=False)
    assert _rel(dw, dw_ref.reshape(9 * cs.c, cs.n)) <= 1e-12


def test_kernel_association_is_the_published_matrices():
    """The 1-D forms written after radnet_wino4.h / the F(2x2) kernels, in float64, are the literal matrices."""
    rs = np.random.RandomState(1)
    for form in W.FORMS:
        for kind, fn in W.ONE_D[form].items():
            L = W.matrices(form)[kind]
            X = rs.standard_normal((L.shape[1], 5))
            assert np.abs(np.stack(fn(list(X))) - L @ X).max() <= 1e-14, (form, kind)


@pytest.mark.parametrize("name,form", ALL)
def test_fp32_emulations_stay_inside_the_bound_and_integers_are_exact(name, form):
    worst = 0.0
    for stage in W.STAGES:
        for var in W.variants(stage):
            for ints in (False, True):
                ref = W.compute(name, form, stage, var, ints)
                ins = ref["inside"]
                assert not np.isnan(ref["buf"][ins]).any() and np.isnan(ref["buf"][~ins]).all()
                for arith in ("kernel", "matmul"):
                    em = W.emulate(name, form, stage, var, ints, arith)
                    err = np.abs(em["buf"][ins].astype(np.float64) - ref["buf"][ins])
                    assert (err <= ref["tol"][ins]).all(), (name, form, stage, var, ints, arith, float((err / np.maximum(ref["tol"][ins], 1e-300)).max()))
                    worst = max(worst, float((err / np.maximum(ref["tol"][ins], 1e-300)).max()))
                    if ints and stage in W.EXACT[form]:
                        assert np.array_equal(em["buf"][ins].astype(np.float64), ref["buf"][ins]), (name, form, stage, var, arith)
                        assert np.array_equal(ref["buf"][ins].astype(np.float32).astype(np.float64), ref["buf"][ins])      # fp32 holds it
    print("%s F(%dx%d): worst fp32 emulation err / tol %.3f" % (name, form, form, worst))
    assert worst < 1.0


def test_emulation_runs_in_fp32():
    """An emulation that silently ran in float64 would prove nothing: its intermediate type is float32."""
    x = np.ones((6, 6, 2, 4), np.float32)
    for arith in ("kernel", "matmul"):
        assert W.transform("input", 4, x, arith).dtype == np.float32
        assert W.transform("filter", 4, x[:3, :3], arith).dtype == np.float32
        assert W.transform("filter_grad", 2, x[:4, :4], arith).dtype == np.float32


def _outside(ref, mu):
    """Whether a mutant's buffer differs from the reference's: an element inside the rows off by more than 4 * tol (or never written,
    or NaN), or an element outside the rows written."""
    ins = ref["inside"]
    return bool((~(np.abs(mu["buf"][ins] - ref["buf"][ins]) <= 4 * ref["tol"][ins])).any() or (~np.isnan(mu["buf"][~ins])).any())


def test_every_mutant_fails_where_it_applies_and_changes_nothing_elsewhere():
    hit = {m: 0 for m in W.MUTANTS}
    for name, form, stage, var in RUNS:
        cs = W.CASES[name]
        ref = W.compute(name, form, stage, var)
        for mut in W.MUTANTS:
            touches = mut in {"filter": ("transpose_p", "g_24_to_12"),
                              "input": ("replicate", "no_image_pad", "swap_titj", "transpose_p", "bt_5_to_4"),
                              "output": ("overrun", "swap_titj", "transpose_p", "dense_ldy", "shift_dropped_without_scale", "relu_without_act"),
                              "dy": ("swap_titj", "transpose_p", "dense_ld_dy", "no_gscale", "gscale_next_quad"),
                              "filter_grad": ("transpose_p", "g_24_to_12", "accumulate_drops_old")}[stage]
            if not touches:
                assert not W.applies(mut, cs, form, stage, var), (mut, stage)
                continue
            mu = W.mutant(name, form, stage, var, mut)
            if W.applies(mut, cs, form, stage, var):
                assert _outside(ref, mu), (name, form, stage, var, mut)
                hit[mut] += 1
            else:
                same = np.array_equal(mu["buf"], ref["buf"], equal_nan=True)
                assert same, ("a mutant said not to apply changes the result", name, form, stage, var, mut)
    assert all(hit.values()), hit


def test_batched_references_have_teeth():
    rs = np.random.RandomState(3)
    for batch, T, c, n in W.BATCHED:
        v, u, dz = rs.standard_normal((batch, T, c)), rs.standard_normal((batch, c, n)), rs.standard_normal((batch, T, n))
        old = rs.standard_normal((batch, c, n))
        ref = W.ref_gemm(v, u)
        v2 = v.copy()
        v2[:, :, -1] = 0                                                                              # the last k dropped
        assert _outside(ref, W.ref_gemm(v2, u))
        got = (v.astype(np.float32) @ u.astype(np.float32)).astype(np.float64).ravel()               # fp32 products stay inside
        ins = ref["inside"]
        assert (np.abs(got - ref["buf"][ins]) <= ref["tol"][ins]).all()
        ref = W.ref_wgrad(v, dz, old)
        assert _outside(ref, W.ref_wgrad(v, dz, old, "accumulate_drops_old"))
        assert T == 1 or _outside(W.ref_wgrad(v, dz), W.ref_wgrad(v2[:, ::-1], dz))                    # rows paired with the wrong tile


def test_table_counts_and_reach():
    forms = {}
    for name, cs in W.CASES.items():
        assert cs.c % 4 == 0 and cs.n % 4 == 0
        assert not cs.chain or cs.c % 32 == 0
        assert "g" not in cs.chain or cs.c % 64 == 0
        for form in W.FORMS:
            g = W.geometry(cs, form)
            assert cs.expect[form] == (g["T"], g["in_units"], g["out_units"], -(-g["in_units"] // 64), -(-g["out_units"] // 64)), (name, form)
            assert len(W.tile_list(cs.nb, cs.h, cs.w, form)) == g["T"]
            forms.setdefault(form, []).append((cs, g))
    sizes = {(cs.h, cs.w) for cs in W.CASES.values()}
    assert {(1, 1), (1, 5), (2, 3), (3, 2), (4, 4), (5, 7), (6, 9), (7, 8)} <= sizes
    assert {h % 4 for h, _ in sizes} == {0, 1, 2, 3} and {w % 4 for _, w in sizes} == {0, 1, 2, 3}
    assert {cs.nb for cs in W.CASES.values()} >= {1, 2, 3}
    assert {cs.n for cs in W.CASES.values()} >= {4, 36, 68} and {cs.c for cs in W.CASES.values() if not cs.chain} >= {4, 36}
    for form, lst in forms.items():
        assert any(min(cs.h, cs.w) < form for cs, _ in lst)                                          # a map smaller than a tile
        assert any(g["in_units"] > 256 and g["out_units"] > 256 for _, g in lst)                     # a second grid-stride block
        assert any(cs.chain == "f" for cs, _ in lst) and any(cs.chain == "fg" for cs, _ in lst)
    # the six-wave kernels: more than one workgroup with the last one partly live
    assert any(g["in_units"] > 64 and g["in_units"] % 64 for _, g in forms[4]) and any(g["out_units"] > 64 and g["out_units"] % 64 for _, g in forms[4])
    assert any(cs.chain and g["T"] == 1 and cs.c == 32 and cs.n == 4 for cs, g in forms[4])            # T = 1, one K tile, n % 32 != 0
    p = [W.pitches(cs) for cs in W.CASES.values()]
    assert all(q["ldw"] == cs.n + 4 and q["ldy"] == cs.n + 8 and q["ld_dy"] == cs.n + 12 for q, cs in zip(p, W.CASES.values()))
    assert len(W.EPILOGUES) == 8 and len(set(W.EPILOGUES)) == 8
    assert {s[1] for s in W.BATCHED} == {1, 23, 75} and {s[3] for s in W.BATCHED} == {4, 36, 96}
    assert {s[2] for s in W.BATCHED} == {32, 64, 128} and {s[0] for s in W.BATCHED} == {16, 36}
    for batch, T, c, n in W.BATCHED:
        shapes = W.gemm_shapes(batch, n)
        assert {s[2] for s in shapes} >= {1, -1, 2, 3, -4, 5, 7, -12} and len(shapes) >= 5 * 2 + 3 * 6
        assert c % 64 or len(W.wgrad_shapes(c, n)) >= 2


def test_s_is_the_documented_count():
    per_pass = {4: dict(filter=4, input=3, output=4, dy=3, filter_grad=5), 2: dict(filter=3, input=1, output=2, dy=1, filter_grad=3)}
    epilogue = dict(filter=0, input=0, output=2, dy=0, filter_grad=1)
    for form in W.FORMS:
        for stage in W.STAGES:
            assert W.S[form][stage] == 2 * per_pass[form][stage] + epilogue[stage] <= 13
    # the multiply by gscale is one rounding more, and only where there is a gscale
    for form in W.FORMS:
        with_gs, without = W.compute("s_2x3", form, "dy", True), W.compute("s_2x3", form, "dy", False)
        bound = W.absbound("dy", form, W.dy_blocks(W.inputs("s_2x3", form)["dy"], 3, 2, 3, form)).ravel()
        assert np.allclose(without["tol"][without["inside"]], W.S[form]["dy"] * W.U * bound, rtol=1e-12, atol=0)
        assert (with_gs["tol"][with_gs["inside"]] > 0).any() and W.S[form]["dy"] + 1 <= 13
