"""Device-free checks of tests/fused_fwd_edge_cases.py, the case tables and references of tests/test_gpu_fused_fwd_edges.py:

  * the tables say what their comments claim (M, chunk counts, the rows that straddle M inside a lane's registers, the pitches) and
    respect what the two entry points take in their one-launch form;
  * the references are right: layer by layer they equal oracle.dense.conv2d in float64, the gather equals the shared im2col, a
    launch emulated one output tile at a time fills the same buffers;
  * the bounds are the stated formulas, an fp32 NumPy emulation of each path (two summation orders) lies inside them on every element
    of every case -- nothing masked, nothing skipped --, and the integer cases are exact in fp32 by their magnitudes;
  * the bounds have teeth: every mutant of the reference misses 4 x the bound, or leaves a hole / a spill, on each case named for it.

Achieved factors (worst |mutant - reference| / bound; inf = NaN padding taken in, an element never written, or one written outside
the rows; `-s` prints them):
  pair   add_with_ldy inf, y_with_ld_add inf (p_pitch); wrap_taps 2.3e+04 (p_3x3_two_images); second_with_n1 inf (p_n_order, every
         tile; silent on p_n_order_swapped, which is why both orders run); gx1_for_second inf (p_diff_m, every tile)
  bneck  add_with_ldy inf, y_with_ld_add inf (b_pitch); shift_prev_chunk 2.6e+03 (b_n2_320 + next), 1.7e+03 (b_m_seams_65);
         w3_no_chunk_offset 180 (b_m_seams_65 + next), 202 (b_n2_320 + next); no_relu 6.9e+03, no_relu_2 4.1e+03 (b_relu_exact);
         wrap_taps 7.2e+03 (b_two_images), 8.1e+03 (b_w1 + next); store_row_m inf (b_m_small, b_m_seams_65 + next)
The fp32 emulations stay below 0.2 of the bound on every case.
"""
import numpy as np
import pytest

import fp32_edge_cases as F32
import fused_fwd_edge_cases as F
from oracle import dense

PAIR_RUN = [n for n, cs in F.PAIRS.items() if cs.tiles]
EMULATED = [(n, nx) for n, cs in F.BNECKS.items() if n not in F.PITCHED_INTERMEDIATE for nx in cs.forms]


def _cpu_verdict(got, ref):
    """Worst factor over every buffer of a CPU result (NaN = untouched); (factor, outside the bound, spilled)."""
    worst, bad, spilled = 0.0, 0, 0
    assert sorted(got.val) == sorted(ref.val)
    for key in ref.val:
        w, b, s = F.verdict(got.val[key], np.isnan(got.val[key]), ref.val[key], ref.tol[key])
        worst, bad, spilled = max(worst, w), bad + b, spilled + s
    return worst, bad, spilled


# ---------------------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("name", list(F.PAIRS))
def test_pair_case_is_what_its_comment_says(name):
    cs = F.PAIRS[name]
    (l1, l2), g1, g2 = cs.layers, F.grid(cs.shapes[0], cs.layers[0]), F.grid(cs.shapes[1], cs.layers[1])
    assert g1[2] == cs.expect["M"]
    if "nk" in cs.expect:
        assert F.cdiv(g1[3], 32) == cs.expect["nk"]
    for l in cs.layers:
        assert l.n % 4 == 0 and l.ldw % 4 == 0 and l.ldw >= l.n and l.ldy >= l.n and (not l.addend or l.ld_add >= l.n)
    takes = g1[2] == g2[2] and g1[3] == g2[3] and l1.c == l2.c and l1.k == l2.k and l1.stride == l2.stride and l1.c % 32 == 0
    assert takes == bool(cs.tiles), "the paired launch takes exactly the cases that name tiles"
    assert (name in F.PAIR_FALLBACK_SHAPES) == (not cs.tiles)
    b = F.pair(name)
    for i in range(2):
        key, c0, ld = F.pair_slot(cs, i)
        assert b.val[key].shape == (cs.expect["M"] + 1 if i == 0 or cs.tiles else F.grid(cs.shapes[1], l2)[2] + 1, ld)


def test_pair_table_reaches_every_edge_the_issue_names():
    P = F.PAIRS
    assert P["p_ragged"].expect["M"] == 2 * 64 + 7 and [l.n for l in P["p_ragged"].layers] == [68, 36]
    assert {F.cdiv(68, bn) for _, bn in F.TILES} == {2, 3} and {F.cdiv(36, bn) for _, bn in F.TILES} == {1, 2}
    assert [l.n for l in P["p_n_order"].layers] == [36, 132] and [l.n for l in P["p_n_order_swapped"].layers] == [132, 36]
    assert P["p_s2_1x1"].layers[0].stride == 2 and P["p_s2_1x1"].layers[0].c == 64 and P["p_s2_1x1"].expect["M"] == 147
    a, b = P["p_3x3_two_images"].layers
    assert (a.act, a.addend, a.scale, a.shift) == (1, True, True, True) and (b.act, b.act_cols, b.scale) == (2, 20, False)
    assert 99 % 64 != 0 and 99 % 32 != 0                                  # the image seam (row 99) lies inside a tile of either height
    assert not P["p_two_inputs"].same_x and F.pair_inputs("p_two_inputs")["x1"] is not F.pair_inputs("p_two_inputs")["x2"]
    assert P["p_deep_k"].expect["nk"] == 33
    pitches = [v for l in P["p_pitch"].layers for v in (l.ldy, l.ld_add)]
    assert len(set(pitches)) == 4 and all(l.ldw > l.n and l.ldy > l.n and l.ld_add > l.n for l in P["p_pitch"].layers)
    l1, l2 = P["p_col_blocks"].layers
    assert l1.ldy == l2.ldy == l1.n + l2.n + 8 and F.pair_slot(P["p_col_blocks"], 1)[:2] == ("y", l1.n)
    y = F.pair("p_col_blocks").val["y"]
    assert np.isnan(y[:, l1.n + l2.n:]).all() and np.isnan(y[-1]).all() and np.isfinite(y[:-1, :l1.n + l2.n]).all()
    assert F.grid(P["p_diff_m"].shapes[0], P["p_diff_m"].layers[0])[2] != F.grid(P["p_diff_m"].shapes[1], P["p_diff_m"].layers[1])[2]
    assert P["p_stem"].layers[0].c == 4


@pytest.mark.parametrize("name", list(F.BNECKS))
def test_bottleneck_case_is_what_its_comment_says(name):
    cs = F.BNECKS[name]
    lb, lc, la = cs.layers
    M = cs.shape[0] * cs.shape[1] * cs.shape[2]
    assert M == cs.expect["M"] and M <= 198
    assert lc.n // 64 == cs.expect.get("chunks", lc.n // 64) and 9 * lb.c == cs.expect.get("K1", 9 * lb.c)
    for bm in (64, 32):
        if "straddle%d" % bm in cs.expect:
            assert F.straddling(M, bm) == cs.expect["straddle%d" % bm], (name, bm, F.straddling(M, bm))
    # what radnet_conv_bottleneck takes as one launch, as its header and guard state it -- the pitched intermediates included in the refusals
    takes = (lb.k == 3 and lb.pad == 1 and lb.stride == 1 and lb.n == 64 and lb.act == 1 and not lb.addend and lb.c % 32 == 0 and cs.linked
             and lc.c == 64 and lc.act == 1 and lc.n % 64 == 0 and lb.ldy == lb.n)
    takes_next = takes and la.n == 64 and la.act == 1 and not la.addend and lc.ldy == lc.n
    for nx in cs.forms:
        assert (takes_next if nx else takes) == cs.fusable, (name, nx)
    for l in cs.layers:
        assert l.ldw % 4 == 0 and l.ldw >= l.n and l.ldy >= l.n and l.ldy % 4 == 0 and l.ld_add % 4 == 0


def test_bottleneck_table_reaches_every_edge_the_issue_names():
    B = F.BNECKS
    assert [B["b_m_seams_%d" % m].expect["M"] for m in (29, 35, 61, 64, 65)] == [29, 35, 61, 64, 65]
    assert B["b_m_small"].expect["M"] == 15 < 32 and B["b_two_images"].shape == (3, 5, 7)
    assert B["b_h1"].shape[1] == 1 and B["b_w1"].shape[2] == 1
    assert B["b_n2_320"].layers[1].n == 320 and B["b_n2_320"].expect["M"] == 198 and B["b_n2_64"].layers[1].n == 64
    assert B["b_c32"].layers[0].c == 32 and B["b_c96"].layers[0].c == 96
    nulls = {n: cs for n, cs in B.items() if n.startswith("b_nulls_")}
    assert len(nulls) == 8
    flags = lambda cs: [(l.scale, l.shift) for l in cs.layers] + [cs.layers[1].addend]
    assert flags(B["b_nulls_all"]) == [(False, False)] * 3 + [False]
    single = [flags(cs) for n, cs in nulls.items() if n != "b_nulls_all"]
    assert len({str(f) for f in single}) == 7 and all(str(f).count("False") == 1 for f in single)
    lb, lc, la = B["b_pitch"].layers
    assert lb.ldw > 64 and len({lc.n, lc.ldw, lc.ldy, lc.ld_add}) == 4 and min(lc.ldw, lc.ldy, lc.ld_add) > lc.n and B["b_pitch"].forms == (False,)
    lb, lc, la = B["b_pitch_next"].layers
    assert la.ldy > 64 and la.ldw > 64 and la.ldy != la.ldw and lc.ldy == lc.n and B["b_pitch_next"].forms == (True,)
    assert B["b_pitched_t2"].layers[0].ldy == 72 and B["b_pitched_y_with_next"].layers[1].ldy == 128 + 8
    for key in ("t2", "y", "t"):
        pre = F.chain("b_relu_exact", True).pre[key][:-1]
        assert 0.4 < (pre < 0).mean() < 0.6, (key, (pre < 0).mean())
        assert (F.chain("b_relu_exact", True).val[key][:-1][pre < 0] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the references
def _oracle_layer(shape, l, x, p):
    nb, h, w = shape
    oh, ow, M, K = F.grid(shape, l)
    w4 = p["w"].astype(np.float64).reshape(l.k, l.k, l.c, l.n)
    y = dense.conv2d(x.reshape(nb, h, w, l.c), w4, None, l.stride, (l.pad,) * 4).reshape(M, l.n)
    pre = y * (p["scale"].astype(np.float64) if l.scale else 1.0) + (p["shift"].astype(np.float64) if l.shift else 0.0)
    pre = pre + (p["addend"].astype(np.float64) if l.addend else 0.0)
    out = np.maximum(pre, 0) if l.act == 1 else pre.copy()
    if l.act == 2:
        out[:, :l.act_cols] = 1.0 / (1.0 + np.exp(-pre[:, :l.act_cols]))
    return out


def _same(a, b):
    return a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-12 * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("name", list(F.PAIRS))
def test_pair_reference_equals_the_oracle(name):
    cs, d, b = F.PAIRS[name], F.pair_inputs(name), F.pair(name)
    for i in range(2):
        key, c0, ld = F.pair_slot(cs, i)
        l = cs.layers[i]
        want = _oracle_layer(cs.shapes[i], l, d["x%d" % (i + 1)].astype(np.float64), d["p%d" % (i + 1)])
        assert _same(b.val[key][:-1, c0:c0 + l.n], want), (name, i)
        outside = np.ones(b.val[key].shape, bool)
        for j in range(2):
            kj, cj, _ = F.pair_slot(cs, j)
            if kj == key:
                outside[:-1, cj:cj + cs.layers[j].n] = False
        assert np.isnan(b.val[key][outside]).all() and np.isnan(b.tol[key][outside]).all() and (b.tol[key][~outside] > 0).all()


@pytest.mark.parametrize("name", [n for n in F.BNECKS if n not in F.PITCHED_INTERMEDIATE])
def test_chain_reference_equals_the_oracle_composed_layer_by_layer(name):
    cs, d = F.BNECKS[name], F.bneck_inputs(name)
    M = cs.shape[0] * cs.shape[1] * cs.shape[2]
    lb, lc, la = cs.layers
    t2 = _oracle_layer(cs.shape, lb, d["x"].astype(np.float64), d["pb"])
    y = _oracle_layer((1, 1, M), lc, t2 if cs.linked else d["x2"].astype(np.float64), d["pc"])
    t = _oracle_layer((1, 1, M), la, y, d["pa"])
    for nx in cs.forms:
        b = F.chain(name, nx)
        assert sorted(b.val) == sorted(["t2", "y"] + (["t"] if nx else []))
        for key, l, want in (("t2", lb, t2), ("y", lc, y), ("t", la, t))[:3 if nx else 2]:
            assert b.val[key].shape == (M + 1, l.ldy)
            assert _same(b.val[key][:-1, :l.n], want), (name, key)
            assert np.isnan(b.val[key][-1]).all() and np.isnan(b.val[key][:, l.n:]).all() and (b.tol[key][:-1, :l.n] > 0).all()


def test_pitched_intermediates_are_read_as_dense_by_the_next_layer():
    """The separate launches, which the header promises: a db->y of pitch 72 is read by dc as [M][64] -- rows shifted, padding read."""
    b = F.chain("b_pitched_t2", False)
    d, cs = F.bneck_inputs("b_pitched_t2"), F.BNECKS["b_pitched_t2"]
    assert b.val["t2"].shape == (66, 72) and np.isfinite(b.val["t2"][:-1, :64]).all() and np.isnan(b.val["t2"][:, 64:]).all()
    want_row0 = _oracle_layer((1, 1, 1), cs.layers[1], b.val["t2"][0:1, :64].copy(), dict(d["pc"], addend=d["pc"]["addend"][:1]))
    assert _same(b.val["y"][0:1, :128], want_row0)                       # row 0 starts at the same address under both readings
    assert np.isnan(b.val["y"][1:9, :128]).all()                         # the next rows take in padding ...
    assert np.isfinite(b.val["y"][9, :128]).all()                        # ... until 9 * 64 = 8 * 72: row 9 is computed from row 8 of t2
    assert np.isnan(b.val["y"][:-1, :128]).any(axis=1).sum() == 65 - 8   # rows 0, 9, 18, ..., 63 alone read no padding
    b = F.chain("b_pitched_y_with_next", True)
    assert np.isfinite(b.val["y"][:-1, :128]).all() and np.isnan(b.val["t"][1:17, :64]).all() and np.isfinite(b.val["t"][17, :64]).all()


def test_gather_is_the_shared_im2col():
    for name in ("p_3x3_two_images", "p_s2_1x1", "p_stem"):
        cs = F.PAIRS[name]
        l, (nb, h, w) = cs.layers[0], cs.shapes[0]
        oh, ow, M, K = F.grid(cs.shapes[0], l)
        x = F.pair_inputs(name)["x1"].reshape(nb, h, w, l.c)
        c32 = F32.Case(name, "fwd", nb, h, w, l.c, l.k, l.k, l.stride, (l.pad,) * 4, l.n, (), {}, {})
        assert (oh, ow) == ((h + 2 * l.pad - l.k) // l.stride + 1, (w + 2 * l.pad - l.k) // l.stride + 1)
        assert np.array_equal(F.gather(x, nb, h, w, oh, ow, l.k, l.k, l.stride, l.pad, l.pad).reshape(M, K), F.im2col(x, c32))


@pytest.mark.parametrize("name", PAIR_RUN + ["p_diff_m"])
def test_a_launch_emulated_tile_by_tile_fills_the_same_buffers(name):
    ref = F.pair(name)
    for bm, bn in F.TILES:
        got = F.pair_by_tiles(name, bm, bn)
        for key in ref.val:
            assert np.array_equal(got.val[key], ref.val[key], equal_nan=True), (name, bm, bn, key)
        units = F.pair_units(F.PAIRS[name], bm, bn)
        assert len(set(units)) == len(units)                            # no tile twice


def test_bounds_are_the_stated_formulas():
    u = 2.0 ** -24
    name = "b_n2_320"
    cs, d, b = F.BNECKS[name], F.bneck_inputs(name), F.chain(name, True)
    lb, lc, la = cs.layers
    f = lambda a: np.abs(np.asarray(a, np.float64))
    A1 = f(F.gather(d["x"].reshape(2, 9, 11, 64), 2, 9, 11, 9, 11, 3, 3, 1, 1, 1).reshape(198, 576)) @ f(d["pb"]["w"])
    E1 = (9 * 64 + 8) * u * (A1 * f(d["pb"]["scale"]) + f(d["pb"]["shift"]))
    t2, y = b.val["t2"][:-1], b.val["y"][:-1]
    A2 = (f(t2) + E1) @ f(d["pc"]["w"])
    E2 = (64 + 8) * u * (A2 * f(d["pc"]["scale"]) + f(d["pc"]["shift"]) + f(d["pc"]["addend"])) + (E1 @ f(d["pc"]["w"])) * f(d["pc"]["scale"])
    A3 = (f(y) + E2) @ f(d["pa"]["w"])
    E3 = (320 + 8) * u * (A3 * f(d["pa"]["scale"]) + f(d["pa"]["shift"])) + (E2 @ f(d["pa"]["w"])) * f(d["pa"]["scale"])
    for key, E in (("t2", E1), ("y", E2), ("t", E3)):
        assert np.allclose(b.tol[key][:-1], E, rtol=1e-13, atol=0), key
    # the pair: the fp32 suite's single-layer bound, sigmoid columns a quarter of it plus the slack
    name = "p_3x3_two_images"
    cs, d, b = F.PAIRS[name], F.pair_inputs(name), F.pair(name)
    A = f(F.gather(d["x1"].reshape(2, 9, 11, 32), 2, 9, 11, 9, 11, 3, 3, 1, 1, 1).reshape(198, 288))
    p1, p2 = d["p1"], d["p2"]
    assert np.allclose(b.tol["y1"][:-1], (288 + 8) * u * ((A @ f(p1["w"])) * f(p1["scale"]) + f(p1["shift"]) + f(p1["addend"])), rtol=1e-13, atol=0)
    base = (288 + 8) * u * (A @ f(p2["w"]) + f(p2["shift"]))
    assert np.allclose(b.tol["y2"][:-1, 20:], base[:, 20:], rtol=1e-13, atol=0)
    assert np.allclose(b.tol["y2"][:-1, :20], 0.25 * base[:, :20] + F.SIGMOID_SLACK, rtol=1e-13, atol=0)
    assert ((b.val["y2"][:-1, :20] > 0) & (b.val["y2"][:-1, :20] < 1)).all() and (b.val["y2"][:-1, 20:] < 0).any()


# ---------------------------------------------------------------------------------------------------------------- emulations
@pytest.mark.parametrize("order", ["blas", "chain"])
@pytest.mark.parametrize("name", list(F.PAIRS))
def test_fp32_emulation_of_a_pair_is_inside_the_bound(name, order):
    worst, bad, spilled = _cpu_verdict(F.emulate_pair(name, order), F.pair(name))
    print("%s/%s: worst err / tol %.4f" % (name, order, worst))
    assert bad == 0 and spilled == 0 and worst <= 1.0
    if F.PAIRS[name].exact:
        assert worst == 0.0


@pytest.mark.parametrize("order", ["blas", "chain"])
@pytest.mark.parametrize("name,with_next", EMULATED)
def test_fp32_emulation_of_a_chain_is_inside_the_bound(name, with_next, order):
    worst, bad, spilled = _cpu_verdict(F.emulate_chain(name, with_next, order), F.chain(name, with_next))
    print("%s/%s/%s: worst err / tol %.4f" % (name, with_next, order, worst))
    assert bad == 0 and spilled == 0 and worst <= 1.0
    if F.BNECKS[name].exact:
        assert worst == 0.0


def test_integer_cases_are_exact_in_fp32_by_their_magnitudes():
    """Inputs, weights, shifts and addends are integers, every scale 2^-3: layer i's products are multiples of unit_i = 8^-i, and
    sum|a b| / unit_i as well as the finished pre-activation / (unit_i / 8) stay below 2^24 -- no partial sum in any order rounds."""
    f = lambda a: np.abs(np.asarray(a, np.float64))
    cs, d, b = F.BNECKS["b_exact"], F.bneck_inputs("b_exact"), F.chain("b_exact", True)
    x, unit = f(d["x"]), 1.0
    for key, pk, l in zip(F.BNECK_KEYS, ("pb", "pc", "pa"), cs.layers):
        p = d[pk]
        assert (p["scale"] == 0.125).all() and (p["w"] == np.rint(p["w"])).all() and (x / unit == np.rint(x / unit)).all()
        A = f(F.gather(x.reshape(cs.shape + (l.c,)), cs.shape[0], cs.shape[1], cs.shape[2], cs.shape[1], cs.shape[2], 3, 3, 1, 1, 1)) if l.k == 3 else x
        absdot = A.reshape(x.shape[0], -1) @ f(p["w"])
        assert absdot.max() / unit < 2 ** 24, (key, absdot.max() / unit)
        total = absdot * 0.125 + f(p["shift"]) + (f(p["addend"]) if l.addend else 0.0)
        unit /= 8
        assert total.max() / unit < 2 ** 24, (key, total.max() / unit)
        x = f(b.val[key][:-1])
        assert (b.val[key][:-1] > 0).any() and (b.pre[key][:-1] < 0).any()
    cs, d = F.PAIRS["p_exact"], F.pair_inputs("p_exact")
    for i, l in enumerate(cs.layers):
        p, (nb, h, w) = d["p%d" % (i + 1)], cs.shapes[i]
        A = f(F.gather(d["x1"].reshape(nb, h, w, l.c), nb, h, w, h, w, 3, 3, 1, 1, 1)).reshape(nb * h * w, -1)
        total = (A @ f(p["w"])) * 0.125 + f(p["shift"]) + (f(p["addend"]) if l.addend else 0.0)
        assert (p["scale"] == 0.125).all() and (A @ f(p["w"])).max() < 2 ** 24 and total.max() * 8 < 2 ** 24


# ---------------------------------------------------------------------------------------------------------------- teeth
def _factor(got, ref):
    worst, bad, spilled = _cpu_verdict(got, ref)
    return float("inf") if spilled else worst


@pytest.mark.parametrize("mut", list(F.PAIR_MUTANTS))
def test_pair_mutants_are_caught(mut):
    for name in F.PAIR_MUTANTS[mut]:
        tiles = F.TILES if mut in ("second_with_n1", "gx1_for_second") else ((64, 64),)
        for tile in tiles:
            fac = _factor(F.pair_mutant(name, mut, tile), F.pair(name))
            print("pair %s on %s %s: factor %.3g" % (mut, name, tile, fac))
            assert fac >= 4.0, (mut, name, tile, fac)


def test_second_with_n1_is_silent_where_the_second_problem_is_the_narrower_one():
    """Why p_n_order runs in both orders: extra column tiles fall off the descriptor, missing ones leave a hole."""
    cs = F.PAIRS["p_n_order_swapped"]
    got = F._pair_buffers("p_n_order_swapped", F._pair_outputs("p_n_order_swapped"), units=((64, 64), F.pair_units(cs, 64, 64, "second_with_n1")))
    assert _factor(got, F.pair("p_n_order_swapped")) == 0.0


@pytest.mark.parametrize("mut", list(F.BNECK_MUTANTS))
def test_bottleneck_mutants_are_caught(mut):
    for name, with_next in F.BNECK_MUTANTS[mut][1]:
        fac = _factor(F.chain_mutant(name, with_next, mut), F.chain(name, with_next))
        print("bneck %s on %s%s: factor %.3g" % (mut, name, " + next" if with_next else "", fac))
        assert fac >= 4.0, (mut, name, with_next, fac)


def test_every_mutant_the_issue_lists_exists():
    assert set(F.PAIR_MUTANTS) >= {"add_with_ldy", "y_with_ld_add", "wrap_taps", "second_with_n1", "gx1_for_second"}
    assert set(F.BNECK_MUTANTS) >= {"add_with_ldy", "y_with_ld_add", "shift_prev_chunk", "w3_no_chunk_offset", "no_relu", "wrap_taps", "store_row_m"}


def test_table_lines_have_the_keys_the_launchers_look_up():
    cs = F.PAIRS["p_s2_1x1"]
    assert F.pair_line(cs, 32, 64, 1) == "32 147 %d 64 64 1 2 32 64 1 0.01 4" % (40 * 65536 + 100)
    assert F.single_line(cs.shapes[0], cs.layers[1]) == "0 147 100 64 64 1 2 64 64 1 0.01 4"
    cs = F.BNECKS["b_n2_320"]
    assert F.bneck_line(cs, True, 32, 1) == "33 198 %d 576 64 9 1 32 64 1 0.01 4" % (320 * 65536 + 64)
    assert F.bneck_line(cs, False, 64, 2) == "33 198 %d 576 64 9 1 64 64 2 0.01 4" % (320 * 65536)
    assert F.single_line(cs.shape, cs.layers[0]) == "0 198 64 576 64 9 1 64 64 1 0.01 4"
    assert F.single_line((1, 1, 198), cs.layers[2]) == "0 198 64 320 320 1 1 64 64 1 0.01 4"
