"""Device-free check of tests/wgrad_multi_cases.py: every table reaches what it claims under the model of the launch policy and of
wgrad_multi_plan, the arenas are laid out as stated, the references agree with an explicit loop, honest fp32 Adam stays inside the bounds,
every tail layout lies inside radnet_adam_step_tail's contract and every refusal outside it for the reason it names, and every named mutant
of the references misses its bound by more than 4x on the case named for it."""
import numpy as np
import pytest

import fp32_edge_cases as P
import update_edge_cases as E
import wgrad_multi_cases as M

F = M.F


def _shapes(t, ordered=True):
    return [M.launch_shape(e, t.ws, ordered) for e in t.entries]


def _miss(res, mutated):
    """By how much the worst element of a mutated full buffer misses the verdict of `res`: err / tol, inf where no error is allowed."""
    m = np.asarray(mutated, np.float64).ravel()
    k = m.size
    ins = res["inside"][:k]
    old = res["prefill"][:k].view(F).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(ins, np.abs(m - res["ref"][:k]), np.where((m == old) | (np.isnan(m) & np.isnan(old)), 0.0, np.inf))
        ratio = np.where(err > 0, err / np.where(ins, res["tol"][:k], 0.0), 0.0)
    return float(np.nan_to_num(ratio, nan=np.inf).max())


def _miss_grad(ref, mutated, key="out", tol="tol"):
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(np.asarray(mutated[key], np.float64) - ref[key])
        ratio = np.where(err > 0, err / ref[tol], 0.0)
    return float(np.nan_to_num(np.where(np.isnan(err), np.inf, ratio), nan=np.inf).max())


# ---------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("name", list(M.TABLES))
def test_every_table_reaches_what_it_claims(name):
    t = M.TABLES[name]
    launches, split = M.CLAIMS[name]
    shapes = _shapes(t)
    lz = M.plan(t.entries, t.ws)
    assert len(lz) == launches
    assert {i: s["slices"] for i, s in enumerate(shapes) if s["slices"] > 1} == split
    assert sorted(i for l in lz for i in l["problems"]) == list(range(len(t.entries))), "a problem is left unjudged"
    assert M.unpinned_hits_a_pin(t.entries) == [] and len(M.pin_lines(t.entries)) == len({(e.case, e.cols, e.mode == 1) for e in t.entries if e.pin})
    for e, s in zip(t.entries, shapes):
        d = M.dims(e)
        assert d["c"] % s["bmk"] == 0, "no problem is skipped because a tile does not divide c: the count the GPU test asserts is 0"
        assert d["c"] % 64 == 0 and d["N"] % 4 == 0 and d["ld_dy"] % 4 == 0 and d["ldw"] % 4 == 0 and d["ldw"] > d["N"]
        assert s["slices"] == 1 or d["nmt"] // s["slices"] >= 1
    for l in lz:
        assert len(l["problems"]) <= M.K_MULTI_MAX and all(off % 256 == 0 for off in l["slab_off"])
        ends = [off + shapes[i]["slab_bytes"] for off, i in zip(l["slab_off"], l["problems"])]
        assert all(a <= b for a, b in zip(ends, l["slab_off"][1:])) and (not ends or max(ends) <= max(t.ws, 0)), "slabs of one launch overlap"
    # with atomics nothing needs slabs, and the fallback does not run
    assert all(s["slab_bytes"] == 0 and s["counters"] == 0 for s in _shapes(t, ordered=False))


def test_the_tables_cover_the_named_paths():
    T = M.TABLES
    assert {e.case for e in T["all_default"].entries} == set(M.PROBLEMS) == {e.case for e in T["pinned_mixed"].entries}
    assert all(e.pin is None for e in T["all_default"].entries) and all(e.pin for e in T["pinned_mixed"].entries)
    # all_default: at least three launches and a split problem; a tile shape other than 64x64 never stands beside itself
    sh = [(s["bmk"], s["bn"]) for s in _shapes(T["all_default"])]
    assert len(set(sh)) >= 3 and len(M.plan(T["all_default"].entries, M.WS_BIG)) >= 3 and M.CLAIMS["all_default"][1]
    assert all(a != b or a == (64, 64) for a, b in zip(sh, sh[1:])) and max(sh.count(s) for s in set(sh) if s != (64, 64)) == 2
    # pinned_mixed: all four tile shapes; slices 1, 2, 3, 8 side by side in the 64x64 launch; w_deep_m's offsets are no multiples of its own sizes
    sp = _shapes(T["pinned_mixed"])
    assert {(s["bmk"], s["bn"]) for s in sp} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    l64 = next(l for l in M.plan(T["pinned_mixed"].entries, M.WS_BIG) if (l["bmk"], l["bn"]) == (64, 64))
    assert [sp[i]["slices"] for i in l64["problems"]] == [1, 2, 3, 8, 1, 2]
    k = l64["problems"].index(6)
    assert T["pinned_mixed"].entries[6].case == "w_deep_m" and l64["slab_off"][k] % sp[6]["slab_bytes"] != 0 and l64["slab_off"][k] > 0
    assert l64["counter_off"][k] == 10 and l64["counter_off"][k + 2] == 11 and l64["first"][k] == 1 + 2 + 27
    # seventeen: one tile shape, the seventeenth problem opens a launch that starts again at slab offset 0 and counter 0
    l17 = M.plan(T["seventeen"].entries, M.WS_BIG)
    assert [len(l["problems"]) for l in l17] == [16, 1] and l17[1]["problems"] == [16] and l17[1]["slab_off"] == [0] and l17[1]["counter_off"] == [0]
    assert l17[0]["slab_off"][1] > 0 and len({e.case for e in T["seventeen"].entries}) == 4
    # tight_two: any one problem's slabs fit, two do not
    s2 = _shapes(T["tight_two"])
    assert max(s["slab_bytes"] for s in s2) <= T["tight_two"].ws < s2[0]["slab_bytes"] + s2[1]["slab_bytes"]
    assert [l["problems"] for l in M.plan(T["tight_two"].entries, T["tight_two"].ws)] == [[0], [1, 2]]
    # tight_halving: 8 slices do not fit, 4 do
    e = T["tight_halving"].entries[0]
    assert M.default_shape(64, 64, 8, 34) == (64, 64, 8) and M.slab_bytes(64, 8, 64, 64, 8) > T["tight_halving"].ws >= M.slab_bytes(64, 8, 64, 64, 4) and e.case == "w_deep_m"
    # no_workspace: every ordered reduction falls back to one slice; with atomics the choices stay
    assert all(s["slices"] == 1 for s in _shapes(T["no_workspace"])) and [s["slices"] for s in _shapes(T["no_workspace"], False)] == [8, 3, 1]
    # shared_x: one geometry, another dy pointer and n
    a, b = T["shared_x"].entries
    assert a.case == b.case and M.dims(b)["c0"] == 16 and M.dims(b)["N"] == 20 != M.dims(a)["N"]
    assert T["zero_live"].entries[0].zero and not any(e.zero for e in T["zero_live"].entries[1:]) and not M.problem_inputs(T["zero_live"].entries[0])["dy"][:, :32].any()
    assert {e.mode for e in T["modes"].entries} == {0, 1, 2} and {e.db for e in T["modes"].entries} == {True, False}
    assert any(l.startswith("3 ") for l in M.pin_lines(T["modes"].entries)) and any(l.startswith("2 ") for l in M.pin_lines(T["modes"].entries))
    assert set(M.OPT_TABLES) == set(T) - {"modes"}
    # the problems span what the issue names
    ms = {P.geometry(P.CASES[n], "wgrad")["M"] for n in M.PROBLEMS}
    assert min(ms) == 1 and max(ms) == 1085 and {P.CASES[n].n for n in M.PROBLEMS} >= {4, 36, 68, 72} and {P.CASES[n].c for n in M.PROBLEMS} == {64, 128}


@pytest.mark.parametrize("name", M.OPT_TABLES)
def test_the_optimizer_arenas_are_laid_out_as_stated(name):
    ar, t = M.arena_of(name), M.TABLES[name]
    assert all(off % 4 == 0 for off in ar.offs) and ar.n % 4 == 0
    ends = [off + M.dims(e)["K"] * M.dims(e)["ldw"] for off, e in zip(ar.offs, t.entries)]
    assert [off - end for off, end in zip(ar.offs, [0] + ends)] == [M.GAPS[i % 3] for i in range(len(t.entries))]
    assert ar.bias == (ends[-1], M.OPT_BIAS_LEN) and ar.dense[0] + ar.dense[1] == ar.n
    idx, pad = M.layer_index(name), M.pad_index(name)
    assert len(set(idx.tolist())) == idx.size == sum(M.dims(e)["K"] * M.dims(e)["N"] for e in t.entries)
    assert not set(idx.tolist()) & set(pad.tolist()) and max(idx.max(), pad.max()) < ends[-1] and pad.size == 4 * sum(M.dims(e)["K"] for e in t.entries)
    if len(t.entries) >= 3:
        assert set(np.asarray(M.GAPS)) <= {off - end for off, end in zip(ar.offs, [0] + ends)}
    # the inputs of the first step are nowhere borderline, and honest fp32 Adam stays inside the bounds (unfused and either product fused)
    grads = M.reference_grads(name)
    for which in M.OPT_STATES:
        st = M.opt_state(name, which)
        assert len(M.OPT_STEPS[which]) == 2 and set(M.OPT_STEPS["random"] + M.OPT_STEPS["zero_moments"]) == set(E.STEPS_FOUR)
        t_, gs = M.OPT_STEPS[which][0]
        g = M.grads_flat(name, grads)
        assert E.borderline_adam(st["p"][idx], g, st["m"][idx], st["v"][idx], t_, gs) == 0
        refs = M.epilogue_refs(name, st, grads, t_, gs)
        for fuse in (None, "first", "second"):
            emu = dict(zip("pmv", E.adam_emulate(st["p"][idx], g, st["m"][idx], st["v"][idx], t_, gs, fuse)))
            for k in "pmv":
                got = st[k].copy()
                got[idx] = emu[k]
                bad, worst = M.verdict(refs[k], got)
                assert bad == 0 and worst <= 1.0, (name, which, k, fuse, bad, worst)


# ---------------------------------------------------------------------------------------------------------------- references
def test_the_references_agree_with_an_explicit_loop_on_the_two_smallest_problems():
    work = sorted(M.PROBLEMS, key=lambda n: P.geometry(P.CASES[n], "wgrad")["M"] * P.geometry(P.CASES[n], "wgrad")["K"] * P.CASES[n].n)
    assert work[:2] == ["w_m1", "w_3x1_s2"]
    for e in (M.entry("w_m1", mode=1), M.entry("w_3x1_s2", mode=0), M.entry("w_m1", cols=(0, 4), mode=2)):
        dw, db = M.loop_ref(e)
        r = M.problem_ref(e)
        assert np.abs(dw - r["out"]).max() <= 1e-12 * max(1.0, np.abs(r["out"]).max()) and np.abs(db - r["db"]).max() <= 1e-12 * max(1.0, np.abs(r["db"]).max())
        assert (r["tol"] >= 0).all() and r["out"].shape == (M.dims(e)["K"], M.dims(e)["N"])
    # a column block is the same columns of its case; a problem without live rows is exactly zero with no slack
    a, b = M.TABLES["shared_x"].entries
    assert np.array_equal(M.problem_ref(b)["out"], M.problem_ref(a._replace(mode=2))["out"][:, 16:36])
    z = M.problem_ref(M.TABLES["zero_live"].entries[0])
    assert not z["out"].any() and not z["tol"].any() and not z["db"].any() and not z["db_tol"].any()
    # Adam of one element from the definition
    name = "one"
    st, grads = M.opt_state(name, "random"), M.reference_grads(name)
    t_, gs = M.OPT_STEPS["random"][0]
    refs = M.epilogue_refs(name, st, grads, t_, gs)
    i = int(M.layer_index(name)[5])
    g = float(grads[0].reshape(-1)[5]) * float(gs)
    m2 = float(E.B1) * float(st["m"][i]) + (1.0 - float(E.B1)) * g
    v2 = float(E.B2) * float(st["v"][i]) + (1.0 - float(E.B2)) * g * g
    p2 = float(st["p"][i]) - float(E.lr_t(t_)) * m2 / (np.sqrt(v2) + float(E.EPS))
    assert abs(refs["m"]["ref"][i] - m2) <= 1e-15 and abs(refs["v"]["ref"][i] - v2) <= 1e-15 and abs(refs["p"]["ref"][i] - p2) <= 1e-14
    assert refs["p"]["inside"][i] and not refs["p"]["inside"][i - 5 - 1 + M.dims(M.TABLES[name].entries[0])["ldw"]]


# ---------------------------------------------------------------------------------------------------------------- tails
@pytest.mark.parametrize("name", list(M.TAILS))
def test_every_tail_layout_lies_inside_the_contract(name):
    lay = M.TAILS[name]
    assert M.tail_violations(lay) == []
    ranges = M.tail_ranges(lay)
    gap0, pref = E.gap_table(lay.n, ranges)
    assert 4 * pref[-1] == lay.n - lay.sweep_from and len(ranges) <= M.GAP_RANGES_MAX and sum(ln for _, ln in ranges) == lay.sweep_from
    for j in (0, pref[-1] - 1) if pref[-1] else ():
        assert 4 * E.sweep_chunk(gap0, pref, j)[0] >= lay.sweep_from, "the sweep reaches in front of sweep_from"
    if lay.bias:
        assert lay.sweep_from <= lay.bias[0] and lay.bias[0] + lay.bias[1] <= lay.n
    st = M.tail_state(name)
    for t_, gs in lay.steps[:1]:
        sw = slice(lay.sweep_from, lay.n)
        assert E.borderline_adam(st["p"][sw], st["g"][sw], st["m"][sw], st["v"][sw], t_, gs) == 0


def test_the_tail_layouts_cover_the_named_paths():
    T = M.TAILS
    assert {len(l.wino) for l in T.values()} == {1, 3, 7}
    ends_at = lambda l: max(off + 9 * c * n for off, c, n in l.wino) == l.sweep_from
    adjacent = lambda l: any(a[0] + 9 * a[1] * a[2] == b[0] for a, b in zip(sorted(l.wino), sorted(l.wino)[1:]))
    for k in (3, 7):
        assert {adjacent(l) for l in T.values() if len(l.wino) == k} == {True, False}
    assert ends_at(T["three_adjacent_to_sweep"]) and ends_at(T["seven_adjacent"]) and not ends_at(T["seven_gaps"])
    assert len(M.tail_ranges(T["seven_gaps"])) == 15 and len(M.tail_ranges(T["seven_adjacent"])) == 7
    where = lambda l: "start" if l.bias[0] == l.sweep_from else "end" if l.bias[0] + l.bias[1] == l.n else "middle"
    assert {where(l) for l in T.values() if l.bias} == {"start", "middle", "end"}
    assert T["sweep_at_n"].sweep_from == T["sweep_at_n"].n and T["sweep_at_n"].bias is None
    oc = T["over_cap"]
    assert (oc.n - oc.sweep_from) // 4 == E.SWEEP_CAP + 192 and oc.steps == E.STEPS_ONE and (oc.bias[0] - oc.sweep_from) // 4 >= E.SWEEP_CAP
    assert oc.n // 4 - E.SWEEP_CAP < 1000, "the largest arena: 2,097,152 + a few hundred float4"


@pytest.mark.parametrize("name", list(M.TAIL_REFUSALS))
def test_every_tail_refusal_breaks_exactly_the_rule_it_names(name):
    lay, fragment = M.TAIL_REFUSALS[name]
    bad = M.tail_violations(lay)
    words = {"eight_layers_nine_gaps": "too many layers", "sweep_from_0": "positive", "sweep_from_not_multiple_of_4": "multiple of 4",
             "sweep_from_past_n": "inside the arena", "layer_past_sweep_from": "reaches past", "bias_in_front_of_sweep_from": "bias range in front"}
    assert bad and words[name] in bad[0], (name, bad)
    assert fragment
    if name == "eight_layers_nine_gaps":
        assert len(lay.wino) == 8 and len(M.tail_ranges(lay)) == 17
        assert M.tail_violations(lay._replace(sweep_from=lay.wino[-1][0] + M._UNIT, bias=None)) == [], "eight layers that end at sweep_from fit"


# ---------------------------------------------------------------------------------------------------------------- teeth
def test_every_mutant_misses_its_bound_by_more_than_4x_on_the_case_named_for_it():
    seen = set()
    # gradients
    for mut, name, k, key, tol in (("neighbour_dy", "shared_x", 1, "out", "tol"), ("neighbour_dy", "shared_x", 1, "db", "db_tol"),
                                   ("db_added_in_mode0", "all_default", 1, "db", "db_tol"), ("seventeenth_dropped", "seventeen", 16, "out", "tol"),
                                   ("seventeenth_dropped", "seventeen", 16, "db", "db_tol")):
        ref, got = M.table_refs(M.TABLES[name])[k], M.table_refs(M.TABLES[name], mut)[k]
        assert _miss_grad(ref, got, key, tol) > 4, (mut, name, key)
        seen.add(mut)
    same = M.table_refs(M.TABLES["seventeen"], "seventeenth_dropped")
    assert all(_miss_grad(r, g) == 0 for r, g in zip(M.table_refs(M.TABLES["seventeen"])[:16], same[:16]))
    # the epilogue
    for mut, name in (("dense_pitch", "pinned_mixed"), ("pad_stepped", "all_default")):
        st, grads = M.opt_state(name, "random"), M.reference_grads(name)
        refs = M.epilogue_refs(name, st, grads, *M.OPT_STEPS["random"][0], mut=mut)
        for k in "pmv":
            assert _miss(refs[k], refs[k]["mutant"]) > 4, (mut, name, k)
        seen.add(mut)
    # the tail
    for mut, name in (("tail_sweeps_from_0", "three_gaps"), ("front_gap_swept", "one_layer_gaps"), ("tail_steps_a_layer", "three_adjacent_to_sweep")):
        lay, st = M.TAILS[name], M.tail_state(name)
        refs = M.tail_refs(lay, st, *lay.steps[0], zero_grad=1, mut=mut)
        for k in "pmv":
            assert _miss(refs[k], refs[k]["mutant"]) > 4, (mut, name, k)
        seen.add(mut)
    # what is derived from the weights: U of a listed layer from the weights before the epilogue's step, the shift from the weights before the sweep's
    lay, st = M.TAILS["three_mixed"], M.tail_state("three_mixed")
    t_, gs = lay.steps[0]
    off, c, n = lay.wino[1]
    ly = slice(off, off + 9 * c * n)
    p_in = st["p"].copy()
    p_in[ly] = E.adam_emulate(st["p"][ly], st["g"][ly], st["m"][ly], st["v"][ly], t_, gs)[0]          # what the epilogue left
    good, stale = E.ref_wino(p_in, off, c, n), E.ref_wino(p_in, off, c, n, p_old=st["p"], mut="wino_from_old_p")
    k = 36 * c * n
    assert float((np.abs(stale["buf"][:k] - good["buf"][:k]) / good["tol"][:k]).max()) > 4
    seen.add("wino_from_old_p")
    sw = slice(lay.sweep_from, lay.n)
    p_new = p_in.copy()
    p_new[sw] = E.adam_emulate(st["p"][sw], st["g"][sw], st["m"][sw], st["v"][sw], t_, gs)[0]
    b = E.bias_inputs(lay.bias[1])
    good, stale = E.ref_shift(p_new, b["scale"], b["t0"], *lay.bias), E.ref_shift(p_new, b["scale"], b["t0"], *lay.bias, p_old=p_in, mut="shift_from_old_p")
    assert float((np.abs(stale["buf"][:lay.bias[1]] - good["buf"][:lay.bias[1]]) / good["tol"][:lay.bias[1]]).max()) > 4
    seen.add("shift_from_old_p")
    assert seen == set(M.MUTANTS)
