"""Device-free check of tests/update_edge_cases.py: every case lies inside the contract of its entry point, the tables reach the paths
they name, the references agree with the oracle, honest fp32 arithmetic in the kernels' association -- unfused and with either product
of every a*b + c contracted -- stays within every bound, no input is borderline, and every named mutant falls outside its bound."""
import numpy as np
import pytest

import head_edge_cases as H
import update_edge_cases as E
import winograd_edge_cases as W

F = E.F
ENTRY_PAIRS = [(name, entry) for name, lay in E.LAYOUTS.items() for entry in lay.entries]


def _state(lay):
    return E.adam_state(lay.n)


def _within(res, got, what):
    """`got` (the written part, fp32) against the full-buffer reference `res`."""
    k = got.size
    ref, tol = res["buf"][:k], res["tol"][:k]
    assert res["inside"][:k].all() and not res["inside"][k:].any(), what
    err = np.abs(got.astype(np.float64).ravel() - ref)
    bad = ~(err <= tol)
    assert not bad.any(), (what, int(bad.sum()), float((err[bad] / np.maximum(tol[bad], 1e-300)).max()))
    return float((err / np.where(tol > 0, tol, np.inf)).max())


def _outside(res, mutated):
    """True when the mutated full buffer breaks the verdict of `res`: an element outside its bound, or a must-be-zero element set."""
    m = np.asarray(mutated, np.float64).ravel()
    k = m.size
    ins = res["inside"][:k]
    with np.errstate(invalid="ignore"):
        off = ins & ~(np.abs(m - res["buf"][:k]) <= res["tol"][:k])
    return bool(off.any() or (res["zero"][:k] & (m != 0)).any())


# ---------------------------------------------------------------------------------------------------------------- contracts and paths
@pytest.mark.parametrize("name,entry", ENTRY_PAIRS)
def test_every_adam_layout_lies_inside_the_contract_of_its_entry(name, entry):
    lay = E.LAYOUTS[name]
    assert E.contract_violations(lay, entry) == []
    gap0, pref = E.gap_table(lay.n, E.layer_ranges(lay, entry))
    assert len(gap0) == len(E.layers_of(lay, entry)) + 1
    assert pref[-1] * 4 + sum(ln for _, ln in E.layer_ranges(lay, entry)) == lay.n
    for t, gs in E.steps_of(name):
        assert t >= 1 and F(gs) in E.GRAD_SCALES


def test_the_steps_cover_every_t_and_every_grad_scale():
    assert {t for t, _ in E.STEPS_ALL} >= set(E.STEPS_T) and {float(gs) for _, gs in E.STEPS_ALL} == {float(g) for g in E.GRAD_SCALES}
    assert E.lr_t(100000) == E.LR and E.lr_t(1) != E.LR
    for name in E.LAYOUTS:
        cls = E.adam_state(E.LAYOUTS[name].n)["cls"]
        assert set(cls.tolist()) == (set(range(8)) if E.LAYOUTS[name].n >= 8 else {0, 1, 2, 3})


def test_the_glue_cases_lie_inside_their_contracts():
    for m in E.COLSUM_M:
        for n in E.COLSUM_N:
            assert m >= 1 and n >= 1 and n <= 65536
    for nb, oh, ow, c, s, h, w, _ in E.scatter_cases() + [E.SCATTER_OVER]:
        assert nb >= 1 and oh >= 1 and ow >= 1 and c >= 4 and c % 4 == 0 and s >= 1 and (oh - 1) * s < h and (ow - 1) * s < w
        assert nb * h * w * (c // 4) < 2 ** 31
    assert all(n >= 0 for n in E.FLAT_N) and all(h >= 1 and w >= 1 and cpad >= 3 for h, w, cpad in E.PREPROCESS)


def test_the_tables_reach_the_paths_they_name():
    L = E.LAYOUTS
    # the ragged bf16 layers: the tile counts the kernel's grid gives them
    assert tuple(E.bf16_tiles(k, n, ldw, ldk) for _, k, n, ldw, ldk in L["ragged_bf16"].bf16) == E.RAGGED_TILES
    assert E.RAGGED[:3] == ((0, 77, 100, 100, 96), (7700, 300, 60, 64, 304), (26900, 9, 8, 8, 40))
    assert (27256, 1, 4, 4, 8) in E.RAGGED and (27264, 64, 64, 64, 64) in E.RAGGED and E.RAGGED_TILES[5] == 4 and E.RAGGED[6][2:4] == (60, 128)
    assert len(L["twelve_layers"].wino) == E.WINO_MAX and len(L["sixteen_layers"].bf16) == E.BF16_MAX
    assert all(c * n == 256 for _, c, n in L["twelve_layers"].wino)
    # the gap in which each bias range lies
    for name, gap in (("bias_in_first_gap", 0), ("bias_in_middle_gap", 1), ("bias_in_last_gap", 3), ("bias_touches_layer_end", 1)):
        for entry in L[name].entries:
            gap0, pref = E.gap_table(L[name].n, E.layer_ranges(L[name], entry))
            off, ln = L[name].bias
            assert E.gap_of_chunk(gap0, pref, off // 4) == gap and E.gap_of_chunk(gap0, pref, (off + ln) // 4 - 1) == gap, (name, entry)
    first = E.layer_ranges(L["bias_touches_layer_end"], "fused")[0]
    assert L["bias_touches_layer_end"].bias[0] == first[0] + first[1]
    # empty gaps
    g0, pf = E.gap_table(L["descending_adjacent"].n, E.layer_ranges(L["descending_adjacent"], "fused"))
    assert pf[1] == 0 and pf[2] == 0 and pf[3] > 0
    assert E.gap_table(L["whole_arena"].n, E.layer_ranges(L["whole_arena"], "fused"))[1][-1] == 0
    # only over_cap takes a second pass of the sweep, and that pass starts in one gap and ends in another, the bias range behind its start
    for name, lay in L.items():
        for entry in lay.entries:
            rest = E.gap_table(lay.n, E.layer_ranges(lay, entry))[1][-1]
            assert (rest > E.SWEEP_CAP) == (name == "over_cap"), (name, entry)
    lay = L["over_cap"]
    for entry in lay.entries:
        gap0, pref = E.gap_table(lay.n, E.layer_ranges(lay, entry))
        assert pref[-1] == E.OVER_REST4 == 2097152 + 192
        c_first, q_first = E.sweep_chunk(gap0, pref, E.SWEEP_CAP)
        c_last, q_last = E.sweep_chunk(gap0, pref, pref[-1] - 1)
        assert q_first != q_last and c_last == lay.n // 4 - 1
        assert lay.bias[0] // 4 >= c_first
        reached = {E.sweep_chunk(gap0, pref, j)[0] for j in range(E.SWEEP_CAP, pref[-1])}
        assert set(range(lay.bias[0] // 4, (lay.bias[0] + lay.bias[1]) // 4)) <= reached          # only the second pass reaches it
    # colsum: the thresholds of the ordered form
    assert E.colsum_rows_per_block(4096, True) == 128 and E.colsum_rows_per_block(4097, True) == 256 and E.colsum_rows_per_block(4097, False) == 128
    assert {128, 129} <= set(E.COLSUM_M) and E.COLSUM_ORDERED_ABOVE == 128
    # past the grid caps
    nb, oh, ow, c, s, h, w, _ = E.SCATTER_OVER
    assert E.SCATTER_CAP < nb * h * w * (c // 4) < E.SCATTER_CAP + 4096
    assert E.FLAT_CAP < E.FLAT_N[-1] < E.FLAT_CAP + 256 and any(h * w > E.FLAT_CAP for h, w, _ in E.PREPROCESS)
    # scatter: the row oh * s exists in the "one_more" cases and must be zero
    assert any(h == oh * s + 1 for _, oh, _, _, s, h, _, _ in E.scatter_cases()) and any(w == ow * s + 1 for _, _, ow, _, s, _, w, _ in E.scatter_cases())
    assert {c[4] for c in E.scatter_cases()} == {1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------- against the oracle
def test_the_adam_reference_agrees_with_the_oracle():
    from oracle import dense
    st = E.adam_state(1028)
    for t in (1, 10):
        p, g, m, v = (st[k].astype(np.float64) for k in "pgmv")
        ref = E.adam_refs(st["p"], st["g"], st["m"], st["v"], t, F(1.0))
        step = np.abs(ref["p"]["buf"][:1028] - p)
        dense.adam_step(p, g, m, v, t, float(E.LR), float(E.B1), float(E.B2), float(E.EPS))
        assert np.allclose(ref["m"]["buf"][:1028], m, rtol=1e-15, atol=0) and np.allclose(ref["v"]["buf"][:1028], v, rtol=1e-15, atol=0)
        assert (np.abs(ref["p"]["buf"][:1028] - p) <= E.U * step + 1e-15).all()          # the oracle's lr_t is not rounded to fp32
    lay = E.LAYOUTS["interior"]
    off, c, n = lay.wino[1]
    res = E.ref_wino(st_p := E.adam_state(lay.n)["p"], off, c, n)
    direct = W.stage_filter(st_p[off:off + 9 * c * n].reshape(9 * c, n), c, n, n, 4)
    assert np.array_equal(res["buf"], direct["buf"], equal_nan=True) and np.array_equal(res["tol"], direct["tol"])
    assert res["shape"] == (36, c, n)


def test_to_bf16_rounds_to_nearest_even():
    rs = np.random.RandomState(1)
    x = np.concatenate([rs.standard_normal(4096).astype(F) * F(10.0) ** rs.randint(-6, 6, 4096).astype(F),
                        np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 0.0, 3.0], F)])          # ties: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    got = (E.to_bf16(x).astype(np.uint32) << np.uint32(16)).view(F).astype(np.float64)
    lo = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F).astype(np.float64)
    ulp = np.where(x != 0, 2.0 ** (np.floor(np.log2(np.maximum(np.abs(x.astype(np.float64)), 1e-300))) - 7), 0.0)
    hi = lo + np.sign(x) * ulp
    x64 = x.astype(np.float64)
    nearest = np.where(np.abs(x64 - lo) < np.abs(hi - x64), lo, hi)
    tie = np.abs(x64 - lo) == np.abs(hi - x64)
    even = np.where(((lo.astype(F).view(np.uint32) >> np.uint32(16)) & np.uint32(1)) == 0, lo, hi)
    assert np.array_equal(got, np.where(tie, even, nearest))
    assert got[-6] == 1.0 and got[-5] == 1.0 and got[-4] == 1.015625 and got[-3] == -1.0


# ---------------------------------------------------------------------------------------------------------------- honest fp32, borderline
@pytest.mark.parametrize("name", list(E.LAYOUTS))
def test_honest_fp32_adam_stays_within_every_bound_and_nothing_is_borderline(name):
    lay, st = E.LAYOUTS[name], _state(E.LAYOUTS[name])
    worst = dict(p=0.0, m=0.0, v=0.0, shift=0.0, u=0.0)
    for t, gs in E.steps_of(name):
        assert E.borderline_adam(st["p"], st["g"], st["m"], st["v"], t, gs) == 0
        refs = E.layout_refs(name, t, gs)
        for fuse in (None, "first", "second") if name != "over_cap" else (None,):
            p2, m2, v2 = E.adam_emulate(st["p"], st["g"], st["m"], st["v"], t, gs, fuse)
            for k, x in (("p", p2), ("m", m2), ("v", v2)):
                worst[k] = max(worst[k], _within(refs[k], x, (name, t, fuse, k)))
            assert np.array_equal(p2[st["cls"] == 0].view(np.uint32), st["p"][st["cls"] == 0].view(np.uint32))
            if lay.bias:
                b = E.bias_inputs(lay.bias[1])
                res = E.ref_shift(p2, b["scale"], b["t0"], *lay.bias)
                for f in (False, True):
                    worst["shift"] = max(worst["shift"], _within(res, E.shift_emulate(p2, b["scale"], b["t0"], *lay.bias, fuse=f), (name, "shift", f)))
            for off, c, n in lay.wino:
                worst["u"] = max(worst["u"], _within(E.ref_wino(p2, off, c, n), E.wino_emulate(p2, off, c, n).astype(F), (name, "u", off)))
            for off, k, n, ldw, ldk in lay.bf16:
                img = E.ref_bf16_image(p2, off, k, n, ldw, ldk)[:n * ldk].reshape(n, ldk)
                assert not img[:, k:].any() and np.array_equal(img[:, :k].T, E.to_bf16(p2[off:off + k * ldw].reshape(k, ldw)[:, :n]))
    for zg in (0, 1):
        g = E.ref_g(st["g"], zg)
        assert g["inside"][:lay.n].all() and not g["tol"].any() and g["zero"][:lay.n].all() == bool(zg)
    print("%s: honest fp32 worst err / tol %s" % (name, {k: round(v, 4) for k, v in worst.items()}))
    assert worst["p"] < 1 and worst["m"] < 1 and worst["v"] < 1


@pytest.mark.parametrize("m", E.COLSUM_M)
def test_honest_fp32_colsum_stays_within_its_bound(m):
    worst = 0.0
    for n in E.COLSUM_N:
        d = E.colsum_inputs(m, n, n + 3)
        assert (d["g"][:, n:] == E.PAD).all()
        for ordered in (True, False):
            rows = E.colsum_rows_per_block(m, ordered)
            for with_gs, acc in E.COLSUM_MODES:
                gs, old = d["gscale"] if with_gs else None, d["old"] if acc else None
                worst = max(worst, _within(E.ref_colsum(d["g"], n, gs, old, rows), E.colsum_emulate(d["g"], n, gs, old, rows, ordered), (m, n, ordered)))
    print("colsum m=%d: honest fp32 worst err / tol %.3f" % (m, worst))


def test_honest_fp32_affine_and_the_bit_exact_references():
    for n in E.FLAT_N[:4]:
        d = E.flat_inputs(n)
        res = E.ref_affine(d["a"], d["b"], d["c"])
        _within(res, d["a"] * d["b"] + d["c"], ("affine", n))
        _within(res, E._fma(d["a"], d["b"], d["c"]), ("affine fused", n))
        acts = d["act"]
        if n >= 255:
            assert np.isnan(acts).any() and (acts == 0).any() and np.signbit(acts[acts == 0]).any() and (acts > 0).any() and (acts < 0).any()
        for res in (E.ref_relu_mask(d["x"], acts), E.ref_scale(d["x"], E.ALPHAS[2])):
            assert not res["tol"].any() and np.array_equal(res["buf"][:n], res["buf"][:n].astype(F).astype(np.float64))
        assert _borderline_act(acts) == 0
    for case in E.scatter_cases():
        d = E.scatter_inputs(case)
        res = E.ref_scatter(d["src"], case[4], case[5], case[6], d["mask"])
        assert not res["tol"].any() and res["inside"][:-E.TAIL].all() and not res["buf"][:-E.TAIL][res["zero"][:-E.TAIL]].any()
        if d["mask"] is None:
            assert int((~res["zero"][:-E.TAIL]).sum()) == d["src"].size          # every compact pixel lands exactly once
            assert np.array_equal(np.sort(res["buf"][:-E.TAIL][~res["zero"][:-E.TAIL]]), np.sort(d["src"].ravel().astype(np.float64)))
        else:
            assert _borderline_act(d["mask"]) == 0
    for h, w, cpad in E.PREPROCESS[:9]:
        res = E.ref_preprocess(E.preprocess_inputs(h, w), cpad)
        assert not res["tol"].any() and int(res["zero"].sum()) == h * w * (cpad - 3)
        assert res["buf"][0] == float(F(0) - E.MEANS[0]) and res["buf"][1] == float(F(255) - E.MEANS[1])


def _borderline_act(x):
    x = np.asarray(x)
    return H.borderline_act(x[~np.isnan(x)])


# ---------------------------------------------------------------------------------------------------------------- mutants
def _adam_case(name, step=0):
    lay = E.LAYOUTS[name]
    st = _state(lay)
    t, gs = E.steps_of(name)[step]
    return lay, st, t, gs, E.layout_refs(name, t, gs)


@pytest.mark.parametrize("mut,quantity,step", [("gs_once", "v", 1), ("v_no_square", "v", 0), ("eps_inside_sqrt", "p", 0), ("lr_not_corrected", "p", 0)])
def test_mutants_of_the_update_rule_fall_outside_the_bound(mut, quantity, step):
    lay, st, t, gs, refs = _adam_case("tiny_1028", step)
    assert mut != "gs_once" or gs != 1
    bad = E.adam_refs(st["p"], st["g"], st["m"], st["v"], t, gs, mut=mut)
    assert _outside(refs[quantity], bad[quantity]["buf"][:lay.n])
    for k in "pmv":                                                            # the reference itself passes its own verdict
        assert not _outside(refs[k], refs[k]["buf"][:lay.n])


@pytest.mark.parametrize("entry", E.LAYOUTS["over_cap"].entries)
def test_mutant_stride_skips_gap(entry):
    lay, st, t, gs, refs = _adam_case("over_cap")
    bad = E.stride_skips_gap(lay, entry, refs, st, t, gs)
    for k in "pmv":
        assert _outside(refs[k], bad[k]), k
    # a small arena never takes the second pass: the same mutant changes nothing there
    lay, st, t, gs, refs = _adam_case("interior")
    same = E.stride_skips_gap(lay, "fused", refs, st, t, gs)
    assert all(np.array_equal(same[k], refs[k]["buf"][:lay.n]) for k in "pmv")


@pytest.mark.parametrize("name", ["interior", "bias_touches_layer_end", "over_cap", "tiny_1028"])
def test_mutants_of_the_shift_refresh(name):
    lay, st, t, gs, _ = _adam_case(name)
    p2 = E.adam_emulate(st["p"], st["g"], st["m"], st["v"], t, gs)[0]
    b = E.bias_inputs(lay.bias[1])
    res = E.ref_shift(p2, b["scale"], b["t0"], *lay.bias)
    for mut in ("shift_from_old_p", "bias_off_by_chunk"):
        assert _outside(res, E.ref_shift(p2, b["scale"], b["t0"], *lay.bias, p_old=st["p"], mut=mut)["buf"][:lay.bias[1]]), mut


def test_mutants_of_the_images():
    lay, st, t, gs, _ = _adam_case("ragged_bf16")
    p2 = E.adam_emulate(st["p"], st["g"], st["m"], st["v"], t, gs)[0]
    for off, k, n, ldw, ldk in lay.bf16:
        good = E.ref_bf16_image(p2, off, k, n, ldw, ldk)
        assert good.size == n * ldk + 2 * E.TAIL and np.array_equal(good[n * ldk:], E.sentinel_halves(2 * E.TAIL))
        for mut in ("image_truncates", "image_pad_kept", "image_untransposed"):
            differs = not np.array_equal(good, E.ref_bf16_image(p2, off, k, n, ldw, ldk, mut=mut))
            expect = {"image_truncates": k * n >= 16, "image_pad_kept": ldk > k, "image_untransposed": k > 1 and n > 1}[mut]
            assert differs or not expect, (mut, off)
    assert (77, 96) in [(k, ldk) for _, k, _, _, ldk in lay.bf16]
    lay, st, t, gs, _ = _adam_case("interior")
    p2 = E.adam_emulate(st["p"], st["g"], st["m"], st["v"], t, gs)[0]
    for off, c, n in lay.wino:
        res = E.ref_wino(p2, off, c, n)
        assert _outside(res, E.ref_wino(p2, off, c, n, p_old=st["p"], mut="wino_from_old_p")["buf"][:36 * c * n])


def test_mutants_of_colsum():
    for m, ordered in ((129, True), (129, False), (4097, True), (513, False)):
        d = E.colsum_inputs(m, 65, 68)
        rows = E.colsum_rows_per_block(m, ordered)
        res = E.ref_colsum(d["g"], 65, d["gscale"], None, rows)
        assert _outside(res, E.ref_colsum(d["g"], 65, d["gscale"], None, rows, mut="colsum_drop_last_row_block")["buf"][:65]), m
    d = E.colsum_inputs(513, 100, 100)
    res = E.ref_colsum(d["g"], 100, d["gscale"], d["old"], 128)
    assert _outside(res, E.ref_colsum(d["g"], 100, d["gscale"], d["old"], 128, mut="colsum_scale_before_old")["buf"][:100])


def test_mutants_of_the_masks_the_scatter_bound_and_the_channel_order():
    hit = dict(scatter_no_bound=0, mask_ge=0, nan_passes=0)
    for case in E.scatter_cases():
        nb, oh, ow, c, s, h, w, masked = case
        d = E.scatter_inputs(case)
        res = E.ref_scatter(d["src"], s, h, w, d["mask"])
        for mut in hit:
            out = _outside(res, E.ref_scatter(d["src"], s, h, w, d["mask"], mut=mut)["buf"][:nb * h * w * c])
            applies = h == oh * s + 1 and not masked if mut == "scatter_no_bound" else masked and nb * h * w * c >= 64
            assert out or not applies, (mut, case)
            hit[mut] += out
    assert all(hit.values()), hit
    for n in (255, 257):
        d = E.flat_inputs(n)
        res = E.ref_relu_mask(d["x"], d["act"])
        for mut in ("mask_ge", "nan_passes"):
            assert _outside(res, E.ref_relu_mask(d["x"], d["act"], mut=mut)["buf"][:n]), (mut, n)
    img = E.preprocess_inputs(15, 17)
    assert _outside(E.ref_preprocess(img, 4), E.ref_preprocess(img, 4, mut="preprocess_rgb_order")["buf"][:15 * 17 * 4])


def test_every_mutant_is_named_and_used():
    import inspect
    src = inspect.getsource(inspect.getmodule(test_every_mutant_is_named_and_used))
    assert all('"%s"' % m in src or "mut=\"%s\"" % m in src for m in E.MUTANTS if m not in ("stride_skips_gap",)), E.MUTANTS
    assert len(set(E.MUTANTS)) == 17
