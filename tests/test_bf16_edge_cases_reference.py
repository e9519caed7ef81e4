"""Device-free checks of tests/bf16_edge_cases.py, the case table and references of tests/test_gpu_bf16_edges.py:

  * the references are right: over unrounded operands they equal oracle.dense.conv2d / conv2d_bwd in float64 (4-tuple padding, so the
    asymmetric and the kh != kw cases are covered) to 1e-12 of the largest value;
  * the rounding guard holds for every case: somewhere the rounded and the unrounded reference differ by more than the bound, so a
    kernel that skipped the bf16 rounding cannot pass the GPU test;
  * every case lands on the output tile it is listed under, by the LIBRARY's rule (radnet_conv_bf16_tile_shape, the function the
    launchers call), and has the reduction tiles its splits need."""
import ctypes as C
import os

import numpy as np
import pytest

import bf16_edge_cases as E
from oracle import dense
from radnet_hip import lib as L


def _lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max()) <= 1e-12 * max(float(np.abs(b).max()), 1e-300)


@pytest.mark.parametrize("name", list(E.CASES))
def test_unrounded_reference_equals_the_oracle(name):
    cs, d, g, r = E.CASES[name], E.inputs(name), E.geometry(E.CASES[name]), E.reference(name)
    w4 = d["w"].astype(np.float64).reshape(cs.kh, cs.kw, cs.c, cs.n)
    if cs.kind == "fwd":
        y = dense.conv2d(d["x"].astype(np.float64), w4, None, cs.stride, cs.pad)
        assert y.shape == (cs.nb, g["oh"], g["ow"], cs.n)
        assert _close(r["dot_u"], y.reshape(g["M"], cs.n))
        return
    gm = E.g_matrix(name).astype(np.float64).reshape(cs.nb, g["oh"], g["ow"], cs.n)
    x = d["x"].astype(np.float64) if cs.kind == "wgrad" else np.zeros((cs.nb, cs.h, cs.w, cs.c))
    dx, dw, db = dense.conv2d_bwd(x, w4, gm, cs.stride, cs.pad, need_dx=cs.kind == "dgrad")
    if cs.kind == "dgrad":
        assert cs.stride == 1 and dx.shape == (cs.nb, cs.h, cs.w, cs.c)
        assert _close(r["dot_u"], dx.reshape(g["P"], cs.c))
    else:
        assert _close(r["dot_u"], dw.reshape(g["K"], cs.n))
        assert _close(r["db_u"], db)


@pytest.mark.parametrize("name", list(E.CASES))
def test_rounding_guard_and_bound_are_meaningful(name):
    cs = E.CASES[name]
    for mode in cs.opts.get("modes", (0,)):
        ref, ref_u, tol = E.expected(name, mode)
        g = E.geometry(cs)
        assert ref.shape == ref_u.shape == tol.shape == (g["rows"], g["cols"])
        assert np.isfinite(ref).all() and np.isfinite(ref_u).all() and (tol > 0).all()
        assert (np.abs(ref_u - ref) > tol).any(), "a kernel on unrounded operands would pass %s" % name


def test_g_is_one_fp32_multiply_before_rounding():
    """bf16(dy * gscale) is not bf16(dy) * gscale: the reference rounds AFTER the multiply, as the kernel headers state."""
    name = "dgrad_3x3_n24_all"
    d = E.inputs(name)
    assert not np.array_equal(E.bf16_round(E.g_matrix(name)), E.bf16_round(d["dy"]) * d["gscale"][None, :].astype(np.float64))
    assert E.g_matrix(name).dtype == np.float32


def test_bf16_round_is_nearest_even():
    v = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 1e-40], np.float32)
    assert list(E.bf16_bits(v)) == [0x3F80, 0x3F82, 0x3F80, 0xBF81, int(np.float32(1e-40).view(np.uint32) + 0x8000) >> 16]
    b = E._biased(np.random.RandomState(0), (4096,))
    lo = (b > 1) & (b < 1 + 2.0 ** -8)
    assert 0.4 < lo.mean() < 0.6 and (E.bf16_round(b[lo]) == 1.0).all()


@pytest.mark.parametrize("name", list(E.CASES))
def test_case_lands_on_its_template_and_has_its_reduction_tiles(name):
    cs, g = E.CASES[name], E.geometry(E.CASES[name])
    bm, bn = C.c_int32(), C.c_int32()
    tiles = _lib().radnet_conv_bf16_tile_shape(g["rows"], g["cols"], C.byref(bm), C.byref(bn))
    assert (bm.value, bn.value) == cs.template, (name, bm.value, bn.value)
    assert tiles == -(-g["rows"] // bm.value) * -(-g["cols"] // bn.value)
    if cs.tiles is not None:
        assert tiles == cs.tiles, (name, tiles)
    assert tiles <= 8192                                                   # the arrival counters of a context
    for s in E.NEEDS_SPLITS.get(name, ()):
        assert s in E.splits(cs), (name, s, g["nrt"])
    if name in E.SINGLE_TILE:
        assert g["nrt"] == 1 and E.splits(cs) == [1]
    # the kernels' stated contract, so that no case is refused
    if cs.kind in ("fwd", "wgrad"):
        assert cs.c % 8 == 0
    if cs.kind == "wgrad":
        assert cs.n % 8 == 0
    if cs.kind == "dgrad":
        assert cs.n % 4 == 0 and cs.stride == 1 and E.pitches(cs)["ld_dy"] > g["n8"] and E.pitches(cs)["ld_dy"] % 4 == 0
    # slabs stay well inside the module's 256 MB workspace, an operand below 20 MB (the largest: dx_add of the 2070 x 2056 data gradient)
    assert tiles * max(E.splits(cs)) * bm.value * bn.value * 4 <= 128 << 20
    assert max(v.nbytes for v in E.inputs(name).values() if v is not None) <= 20 << 20


def test_table_reaches_every_template_and_edge():
    by = {}
    for cs in E.CASES.values():
        by.setdefault(cs.kind, set()).add(cs.template)
    assert all(by[k] == {(128, 128), (128, 64), (64, 64)} for k in ("fwd", "dgrad", "wgrad")), by
    assert all(any(cs.kind == k and cs.kh != cs.kw for cs in E.CASES.values()) for k in ("fwd", "dgrad", "wgrad"))
    nrt = {n: E.geometry(cs)["nrt"] for n, cs in E.CASES.items()}
    assert nrt["wgrad_128x128_ragged"] == 4 and nrt["fwd_deep_k"] == 33 and nrt["dgrad_30_tiles"] == 30 and nrt["wgrad_9_tiles"] >= 8
    order = E.gpu_order()
    assert sorted(order) == sorted(E.CASES) and [E.CASES[n].kind for n in order[:6]] == ["fwd", "dgrad", "wgrad"] * 2
    g = E.geometry(E.CASES["fwd_s2_3x3_pad_br"])
    assert (g["oh"], g["ow"]) == (7, 6)                                    # ceil(13 / 2), ceil(11 / 2) with pad_t = pad_l = 0


def test_tile_shape_rule_matches_its_documentation():
    lib = _lib()
    bm, bn = C.c_int32(-1), C.c_int32(-1)
    assert lib.radnet_conv_bf16_tile_shape(0, 8, C.byref(bm), C.byref(bn)) == 0 and (bm.value, bn.value) == (-1, -1)
    assert lib.radnet_conv_bf16_tile_shape(8, 8, None, C.byref(bn)) == 0
    cd = lambda a, b: -(-a // b)
    for rows, cols in [(1, 1), (16384, 64), (16384, 65), (32768, 64), (980, 2048), (2394, 512), (14700, 256), (1 << 19, 2048), (8192, 128), (8191 * 16 + 1, 128)]:
        t = lib.radnet_conv_bf16_tile_shape(rows, cols, C.byref(bm), C.byref(bn))
        if cols > 64 and cd(rows, 128) * cd(cols, 128) >= 256:
            want = (128, 128)
        elif cd(rows, 128) * cd(cols, 64) >= 256:
            want = (128, 64)
        else:
            want = (64, 64)
        assert (bm.value, bn.value) == want and t == cd(rows, want[0]) * cd(cols, want[1]), (rows, cols)
