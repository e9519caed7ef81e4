"""The optimizer and the gradient glue on the device: the four entry points of csrc/adam.hip (radnet_adam_step, _affine, _fused, _bf16) and
radnet_colsum, radnet_scatter_strided, radnet_relu_mask, radnet_scale, radnet_affine_vec, radnet_preprocess_bgr of csrc/elementwise.hip
against the float64 references of tests/update_edge_cases.py (checked against the oracle, and shown to have teeth, by
tests/test_update_edge_cases_reference.py).

Every layout runs through every entry point its table fits, every step with zero_grad = 0 and = 1.  After EVERY launch, for EVERY element of
the full buffers -- the four arenas, the shift, every image, every glue output, each followed by 64 floats prefilled with the sentinel
bits: an element that must be written lies within its bound of update_edge_cases.py and is no NaN, an element that must not be written
still holds the sentinel, an element the contract says is +0.0 holds those bits.  p, m, v, g are judged against float64 from the step's
inputs; the shift, the Winograd images and the bf16 images (bit for bit, the garbage prefill of their K padding turned into zeros) against
the device's own new p.  colsum runs in the ordered and in the atomic form (radnet_set_deterministic, restored in a finally), the ordered
one twice on the same context with the same bits.  The rejection tests call an entry with arguments its host checks refuse: a negative
code, a message that names the entry, no element touched.

`-s` prints the worst err / tol per quantity."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import update_edge_cases as E  # noqa: E402
from test_gpu_head_edges import ERR_HIP, S_INT, _Deterministic, _dev, _Output  # noqa: E402

ENTRY_PAIRS = [(name, entry) for name, lay in E.LAYOUTS.items() for entry in lay.entries]
ENTRY_FN = dict(adam="radnet_adam_step", affine="radnet_adam_step_affine", fused="radnet_adam_step_fused", bf16="radnet_adam_step_bf16")
_CACHE = {}                               # device copies of the arena references: (layout, t, gs, quantity[, zero_grad]) -> _Output


@pytest.fixture(scope="module")
def ctx():
    """The module's one context, on torch's current stream."""
    from radnet_hip import lib as L
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    cx = L.Context(0)
    yield cx
    torch.cuda.synchronize()
    _CACHE.clear()
    cx.close()


def _sentinel(count):
    return torch.full((count,), S_INT, dtype=torch.int32, device="cuda")


def _finish(ctx, what, rc=0):
    """The return code of a launch and the device's verdict on it; a device error ends the session: nothing else runs on this device."""
    msg = ctx.lib.radnet_last_error(ctx.h) if rc else None
    if rc == ERR_HIP:
        pytest.exit("%s: %s" % (what, msg), returncode=3)
    assert rc == 0, (what, rc, msg)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("%s: %s" % (what, e), returncode=3)


def _glue(ctx, what, refs, launch):
    """Fresh buffers of every output in `refs`, one launch, every buffer judged; -> (worst err / tol, the buffers)."""
    outs = {k: _Output(v) for k, v in refs.items()}
    bufs = {k: o.fresh() for k, o in outs.items()}
    _finish(ctx, what, launch(bufs))
    return max(outs[k].judge(bufs[k], what + (k,)) for k in outs), bufs


# ---------------------------------------------------------------------------------------------------------------- Adam
def _arena_output(lay, t, gs, k, zg):
    key = (lay.name, t, float(gs), k) + ((zg,) if k == "g" else ())
    if key not in _CACHE:
        _CACHE[key] = _Output(E.ref_g(E.adam_state(lay.n)["g"], zg) if k == "g" else E.layout_refs(lay.name, t, gs)[k])
    return _CACHE[key]


def _adam(ctx, lay, entry, t, gs, zg):
    """One step of `entry` on the layout's input state, everything judged.  -> (worst err / tol per quantity, the buffers)."""
    from radnet_hip import lib as L
    what = ("adam", lay.name, entry, "t=%d" % t, "gs=%g" % gs, "zero_grad=%d" % zg)
    outs = {k: _arena_output(lay, t, gs, k, zg) for k in "pmvg"}
    bufs = {k: o.fresh() for k, o in outs.items()}
    args = [bufs[k].data_ptr() for k in "pgmv"] + [C.c_int64(lay.n), t, C.c_float(E.LR), C.c_float(E.B1), C.c_float(E.B2), C.c_float(E.EPS), C.c_float(gs), zg]
    bias = lay.bias if entry != "adam" else None
    if bias:
        b = E.bias_inputs(bias[1])
        sd, td = _dev(b["scale"]), _dev(b["t0"])
        bufs["shift"] = _sentinel(bias[1] + E.TAIL).view(torch.float32)
        args += [C.c_int64(bias[0]), C.c_int64(bias[1]), sd.data_ptr(), td.data_ptr(), bufs["shift"].data_ptr()]
    elif entry != "adam":
        args += [C.c_int64(0), C.c_int64(0), None, None, None]
    layers = E.layers_of(lay, entry)
    if entry == "fused":
        arr = (L.AdamWino * max(len(layers), 1))()
        for i, (off, c, n) in enumerate(layers):
            bufs["u%d" % i] = _sentinel(36 * c * n + E.TAIL).view(torch.float32)
            arr[i].off, arr[i].c, arr[i].n, arr[i].u = off, c, n, bufs["u%d" % i].data_ptr()
        args += [arr, len(layers)]
    elif entry == "bf16":
        arr = (L.AdamBf16 * max(len(layers), 1))()
        for i, (off, k, n, ldw, ldk) in enumerate(layers):
            bufs["wt%d" % i] = _sentinel((n * ldk + 2 * E.TAIL) // 2)
            arr[i].off, arr[i].k, arr[i].n, arr[i].ldw, arr[i].wt, arr[i].ldk = off, k, n, ldw, bufs["wt%d" % i].data_ptr(), ldk
        args += [arr, len(layers)]
    _finish(ctx, what, getattr(ctx.lib, ENTRY_FN[entry])(ctx.h, *args))
    worst = {k: outs[k].judge(bufs[k], what + (k,)) for k in "pmvg"}
    assert worst["g"] == 0.0
    if bias or layers:
        p_new = bufs["p"][:lay.n].cpu().numpy()
    if bias:
        worst["shift"] = _Output(E.ref_shift(p_new, b["scale"], b["t0"], *bias)).judge(bufs["shift"], what + ("shift",))
    for i, layer in enumerate(layers):
        if entry == "fused":
            worst["u"] = max(worst.get("u", 0.0), _Output(E.ref_wino(p_new, *layer)).judge(bufs["u%d" % i], what + ("u%d" % i,)))
        else:
            want = torch.from_numpy(E.ref_bf16_image(p_new, *layer).view(np.int16)).cuda()
            got = bufs["wt%d" % i].view(torch.int16)
            wrong = int((got != want).sum())
            assert wrong == 0, (what, "wt%d" % i, layer, "%d words of the image or of its tail differ" % wrong, torch.nonzero(got != want)[:4].tolist())
    return worst, bufs


@pytest.mark.parametrize("name,entry", ENTRY_PAIRS)
def test_adam_every_layout_through_every_entry_it_fits(ctx, name, entry):
    lay = E.LAYOUTS[name]
    worst, launches = {}, 0
    for t, gs in E.steps_of(name):
        for zg in (1, 0):
            w, _ = _adam(ctx, lay, entry, t, gs, zg)
            worst = {k: max(worst.get(k, 0.0), v) for k, v in w.items()}
            launches += 1
    print("adam %s through %s: %d launches, worst err / tol %s" % (name, ENTRY_FN[entry], launches, {k: round(v, 4) for k, v in sorted(worst.items())}))
    assert launches == 2 * len(E.steps_of(name))


@pytest.mark.parametrize("name", [n for n, lay in E.LAYOUTS.items() if not lay.wino and not lay.bf16 and "affine" in lay.entries])
def test_adam_routes_without_layers_give_the_same_bits(ctx, name):
    """_fused with 0 layers and _bf16 with 0 layers against _affine: one sweep, one update routine, the same bits in every buffer."""
    lay = E.LAYOUTS[name]
    for t, gs in E.steps_of(name)[:3]:
        ref = _adam(ctx, lay, "affine", t, gs, 1)[1]
        for entry in ("fused", "bf16"):
            got = _adam(ctx, lay, entry, t, gs, 1)[1]
            assert set(got) == set(ref) == {"p", "m", "v", "g", "shift"}
            for k in ref:
                assert torch.equal(ref[k].view(torch.int32), got[k].view(torch.int32)), (name, entry, t, k)


# ---------------------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("m", E.COLSUM_M)
def test_colsum_ordered_and_atomic(ctx, m):
    worst, launches = 0.0, 0
    for n in E.COLSUM_N:
        for ld in (n, n + 3):
            d = E.colsum_inputs(m, n, ld)
            g, gsd = _dev(d["g"]), _dev(d["gscale"])
            for with_gs, acc in E.COLSUM_MODES:
                for det in (1, 0):
                    ref = dict(out=E.ref_colsum(d["g"], n, d["gscale"] if with_gs else None, d["old"] if acc else None, E.colsum_rows_per_block(m, bool(det))))
                    what = ("colsum", m, n, ld, "gscale" if with_gs else "no gscale", "accumulate" if acc else "store", "ordered" if det else "atomic")
                    call = lambda b: ctx.lib.radnet_colsum(ctx.h, g.data_ptr(), m, n, ld, gsd.data_ptr() if with_gs else None, b["out"].data_ptr(), acc)
                    with _Deterministic(ctx, det):
                        w, first = _glue(ctx, what, ref, call)
                        if det:                                                   # the tickets are back at zero: the same bits, and correct again
                            w2, second = _glue(ctx, what + ("second launch",), ref, call)
                            assert torch.equal(first["out"].view(torch.int32), second["out"].view(torch.int32)), what
                            w, launches = max(w, w2), launches + 1
                    worst, launches = max(worst, w), launches + 1
    print("colsum m=%d: %d launches, worst err / tol %.3f" % (m, launches, worst))
    assert launches == len(E.COLSUM_N) * 2 * len(E.COLSUM_MODES) * 3


# ---------------------------------------------------------------------------------------------------------------- scatter_strided
def _scatter(ctx, case):
    nb, oh, ow, c, s, h, w, masked = case
    d = E.scatter_inputs(case)
    src, mask = _dev(d["src"]), _dev(d["mask"])
    worst, _ = _glue(ctx, ("scatter_strided", case), dict(dst=E.ref_scatter(d["src"], s, h, w, d["mask"])),
                     lambda b: ctx.lib.radnet_scatter_strided(ctx.h, src.data_ptr(), nb, oh, ow, c, s, h, w, mask.data_ptr() if masked else None, b["dst"].data_ptr()))
    assert worst == 0.0                                                           # bit-exact


@pytest.mark.parametrize("s", (1, 2, 3))
def test_scatter_strided_every_extent_channel_count_batch_and_mask(ctx, s):
    cases = [c for c in E.scatter_cases() if c[4] == s]
    assert len(cases) == 24
    for case in cases:
        _scatter(ctx, case)


def test_scatter_strided_past_the_grid_cap(ctx):
    _scatter(ctx, E.SCATTER_OVER)


# ---------------------------------------------------------------------------------------------------------------- relu_mask, scale, affine_vec
@pytest.mark.parametrize("n", E.FLAT_N)
def test_relu_mask_scale_and_affine_vec(ctx, n):
    d = E.flat_inputs(n)
    act, a, b, c = (_dev(d[k]) for k in ("act", "a", "b", "c"))
    exact, _ = _glue(ctx, ("relu_mask", n), dict(g=E.ref_relu_mask(d["x"], d["act"])),
                     lambda o: ctx.lib.radnet_relu_mask(ctx.h, o["g"].data_ptr(), act.data_ptr(), C.c_int64(n)))
    assert exact == 0.0
    for alpha in E.ALPHAS:
        exact, _ = _glue(ctx, ("scale", n, float(alpha)), dict(x=E.ref_scale(d["x"], alpha)),
                         lambda o: ctx.lib.radnet_scale(ctx.h, o["x"].data_ptr(), C.c_int64(n), C.c_float(alpha)))
        assert exact == 0.0
    worst, _ = _glue(ctx, ("affine_vec", n), dict(out=E.ref_affine(d["a"], d["b"], d["c"])),
                     lambda o: ctx.lib.radnet_affine_vec(ctx.h, o["out"].data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr(), C.c_int64(n)))
    print("affine_vec n=%d: worst err / tol %.3f" % (n, worst))


# ---------------------------------------------------------------------------------------------------------------- preprocess_bgr
@pytest.mark.parametrize("i", range(len(E.PREPROCESS)), ids=[str(c) for c in E.PREPROCESS])
def test_preprocess_bgr(ctx, i):
    h, w, cpad = E.PREPROCESS[i]
    img = E.preprocess_inputs(h, w)
    imgd = _dev(img)
    exact, _ = _glue(ctx, ("preprocess_bgr", E.PREPROCESS[i]), dict(out=E.ref_preprocess(img, cpad)),
                     lambda o: ctx.lib.radnet_preprocess_bgr(ctx.h, imgd.data_ptr(), h, w, cpad, o["out"].data_ptr()))
    assert exact == 0.0


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusals(lib, h, z, o):
    """entry -> (the prefix of its messages, [(what, the call)]): arguments the host checks refuse before the memset or the launch."""
    n1 = C.c_int64(-1)
    return {
        "radnet_colsum": ("colsum:", [
            ("m = 0", lambda: lib.radnet_colsum(h, z, 0, 8, 8, None, o, 0)), ("n = 0", lambda: lib.radnet_colsum(h, z, 8, 0, 8, None, o, 0)),
            ("m < 0", lambda: lib.radnet_colsum(h, z, -3, 8, 8, None, o, 1)), ("ld < n", lambda: lib.radnet_colsum(h, z, 8, 8, 7, None, o, 0))]),
        "radnet_scatter_strided": ("scatter_strided:", [
            ("nb = 0", lambda: lib.radnet_scatter_strided(h, z, 0, 3, 4, 4, 2, 6, 8, None, o)), ("oh = 0", lambda: lib.radnet_scatter_strided(h, z, 1, 0, 4, 4, 2, 6, 8, None, o)),
            ("ow = 0", lambda: lib.radnet_scatter_strided(h, z, 1, 3, 0, 4, 2, 6, 8, None, o)), ("c = 0", lambda: lib.radnet_scatter_strided(h, z, 1, 3, 4, 0, 2, 6, 8, None, o)),
            ("c = -4", lambda: lib.radnet_scatter_strided(h, z, 1, 3, 4, -4, 2, 6, 8, None, o)), ("c % 4", lambda: lib.radnet_scatter_strided(h, z, 1, 3, 4, 6, 2, 6, 8, None, o)),
            ("stride = 0", lambda: lib.radnet_scatter_strided(h, z, 1, 3, 4, 4, 0, 6, 8, None, o)),
            ("the grid does not fit", lambda: lib.radnet_scatter_strided(h, z, 1, 3, 4, 4, 2, 4, 8, None, o))]),
        "radnet_preprocess_bgr": ("preprocess:", [
            ("h = 0", lambda: lib.radnet_preprocess_bgr(h, z, 0, 5, 4, o)), ("w = 0", lambda: lib.radnet_preprocess_bgr(h, z, 5, 0, 4, o)),
            ("h < 0", lambda: lib.radnet_preprocess_bgr(h, z, -5, -5, 4, o))]),
        "radnet_scale": ("scale:", [("n < 0", lambda: lib.radnet_scale(h, o, n1, C.c_float(2.0)))]),
        "radnet_relu_mask": ("relu_mask:", [("n < 0", lambda: lib.radnet_relu_mask(h, o, z, n1))]),
        "radnet_affine_vec": ("affine_vec:", [("n < 0", lambda: lib.radnet_affine_vec(h, o, z, z, z, n1))]),
    }


ENTRIES = ("radnet_colsum", "radnet_scatter_strided", "radnet_preprocess_bgr", "radnet_scale", "radnet_relu_mask", "radnet_affine_vec")


@pytest.mark.parametrize("entry", ENTRIES)
def test_refused_arguments_launch_nothing(ctx, entry):
    zeros = torch.zeros(1 << 16, device="cuda")
    out = _sentinel(1 << 16)
    lib, h = ctx.lib, ctx.h
    table = _refusals(lib, h, zeros.data_ptr(), out.data_ptr())
    assert set(table) == set(ENTRIES)
    prefix, calls = table[entry]
    for what, call in calls:
        rc = call()
        msg = lib.radnet_last_error(h)
        assert rc < 0, (entry, what, rc)
        assert msg and msg.decode().startswith(prefix), (entry, what, msg)
    # n = 0 stays a no-op
    zero = C.c_int64(0)
    for rc in (lib.radnet_scale(h, out.data_ptr(), zero, C.c_float(2.0)), lib.radnet_relu_mask(h, out.data_ptr(), zeros.data_ptr(), zero),
               lib.radnet_affine_vec(h, out.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), zeros.data_ptr(), zero)):
        assert rc == 0
    torch.cuda.synchronize()
    assert bool((out == S_INT).all()), (entry, "a refused call or an empty one wrote to an output")
    test_preprocess_bgr(ctx, 0)                                                   # the context still works
