"""Edge shapes, pitches and PINNED decisions of the two fused forward launches, radnet_conv_fwd_pair (conv_fwd_pair_kernel) and
radnet_conv_bottleneck (conv_bneck_kernel, bneck_tail: csrc/conv_mfma.hip, conv_igemm_body.h), against the full-buffer float64
references of tests/fused_fwd_edge_cases.py (proved against the oracle, and shown to have teeth, by
tests/test_fused_fwd_edge_cases_reference.py).

Both entry points decide per shape whether the one-launch form runs (a measurement kept in the tuning table).  Nothing is measured
here: every test writes the table entry it wants -- kind 32 / 33 with slices 1 (one launch on that tile) or 2 (the separate launches),
and kind-0 lines for the layers' own launches -- loads it into an autotuning context, and PROVES which path ran: the class-0 launch
count of that one call (1; 2 for a separate pair; 2 or 3 for a separate bottleneck), the number of tuned shapes unchanged by the call,
and for the bottleneck db->y, which the fused launch leaves at its prefill and the separate launches write.

After every call, for every element of every output buffer: inside the rows |gpu - ref| <= the derived bound (fused_fwd_edge_cases.py),
outside them -- pitch padding, one extra row, the sentinel columns of p_col_blocks -- the prefilled sentinel bits.  Input padding holds
NaN.  An output whose pre-activation is below minus its bound under a ReLU is +0.0 exactly; the integer cases equal float64 exactly.
The paired launch on tile (bm, bn) gives the bits of radnet_conv_fwd of each descriptor forced to that tile with 4 waves (the same
conv_igemm_body instantiation, no unit table), and the same bits twice.  The pitched intermediates (b_pitched_*) give the same
buffers whichever form the table asks for.

`-s` prints the worst err / tol per case, and per entry point at the module's end."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import fused_fwd_edge_cases as F  # noqa: E402

S_INT = int(F.SENTINEL)
ERR_ARG = -1
WORST = {}                   # entry point -> (max err / tol, case, what)


@pytest.fixture(scope="module")
def ctx():
    """The module's one context: a workspace, autotune ON (the fused forms exist only there), launch timing on (the launch counts)."""
    from radnet_hip import lib as L
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test on a machine without a GPU")
    cx = L.Context(0)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    cx.check(cx.lib.radnet_set_workspace(cx.h, ws.data_ptr(), ws.numel()), "set_workspace")
    cx.check(cx.lib.radnet_set_autotune(cx.h, 1), "set_autotune")
    cx.timing(True)
    cx._ws, cx._tables = ws, 0
    yield cx
    torch.cuda.synchronize()
    _restore(cx)
    for entry, (ratio, name, what) in sorted(WORST.items()):
        print("\nfused fwd edges: worst err / tol of %s = %.4f (%s, %s)" % (entry, ratio, name, what), end="")
    print()
    cx.timing(False)
    cx.close()


def _restore(cx):
    cx.lib.radnet_force_config(cx.h, 0, 0, 0)
    cx.lib.radnet_force_waves(cx.h, 0)
    cx.lib.radnet_set_autotune(cx.h, 1)


def _pin(cx, tmp_path, lines):
    """Load a tuning table of these lines (an entry loaded again overwrites the one before)."""
    cx._tables += 1
    table = tmp_path / ("table%d.txt" % cx._tables)
    table.write_text(F.TABLE_HEADER + "\n".join(lines) + "\n")
    cx.check(cx.lib.radnet_tune_load(cx.h, str(table).encode()), "tune_load")


def _counted(cx, call):
    """(return code, class-0 launches of this one call, tuned shapes it added)."""
    torch.cuda.synchronize()
    cx.timing_reset()
    before = cx.lib.radnet_tuned_shapes(cx.h)
    rc = call()
    launches = cx.timing_read(0)[1]
    return rc, launches, cx.lib.radnet_tuned_shapes(cx.h) - before


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the cached inputs are read-only


def _ptr(t):
    return None if t is None else t.data_ptr()


def _upload(l, p):
    """A layer's parameters on the device, laid out with its pitches: NaN in every padding."""
    return dict(w=_dev(F.padded(p["w"], l.ldw)), scale=_dev(p["scale"]), shift=_dev(p["shift"]),
                addend=_dev(F.padded(p["addend"], l.ld_add)) if l.addend else None)


def _desc(shape, l, x_ptr, dv, y_ptr, w_ptr=None):
    from radnet_hip import lib as L
    oh, ow, M, K = F.grid(shape, l)
    d = L.ConvDesc()
    d.nb, d.h, d.w_, d.c, d.oh, d.ow, d.kh, d.kw = shape[0], shape[1], shape[2], l.c, oh, ow, l.k, l.k
    d.stride, d.pad_t, d.pad_l, d.n = l.stride, l.pad, l.pad, l.n
    d.x, d.w, d.y = x_ptr, w_ptr or _ptr(dv["w"]), y_ptr
    d.scale, d.shift, d.addend = _ptr(dv["scale"]), _ptr(dv["shift"]), _ptr(dv["addend"])
    d.ldw, d.ldy, d.ld_add, d.act, d.act_cols = l.ldw, l.ldy, l.ld_add, l.act, l.act_cols
    return d


def _fresh(ref):
    """Every output buffer of a reference, prefilled with the sentinel."""
    return {key: torch.full(v.shape, S_INT, dtype=torch.int32, device="cuda").view(torch.float32) for key, v in ref.val.items()}


def _same_bits(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def _untouched(buf):
    return bool((buf.view(torch.int32) == S_INT).all())


def _judge(bufs, ref, what, entry, keys=None, relu=(), exact=False, half_zero=False):
    """Every element of the buffers `keys` (default: all) against the reference; returns the worst err / tol.  relu: the buffers behind
    a ReLU, whose elements below zero by more than the bound must be +0.0 (half_zero: and are between 0.35 and 0.65 of all)."""
    worst_all = 0.0
    for key in keys or sorted(ref.val):
        got = bufs[key].cpu().numpy()
        bits = got.view(np.int32)
        want, tol = ref.val[key], ref.tol[key]
        worst, bad, spilled = F.verdict(got, bits == S_INT, want, tol)
        if worst > WORST.get(entry, (-1.0,))[0]:
            WORST[entry] = (worst, what[0], what[1:] + (key,))
        assert spilled == 0, (what, key, "%d elements outside the rows lost their sentinel" % spilled)
        assert bad == 0, (what, key, "%d elements outside the bound, worst err / tol %.3f" % (bad, worst))
        inside = ~np.isnan(want)
        if key in relu:
            zero = inside & (np.nan_to_num(ref.pre[key]) < -np.nan_to_num(tol))
            assert (bits[zero] == 0).all(), (what, key, "a ReLU output below zero is not +0.0")
            assert not half_zero or 0.35 < zero.sum() / inside.sum() < 0.65, (what, key, zero.sum(), inside.sum())
        if exact:
            assert np.array_equal(got[inside].astype(np.float64), want[inside]), (what, key, "an integer case is not exact")
        worst_all = max(worst_all, worst)
    return worst_all


# ================================================================================================================ the pair
class _PairProblem:
    def __init__(self, name):
        self.name, self.cs = name, F.PAIRS[name]
        d = F.pair_inputs(name)
        self.x = [_dev(d["x1"])]
        self.x.append(self.x[0] if self.cs.same_x else _dev(d["x2"]))
        self.par = [_upload(l, d["p%d" % (i + 1)]) for i, l in enumerate(self.cs.layers)]
        self.ref = F.pair(name)
        self.relu = [F.pair_slot(self.cs, i)[0] for i, l in enumerate(self.cs.layers) if l.act == 1 and not self.cs.col_block]

    def descs(self, bufs):
        out = []
        for i, l in enumerate(self.cs.layers):
            key, c0, ld = F.pair_slot(self.cs, i)
            out.append(_desc(self.cs.shapes[i], l, _ptr(self.x[i]), self.par[i], bufs[key].data_ptr() + 4 * c0))
        return out

    def single_lines(self):
        return [F.single_line(self.cs.shapes[i], l) for i, l in enumerate(self.cs.layers)]

    def paired(self, cx):
        bufs = _fresh(self.ref)
        d1, d2 = self.descs(bufs)
        rc, launches, grown = _counted(cx, lambda: cx.lib.radnet_conv_fwd_pair(cx.h, C.byref(d1), C.byref(d2)))
        cx.check(rc, self.name)
        return bufs, launches, grown

    def singles(self, cx):
        bufs = _fresh(self.ref)
        d1, d2 = self.descs(bufs)

        def both():
            rc = cx.lib.radnet_conv_fwd(cx.h, C.byref(d1))
            return rc if rc != 0 else cx.lib.radnet_conv_fwd(cx.h, C.byref(d2))
        rc, launches, grown = _counted(cx, both)
        cx.check(rc, self.name)
        return bufs, launches, grown

    def judge(self, bufs, what, entry):
        return _judge(bufs, self.ref, (self.name,) + what, entry, relu=self.relu, exact=self.cs.exact)


@pytest.mark.parametrize("name", [n for n, cs in F.PAIRS.items() if cs.tiles])
def test_pair_case_on_every_tile(ctx, tmp_path, name):
    pr = _PairProblem(name)
    worst = 0.0
    try:
        for bm, bn in pr.cs.tiles:
            _pin(ctx, tmp_path, [F.pair_line(pr.cs, bm, bn, 1)])
            bufs, launches, grown = pr.paired(ctx)
            assert (launches, grown) == (1, 0), (name, bm, bn, "the paired launch did not run as one launch", launches, grown)
            worst = max(worst, pr.judge(bufs, (bm, bn), "fwd_pair, one launch"))                                   # (a)
            again, launches, grown = pr.paired(ctx)
            assert (launches, grown) == (1, 0) and _same_bits(bufs, again), ("two runs differ", name, bm, bn)     # (c)
            ctx.check(ctx.lib.radnet_force_config(ctx.h, bm, bn, 1), "force_config")
            ctx.check(ctx.lib.radnet_force_waves(ctx.h, 4), "force_waves")
            alone, launches, grown = pr.singles(ctx)
            _restore(ctx)
            assert (launches, grown) == (2, 0), (name, bm, bn, launches, grown)
            pr.judge(alone, (bm, bn, "forced singles"), "conv_fwd forced to the pair's tile")
            assert _same_bits(bufs, alone), ("the paired launch is not the two forced convolutions bit for bit", name, bm, bn)   # (b)
    finally:
        _restore(ctx)
    print("%s: %d tiles, worst err / tol %.4f" % (name, len(pr.cs.tiles), worst))


PAIR_FALLBACKS = ["p_diff_m", "p_diff_k", "p_stem", "force_config", "autotune_off", "slices_2", "tile_128x128", "tile_64x128"]


@pytest.mark.parametrize("which", PAIR_FALLBACKS)
def test_pair_fallback_is_the_two_calls_bit_for_bit(ctx, tmp_path, which):
    pr = _PairProblem(which if which in F.PAIRS else "p_ragged")
    lines = pr.single_lines()                                   # the layers' own launches: nothing is measured
    if which == "slices_2":
        lines.append(F.pair_line(pr.cs, 64, 64, 2))
    elif which.startswith("tile_"):
        a, b = (int(v) for v in which[5:].split("x"))
        lines.append(F.pair_line(pr.cs, a, b, 1))               # the paired form has no such tile: it returns unsupported
    elif which in ("force_config", "autotune_off"):
        lines.append(F.pair_line(pr.cs, 64, 64, 1))             # the table asks for one launch; the context's state overrides it
    _pin(ctx, tmp_path, lines)
    try:
        if which == "force_config":
            ctx.check(ctx.lib.radnet_force_config(ctx.h, 64, 64, 1), "force_config")
            ctx.check(ctx.lib.radnet_force_waves(ctx.h, 4), "force_waves")
        if which == "autotune_off":
            ctx.check(ctx.lib.radnet_set_autotune(ctx.h, 0), "set_autotune")
        bufs, launches, grown = pr.paired(ctx)
        assert (launches, grown) == (2, 0), (which, "expected the two launches", launches, grown)
        pr.judge(bufs, (which,), "fwd_pair, two launches")
        alone, launches, grown = pr.singles(ctx)
        assert (launches, grown) == (2, 0) and _same_bits(bufs, alone), (which, "not the two calls bit for bit")
    finally:
        _restore(ctx)


def test_pair_null_arguments_launch_nothing(ctx, tmp_path):
    pr = _PairProblem("p_ragged")
    _pin(ctx, tmp_path, [F.pair_line(pr.cs, 64, 64, 1)])
    bufs = _fresh(pr.ref)
    d1, d2 = pr.descs(bufs)
    lib = ctx.lib
    for what, call in (("ctx", lambda: lib.radnet_conv_fwd_pair(None, C.byref(d1), C.byref(d2))),
                       ("d1", lambda: lib.radnet_conv_fwd_pair(ctx.h, None, C.byref(d2))),
                       ("d2", lambda: lib.radnet_conv_fwd_pair(ctx.h, C.byref(d1), None))):
        rc, launches, grown = _counted(ctx, call)
        assert (rc, launches, grown) == (ERR_ARG, 0, 0), (what, rc, launches, grown)
    torch.cuda.synchronize()
    assert all(_untouched(b) for b in bufs.values())
    ok, launches, grown = pr.paired(ctx)                        # the context still works
    assert launches == 1
    pr.judge(ok, ("after the refusals",), "fwd_pair, one launch")


# ================================================================================================================ the bottleneck
class _BneckProblem:
    def __init__(self, name):
        self.name, self.cs = name, F.BNECKS[name]
        d = F.bneck_inputs(name)
        self.x, self.x2 = _dev(d["x"]), _dev(d["x2"])
        self.par = [_upload(l, d[k]) for l, k in zip(self.cs.layers, ("pb", "pc", "pa"))]
        self.M = self.cs.shape[0] * self.cs.shape[1] * self.cs.shape[2]

    def lines(self, with_next, rows, slices):
        flat = (1, 1, self.M)
        lb, lc, la = self.cs.layers
        out = [F.bneck_line(self.cs, with_next, rows, slices), F.single_line(self.cs.shape, lb), F.single_line(flat, lc)]
        return out + ([F.single_line(flat, la)] if with_next else [])

    def run(self, cx, with_next, w_ptrs=(None, None, None), expect_rc=0):
        ref = F.chain(self.name, with_next)
        bufs = _fresh(ref)
        lb, lc, la = self.cs.layers
        flat = (1, 1, self.M)
        db = _desc(self.cs.shape, lb, _ptr(self.x), self.par[0], bufs["t2"].data_ptr(), w_ptrs[0])
        dc = _desc(flat, lc, bufs["t2"].data_ptr() if self.cs.linked else _ptr(self.x2), self.par[1], bufs["y"].data_ptr(), w_ptrs[1])
        da = _desc(flat, la, bufs["y"].data_ptr(), self.par[2], bufs["t"].data_ptr(), w_ptrs[2]) if with_next else None
        rc, launches, grown = _counted(cx, lambda: cx.lib.radnet_conv_bottleneck(cx.h, C.byref(db), C.byref(dc), C.byref(da) if da else None))
        if expect_rc == 0:
            cx.check(rc, self.name)
        else:
            assert rc == expect_rc, (self.name, rc)
        return bufs, launches, grown

    def judge(self, bufs, with_next, what, entry, keys):
        ref = F.chain(self.name, with_next)
        relu = [k for k, l in zip(F.BNECK_KEYS, self.cs.layers) if l.act == 1 and k in keys]
        return _judge(bufs, ref, (self.name, "next" if with_next else "no next") + what, entry, keys=keys, relu=relu, exact=self.cs.exact,
                      half_zero=self.name == "b_relu_exact")


def _outputs(with_next):
    return ["y", "t"] if with_next else ["y"]


PLAIN = [n for n, cs in F.BNECKS.items() if cs.fusable]
REFUSED_SHAPES = [n for n, cs in F.BNECKS.items() if not cs.fusable and n not in F.PITCHED_INTERMEDIATE]


@pytest.mark.parametrize("name", PLAIN)
def test_bottleneck_case_fused_and_separate(ctx, tmp_path, name):
    pr = _BneckProblem(name)
    worst = {1: 0.0, 2: 0.0}
    for with_next in pr.cs.forms:
        for rows in (64, 32):
            for slices in (1, 2):
                _pin(ctx, tmp_path, pr.lines(with_next, rows, slices))
                bufs, launches, grown = pr.run(ctx, with_next)
                what = (rows, "fused" if slices == 1 else "separate")
                assert grown == 0, (name, what, "something was measured")
                if slices == 1:
                    assert launches == 1, (name, with_next, what, launches)
                    assert _untouched(bufs["t2"]), (name, what, "the fused launch wrote db->y")
                    worst[1] = max(worst[1], pr.judge(bufs, with_next, what, "bottleneck, one launch", _outputs(with_next)))
                    again, launches, grown = pr.run(ctx, with_next)
                    assert launches == 1 and _same_bits(bufs, again), ("two runs differ", name, with_next, what)
                else:
                    assert launches == (3 if with_next else 2), (name, with_next, what, launches)
                    worst[2] = max(worst[2], pr.judge(bufs, with_next, what, "bottleneck, separate launches", ["t2"] + _outputs(with_next)))
    print("%s: worst err / tol fused %.4f, separate %.4f" % (name, worst[1], worst[2]))


@pytest.mark.parametrize("name", REFUSED_SHAPES)
def test_bottleneck_shape_the_fused_kernel_does_not_take_runs_separately(ctx, tmp_path, name):
    pr = _BneckProblem(name)
    for with_next in pr.cs.forms:
        for rows in (64, 32):
            _pin(ctx, tmp_path, pr.lines(with_next, rows, 1))                  # the table asks for one launch
            bufs, launches, grown = pr.run(ctx, with_next)
            assert (launches, grown) == (3 if with_next else 2, 0), (name, with_next, rows, launches, grown)
            pr.judge(bufs, with_next, (rows, "refused shape"), "bottleneck, separate launches", ["t2"] + _outputs(with_next))


@pytest.mark.parametrize("which", ["rows_128", "force_config", "autotune_off"])
@pytest.mark.parametrize("with_next", [False, True])
def test_bottleneck_fallback_by_table_or_context_state(ctx, tmp_path, which, with_next):
    pr = _BneckProblem("b_m_seams_65")
    _pin(ctx, tmp_path, pr.lines(with_next, 128 if which == "rows_128" else 64, 1))
    try:
        if which == "force_config":
            ctx.check(ctx.lib.radnet_force_config(ctx.h, 64, 64, 1), "force_config")
            ctx.check(ctx.lib.radnet_force_waves(ctx.h, 4), "force_waves")
        if which == "autotune_off":
            ctx.check(ctx.lib.radnet_set_autotune(ctx.h, 0), "set_autotune")
        bufs, launches, grown = pr.run(ctx, with_next)
        assert (launches, grown) == (3 if with_next else 2, 0), (which, with_next, launches, grown)
        pr.judge(bufs, with_next, (which,), "bottleneck, separate launches", ["t2"] + _outputs(with_next))
    finally:
        _restore(ctx)
    if which != "rows_128":                                     # the same table entry gives one launch once the context's state is back
        assert pr.run(ctx, with_next)[1] == 1


@pytest.mark.parametrize("layer", [1, 2])
def test_bottleneck_misaligned_weights_are_refused_by_the_separate_launches(ctx, tmp_path, layer):
    """A dc->w / da->w that is not 16-byte aligned keeps the call off the fused kernel (its weight loads need no alignment, the
    guard still asks for it) -- and radnet_conv_fwd, which the call then means, refuses such a pointer: RADNET_ERR_ARG with a message,
    the layers before it have run, the refused layer's output is untouched."""
    pr = _BneckProblem("b_m_seams_65")
    l = pr.cs.layers[layer]
    d = F.bneck_inputs(pr.name)[("pb", "pc", "pa")[layer]]
    shifted = torch.cat([torch.full((1,), float("nan"), device="cuda"), pr.par[layer]["w"].reshape(-1)])
    w_ptrs = [None, None, None]
    w_ptrs[layer] = shifted.data_ptr() + 4
    assert w_ptrs[layer] % 16 == 4 and d["w"].shape == (l.k * l.k * l.c, l.n)
    _pin(ctx, tmp_path, pr.lines(True, 64, 1))
    bufs, launches, grown = pr.run(ctx, True, tuple(w_ptrs), expect_rc=ERR_ARG)
    msg = ctx.lib.radnet_last_error(ctx.h)
    assert msg and b"aligned" in msg, msg
    assert (launches, grown) == (layer, 0)
    assert _untouched(bufs["t"]) and (_untouched(bufs["y"]) if layer == 1 else True)
    pr.judge(bufs, True, ("misaligned w of layer %d" % layer,), "bottleneck, separate launches", ["t2", "y"][:layer])


@pytest.mark.parametrize("name", F.PITCHED_INTERMEDIATE)
def test_bottleneck_pitched_intermediate_gives_the_same_buffers_under_both_pinnings(ctx, tmp_path, name):
    """db->y of pitch 72 (dc->y of pitch n + 8 with da): the next layer reads it as a dense matrix, so only the separate launches can
    mean what the header says -- the table's wish for one launch must not change a single bit."""
    pr = _BneckProblem(name)
    upstream = ["t2"] if name == "b_pitched_t2" else ["t2", "y"]                # what lies before the pitched read: judged against float64
    for with_next in pr.cs.forms:
        for rows in (64, 32):
            got = {}
            for slices in (1, 2):
                _pin(ctx, tmp_path, pr.lines(with_next, rows, slices))
                bufs, launches, grown = pr.run(ctx, with_next)
                assert grown == 0
                pr.judge(bufs, with_next, (rows, "pinned %d" % slices), "bottleneck, separate launches", upstream)
                got[slices] = (bufs, launches)
            assert _same_bits(got[1][0], got[2][0]), (name, with_next, rows, "the two pinnings return different buffers")
            assert got[1][1] == got[2][1] == (3 if with_next else 2), (name, with_next, rows, got[1][1], got[2][1])


def test_bottleneck_null_arguments_launch_nothing(ctx, tmp_path):
    pr = _BneckProblem("b_m_seams_65")
    _pin(ctx, tmp_path, pr.lines(False, 64, 1))
    ref = F.chain(pr.name, False)
    bufs = _fresh(ref)
    lb, lc, la = pr.cs.layers
    db = _desc(pr.cs.shape, lb, _ptr(pr.x), pr.par[0], bufs["t2"].data_ptr())
    dc = _desc((1, 1, pr.M), lc, bufs["t2"].data_ptr(), pr.par[1], bufs["y"].data_ptr())
    lib = ctx.lib
    for what, call in (("ctx", lambda: lib.radnet_conv_bottleneck(None, C.byref(db), C.byref(dc), None)),
                       ("db", lambda: lib.radnet_conv_bottleneck(ctx.h, None, C.byref(dc), None)),
                       ("dc", lambda: lib.radnet_conv_bottleneck(ctx.h, C.byref(db), None, None))):
        rc, launches, grown = _counted(ctx, call)
        assert (rc, launches, grown) == (ERR_ARG, 0, 0), (what, rc, launches, grown)
    torch.cuda.synchronize()
    assert all(_untouched(b) for b in bufs.values())
