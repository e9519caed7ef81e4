"""Edge shapes and forced splits of the three bf16 matrix-core conv kernels (csrc/conv_bf16.hip forward, csrc/conv_bf16_bwd.hip data and
weight gradient) against the full-output float64 references of tests/bf16_edge_cases.py (proved against the oracle on the CPU by
tests/test_bf16_edge_cases_reference.py): ragged last tiles of all three output tile templates, reductions of one tile / with padding
/ with taps that change inside a tile, kh != kw, n % 8 == 4, every split of {1, 2, 3, nrt} -- uneven slices and one tile per slice --
and the workspace rules of a split.

Every output is allocated wider than its row and one row longer, prefilled with a sentinel NaN: after a launch EVERY element inside
[rows) x [cols) is within the bound of the existing bf16 kernel tests, 1e-5 * sum|a*b| (* scale) + 1e-6 * (1 + |tail|), of the
reference over bf16-rounded operands (and somewhere further than that from the unrounded reference), and every element outside still
holds the sentinel's bits.  Input pitches differ from the output's and from each other and hold NaN in their padding.  The cases run
in an order that alternates forward, dgrad and wgrad on ONE context: the three share its arrival counters and slab area, so a counter
one launch left non-zero shows up in the next.

Measured on one MI355X (`-s` prints max err / bound per case and split, and a summary at the module's end): worst err / bound
0.019 forward (fwd_deep_k), 0.017 dgrad (dgrad_30_tiles), 0.012 wgrad (wgrad_128x128_ragged); the module takes 3.4 to 4.7 s.  Each of these
kernel edits made it fail: the addend read with the output's pitch (parity, non-finite), the column guard of the backward epilogue
dropped (sentinels in the pitch padding), dgrad's dy columns >= n left live (non-finite), slices of floor(nrt / split) tiles (parity at
splits 2 and 3), wgrad's dy read with pitch n (non-finite).  Dropping the ROW guard of the epilogue changes nothing: the output's
buffer descriptor ends with the last valid row, so the hardware drops those stores (the extra sentinel row stays as a check of that
extent)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bf16_edge_cases as E  # noqa: E402

WORST = {}                   # kind -> (max err / bound, case, split)


@pytest.fixture(scope="module")
def ctx():
    """The module's one context: a 256 MB workspace, torch's current stream."""
    from radnet_hip import lib as L
    cx = L.Context(0)
    ws = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    cx.check(cx.lib.radnet_set_workspace(cx.h, ws.data_ptr(), ws.numel()), "set_workspace")
    cx._ws = ws
    yield cx
    torch.cuda.synchronize()
    for kind, (ratio, name, s) in sorted(WORST.items()):
        print("\nbf16 edges: worst err / bound of %s = %.3f (%s, split %d)" % (kind, ratio, name, s), end="")
    print()


def _sentinel_buffer(rows, ld, cols=0, inside=None):
    """[rows + 1][ld] fp32 on the device, every element the sentinel NaN but [rows) x [cols) when `inside` is given."""
    a = np.full((rows + 1, ld), E.SENTINEL, np.uint32)
    if inside is not None:
        a.view(np.float32)[:rows, :cols] = inside
    return torch.from_numpy(a.view(np.float32)).cuda()


class _Problem:
    """One case on the device: inputs laid out with the case's pitches (NaN in every padding), and its launches."""

    def __init__(self, cx, name):
        from radnet_hip import lib as L
        self.L, self.name, self.cs = L, name, E.CASES[name]
        cs, d, g, p = self.cs, E.inputs(name), E.geometry(E.CASES[name]), E.pitches(E.CASES[name])
        self.g, self.p = g, p
        cu = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the cached inputs are read-only
        self.w = cu(E.padded(d["w"], p["ldw"]))
        taps = cs.kh * cs.kw
        if cs.kind == "fwd":
            self.x, self.scale, self.shift = cu(d["x"]), cu(d["scale"]), cu(d["shift"])
            self.addend = cu(E.padded(d["addend"], p["ld_add"]))
            self.wt = torch.full((cs.n, p["ldk"]), 0x7FC0, dtype=torch.int16, device="cuda")          # bf16 NaN where the cast must write zeros
            cx.call("radnet_weights_to_bf16", self.w, g["K"], cs.n, p["ldw"], self.wt, p["ldk"])
        elif cs.kind == "dgrad":
            self.dy, self.gscale = cu(E.padded(d["dy"], p["ld_dy"])), cu(d["gscale"])               # NaN in the columns >= n
            self.add = cu(E.padded(d["dx_add"], p["ld_dx_add"])) if d["dx_add"] is not None else None
            self.mask = cu(E.padded(d["dx_mask"], p["ld_dx_mask"])) if d["dx_mask"] is not None else None
            self.wd = torch.full((cs.c, p["ldkd"]), 0x7FC0, dtype=torch.int16, device="cuda")
            cx.call("radnet_weights_to_bf16_dgrad", self.w, taps, cs.c, cs.n, p["ldw"], self.wd, p["ldkd"])
        else:
            self.x, self.dy, self.gscale = cu(d["x"]), cu(E.padded(d["dy"], p["ld_dy_w"])), cu(d["gscale"])
        self.db = None

    def desc(self):
        cs, g, p = self.cs, self.g, self.p
        d = self.L.ConvDesc()
        d.nb, d.h, d.w_, d.c, d.oh, d.ow, d.kh, d.kw = cs.nb, cs.h, cs.w, cs.c, g["oh"], g["ow"], cs.kh, cs.kw
        d.stride, d.pad_t, d.pad_l, d.n = cs.stride, cs.pad[0], cs.pad[1], cs.n
        ptr = lambda t: None if t is None else t.data_ptr()
        if cs.kind == "fwd":
            d.x, d.scale, d.shift, d.addend = ptr(self.x), ptr(self.scale), ptr(self.shift), ptr(self.addend)
            d.ldw, d.ldy, d.ld_add, d.act, d.act_cols = p["ldw"], p["ldy"], p["ld_add"], cs.opts.get("act", 0), cs.opts.get("act_cols", 0)
        elif cs.kind == "dgrad":
            d.dy, d.ld_dy, d.gscale, d.dx_add, d.dx_mask = ptr(self.dy), p["ld_dy"], ptr(self.gscale), ptr(self.add), ptr(self.mask)
            d.ld_dx, d.ld_dx_add, d.ld_dx_mask = p["ld_dx"], p["ld_dx_add"], p["ld_dx_mask"]
        else:
            d.x, d.dy, d.ld_dy, d.gscale, d.ldw = ptr(self.x), ptr(self.dy), p["ld_dy_w"], ptr(self.gscale), p["ld_dw"]
        return d

    def out_pitch(self):
        return {"fwd": self.p["ldy"], "dgrad": self.p["ld_dx"], "wgrad": self.p["ld_dw"]}[self.cs.kind]

    def launch(self, cx, split, mode=0, plain=False):
        """One launch into a fresh sentinel buffer: (return code, the whole buffer on the host as uint32 bits)."""
        cs, g, d = self.cs, self.g, self.desc()
        inside = None
        if cs.kind == "wgrad" and mode != 0:
            inside = E.inputs(self.name)["dw0"] if mode == 1 else 0.0
        out = _sentinel_buffer(g["rows"], self.out_pitch(), g["cols"], inside)
        if cs.kind == "fwd":
            d.y = out.data_ptr()
            rc = cx.lib.radnet_conv_fwd_bf16(cx.h, C.byref(d), self.wt.data_ptr(), self.p["ldk"]) if plain else \
                cx.lib.radnet_conv_fwd_bf16_split(cx.h, C.byref(d), self.wt.data_ptr(), self.p["ldk"], split)
        elif cs.kind == "dgrad":
            d.dx = out.data_ptr()
            rc = cx.lib.radnet_conv_dgrad_bf16(cx.h, C.byref(d), self.wd.data_ptr(), self.p["ldkd"]) if plain else \
                cx.lib.radnet_conv_dgrad_bf16_split(cx.h, C.byref(d), self.wd.data_ptr(), self.p["ldkd"], split)
        else:
            d.dw, d.dw_accumulate = out.data_ptr(), mode
            if cs.opts.get("db"):
                db_in = E.inputs(self.name)["db0"] if mode == 1 else (0.0 if mode == 2 else None)
                self.db = _sentinel_buffer(1, cs.n + 8, cs.n, db_in)
                d.db = self.db.data_ptr()
            rc = cx.lib.radnet_conv_wgrad_bf16(cx.h, C.byref(d), 0 if plain else split)
        return rc, out.cpu().numpy().view(np.uint32)


def _check(name, bits, mode, split):
    """Sentinels outside [rows) x [cols), finite inside, the bound on every element, the bf16 guard."""
    cs, g = E.CASES[name], E.geometry(E.CASES[name])
    rows, cols = g["rows"], g["cols"]
    assert (bits[:rows, cols:] == E.SENTINEL).all(), (name, split, "a store landed in the pitch padding")
    assert (bits[rows:] == E.SENTINEL).all(), (name, split, "a store landed past the last row")
    got = bits.view(np.float32)[:rows, :cols].astype(np.float64)
    assert np.isfinite(got).all(), (name, split, int((~np.isfinite(got)).sum()))
    ref, ref_u, tol = E.expected(name, mode)
    err = np.abs(got - ref)
    ratio, ratio_u = float((err / tol).max()), float((np.abs(got - ref_u) / tol).max())
    print("%s mode %d split %d: max err / bound %.3f (against unrounded operands %.1f)" % (name, mode, split, ratio, ratio_u))
    if ratio > WORST.get(cs.kind, (0.0,))[0]:
        WORST[cs.kind] = (ratio, name, split)
    assert (err <= tol).all(), (name, mode, split, ratio, np.unravel_index(np.argmax(err / tol), err.shape))
    assert ratio_u > 1.0, ("the result is as close to the unrounded operands: not a bf16 path?", name, ratio_u)


def _check_db(pr, mode):
    """db = fp32 column sum of the UNROUNDED dy * gscale added in index order: within M * 2^-24 * sum|g| (the worst case of a sequential
    fp32 sum) + 2^-23 * (1 + |what it was added to|) of the fp64 sum; the sum of the bf16-rounded g lies outside that."""
    name, cs, g = pr.name, pr.cs, pr.g
    r, d = E.reference(name), E.inputs(name)
    bits = pr.db.cpu().numpy().view(np.uint32)
    assert (bits[0, cs.n:] == E.SENTINEL).all() and (bits[1:] == E.SENTINEL).all()
    base = d["db0"].astype(np.float64) if mode == 1 else 0.0
    tol = g["M"] * 2.0 ** -24 * r["db_abs"] + 2.0 ** -23 * (1.0 + np.abs(base))
    got = bits.view(np.float32)[0, :cs.n].astype(np.float64)
    assert (np.abs(got - (r["db_u"] + base)) <= tol).all(), (name, mode, float((np.abs(got - (r["db_u"] + base)) / tol).max()))
    assert (np.abs(E.bf16_round(E.g_matrix(name)).sum(0) - r["db_u"]) > tol).any()


@pytest.mark.parametrize("name", E.gpu_order())
def test_edge_case_every_split(ctx, name):
    cs = E.CASES[name]
    pr = _Problem(ctx, name)
    for mode in cs.opts.get("modes", (0,)):
        first = {}
        for s in E.splits(cs):
            rc, a = pr.launch(ctx, s, mode)
            ctx.check(rc, name)
            _check(name, a, mode, s)
            if pr.db is not None:
                _check_db(pr, mode)
            rc, b = pr.launch(ctx, s, mode)
            ctx.check(rc, name)
            assert np.array_equal(a, b), ("two runs differ", name, mode, s)
            first[s] = a
        rc, plain = pr.launch(ctx, 0, mode, plain=True)
        ctx.check(rc, name)
        assert np.array_equal(plain, first[1]), ("split 1 is not the one-pass launch", name, mode)


# ------------------------------------------------------------------------------------------------------------ workspace rules
def _slab_bytes(cx, cs, split):
    """tiles x split x BM x BN x 4 with the library's own tile shape."""
    g = E.geometry(cs)
    bm, bn = C.c_int32(), C.c_int32()
    tiles = cx.lib.radnet_conv_bf16_tile_shape(g["rows"], g["cols"], C.byref(bm), C.byref(bn))
    return tiles * split * bm.value * bn.value * 4


BWD_WS = ("dgrad_30_tiles", "wgrad_9_tiles")
FWD_WS = "fwd_s2_3x3_split"


def test_small_workspace_backward_halves_forward_refuses(ctx):
    """A workspace that holds the slabs of 2 slices but not of 4: a backward launch asked for 8 runs with 2 (8 -> 4 -> 2), bit for bit
    the split-2 launch of the large context; the forward refuses, writes nothing, and its next split launch is right."""
    from radnet_hip import lib as L
    small = L.Context(0)
    for name in BWD_WS:
        cs, pr = E.CASES[name], _Problem(ctx, name)
        mode = cs.opts.get("modes", (0,))[0]
        assert E.geometry(cs)["nrt"] >= 8
        need2, need4 = _slab_bytes(ctx, cs, 2), _slab_bytes(ctx, cs, 4)
        ws = torch.empty(need2, dtype=torch.uint8, device="cuda")
        assert need2 < need4
        small.check(small.lib.radnet_set_workspace(small.h, ws.data_ptr(), need2), "set_workspace")
        rc, want = pr.launch(ctx, 2, mode)
        ctx.check(rc, name)
        rc, one = pr.launch(ctx, 1, mode)
        ctx.check(rc, name)
        assert not np.array_equal(want, one), "split 2 and one pass give the same bits: the comparison below would prove nothing"
        rc, got = pr.launch(small, 8, mode)
        assert rc == 0, (name, rc)
        _check(name, got, mode, 8)
        assert np.array_equal(got, want), (name, "not the bits of split 2")
    cs, pr = E.CASES[FWD_WS], _Problem(ctx, FWD_WS)
    nrt = E.geometry(cs)["nrt"]
    need2 = _slab_bytes(ctx, cs, 2)
    ws = torch.empty(need2, dtype=torch.uint8, device="cuda")
    small.check(small.lib.radnet_set_workspace(small.h, ws.data_ptr(), need2), "set_workspace")
    rc, got = pr.launch(small, nrt)
    assert rc < 0 and (got == E.SENTINEL).all(), (rc, "a refused forward wrote to its output")
    rc, want = pr.launch(ctx, 2)
    ctx.check(rc, FWD_WS)
    rc, got = pr.launch(small, 2)
    assert rc == 0
    _check(FWD_WS, got, 0, 2)
    assert np.array_equal(got, want)
    small.close()


def test_no_workspace_backward_runs_one_pass_forward_refuses(ctx):
    from radnet_hip import lib as L
    bare = L.Context(0)                                  # radnet_set_workspace is never called before the backward launches
    for name in BWD_WS:
        cs, pr = E.CASES[name], _Problem(ctx, name)
        mode = cs.opts.get("modes", (0,))[0]
        rc, want = pr.launch(ctx, 0, mode, plain=True)
        ctx.check(rc, name)
        rc, got = pr.launch(bare, 8, mode)
        assert rc == 0, (name, rc)
        _check(name, got, mode, 8)
        assert np.array_equal(got, want), (name, "not the bits of the unsplit launch")
    pr = _Problem(ctx, FWD_WS)
    rc, got = pr.launch(bare, 2)
    assert rc < 0 and (got == E.SENTINEL).all(), (rc, "a refused forward wrote to its output")
    # no counter was touched: with a workspace the same context's split launch is the large context's, bit for bit
    ws = torch.empty(_slab_bytes(ctx, E.CASES[FWD_WS], 2), dtype=torch.uint8, device="cuda")
    bare.check(bare.lib.radnet_set_workspace(bare.h, ws.data_ptr(), ws.numel()), "set_workspace")
    rc, want = pr.launch(ctx, 2)
    ctx.check(rc, FWD_WS)
    rc, got = pr.launch(bare, 2)
    assert rc == 0
    _check(FWD_WS, got, 0, 2)
    assert np.array_equal(got, want)
    bare.close()
