"""Shared tables, launch-plan model, float64 references and arena layouts of the edge tests of radnet_conv_wgrad_multi (csrc/conv_wgrad.hip,
csrc/wgrad_multi_plan.cpp), of its Adam epilogue (conv_wgrad_body.h, OPT = true) and of radnet_adam_step_tail (csrc/adam.hip).  Device-free
check of the tables, the model, the references and their teeth: tests/test_wgrad_multi_cases_reference.py; the kernels:
tests/test_gpu_wgrad_multi_edges.py.  NumPy only: no torch, no library.

Nothing is derived here that another suite derives already:
  problems  the weight-gradient cases of fp32_edge_cases.py BY NAME -- its inputs, its pitches, `compute(name, "wgrad", mode)` and its
            per-element bound (M + 8) 2^-24 sum|a b| (+ the old dw in mode 1).  A problem may take a COLUMN BLOCK [c0, c0 + n') of its case
            (dy + c0 with the case's pitch, gscale + c0): reference and bound are the same columns of the case's.
  Adam      update_edge_cases.adam_refs / adam_state / STEPS_FOUR: p, m, v against float64 Adam of the gradient the DEVICE computed (the
            ordered slice reduction makes the epilogue's gradient the bits of a gradients-only call), so tol_p, tol_m, tol_v hold as they are.
  tail      update_edge_cases.ref_shift / ref_wino / gap_table, of the device's own p.

A TABLE is one radnet_conv_wgrad_multi call: entries (case, mode, db present, pinned launch shape or None, dy all zero, column block) and the
workspace the context holds.  `launch_shape` models run_wgrad's choice for an entry on a context without autotuning (a loaded tuning-table
line, else the default branch; then the halving fallback when the ordered slabs exceed the workspace), `plan` is wgrad_multi_plan.  Every
table states what it is there for in CLAIMS -- launches, which problems split and into how many slices -- and the CPU test holds the model
to it; the GPU test holds the device's launch count to the model.

Optimizer layout of a table (modes 0 and 2): the problems' dw blocks [K][ldw] lie in one arena in table order with GAPS[i % 3] floats in
front of block i -- pad columns inside the arena -- then a bias range and a dense block that the call must not touch, then TAIL sentinels.

Tail layouts: radnet_adam_step_tail sweeps [sweep_from, n) and transforms the listed layers, all in front of sweep_from, from the weights as
they are.  What lies in front of sweep_from keeps its bits in p, g, m, v."""
import collections
import functools

import numpy as np

import fp32_edge_cases as P
import update_edge_cases as E

U, SENTINEL, TAIL, F = E.U, E.SENTINEL, E.TAIL, E.F
assert P.SENTINEL == SENTINEL
K_MULTI_MAX = 16                          # kWgradMultiMax (csrc/conv_args.h)
COUNTER_CAP = 65536                       # kAuxWgradCounterCount (csrc/radnet_internal.h)
NUM_CU = 256                              # kNumCU (csrc/conv_args.h)
WS_BIG = 64 << 20

PROBLEMS = ("w_ragged_db", "w_m1", "w_s2_3x3", "w_s2_1x1", "w_pad_br", "w_1x3", "w_3x1_s2", "w_deep_m", "b_3x3", "b_1x1")
assert all("wgrad" in P.sides(P.CASES[n]) for n in PROBLEMS)

Entry = collections.namedtuple("Entry", "case mode db pin zero cols")
Table = collections.namedtuple("Table", "name entries ws")


def entry(case, mode=0, db=True, pin=None, zero=False, cols=None):
    assert case in PROBLEMS and mode in (0, 1, 2) and not (zero and mode == 1)
    return Entry(case, mode, db, pin, zero, cols)


def cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def dims(e):
    """M, K, N (the block's columns), c, taps, stride, reduction tiles of 32 rows, first column, pitches of the entry's own buffers."""
    cs = P.CASES[e.case]
    g = P.geometry(cs, "wgrad")
    c0, n = e.cols if e.cols else (0, cs.n)
    assert c0 % 4 == 0 and n % 4 == 0 and 0 < n and c0 + n <= cs.n
    return dict(M=g["M"], K=g["K"], N=n, c=cs.c, taps=cs.kh * cs.kw, stride=cs.stride, nmt=cdiv(g["M"], 32), c0=c0, ldw=n + 4, ld_db=n + 8,
                ld_dy=P.pitches(cs)["ld_dy"])


# ---------------------------------------------------------------------------------------------------------------- the launch policy
def default_shape(c, K, N, nmt):
    """run_wgrad's last branch: no forced shape, no table entry, no autotuning."""
    bmk, bn, s = (128 if c % 128 == 0 else 64), (128 if N > 64 else 64), 1
    tiles = cdiv(K, bmk) * cdiv(N, bn)
    if tiles < NUM_CU and bmk == 128 and bn == 128:
        bn = 64
        tiles = cdiv(K, bmk) * cdiv(N, bn)
    while tiles * s < 2 * NUM_CU and nmt // (s * 2) >= 4 and s < 16:
        s *= 2
    return bmk, bn, s


def slab_bytes(K, N, bmk, bn, s):
    """Ordered reduction: the partial tiles and the bias partials of every slice."""
    wx, wy = cdiv(K, bmk), cdiv(N, bn)
    return (wx * wy * s * bmk * bn + wy * s * bn) * 4


def launch_shape(e, ws_bytes, ordered=True):
    """-> dict(bmk, bn, slices, wx, wy, slab_bytes, counters): what the entry's own radnet_conv_wgrad call would launch."""
    d = dims(e)
    bmk, bn, s = e.pin if e.pin else default_shape(d["c"], d["K"], d["N"], d["nmt"])
    assert d["c"] % bmk == 0 and (s == 1 or d["nmt"] // s >= 1), (e, "a pin the fp32 suite's rules leave out")
    wx, wy = cdiv(d["K"], bmk), cdiv(d["N"], bn)
    fits = lambda k: wx * wy <= COUNTER_CAP and ws_bytes > 0 and slab_bytes(d["K"], d["N"], bmk, bn, k) <= ws_bytes
    while ordered and s > 1 and not fits(s):          # the halving fallback of run_wgrad
        s = s // 2 if s > 2 else 1
        while s > 1 and cdiv(d["nmt"], cdiv(d["nmt"], s)) != s:
            s -= 1
    split = ordered and s > 1
    return dict(bmk=bmk, bn=bn, slices=s, wx=wx, wy=wy, slab_bytes=slab_bytes(d["K"], d["N"], bmk, bn, s) if split else 0,
                counters=wx * wy if split else 0)


def plan(entries, ws_bytes, ordered=True):
    """wgrad_multi_plan: -> [dict(bmk, bn, problems, slab_off, counter_off, first)] in launch order."""
    items = [launch_shape(e, ws_bytes, ordered) for e in entries]
    out = []
    for first in range(len(items)):
        shape = (items[first]["bmk"], items[first]["bn"])
        if any((it["bmk"], it["bn"]) == shape for it in items[:first]):
            continue
        cur = None
        for i in range(first, len(items)):
            it = items[i]
            if (it["bmk"], it["bn"]) != shape:
                continue
            if cur is not None and (len(cur["problems"]) == K_MULTI_MAX or cur["slab_at"] + it["slab_bytes"] > ws_bytes or
                                    cur["ctr_at"] + it["counters"] > COUNTER_CAP):
                cur = None
            if cur is None:
                cur = dict(bmk=shape[0], bn=shape[1], problems=[], slab_off=[], counter_off=[], first=[], slab_at=0, ctr_at=0, grid=0)
                out.append(cur)
            cur["problems"].append(i)
            cur["slab_off"].append(cur["slab_at"])
            cur["counter_off"].append(cur["ctr_at"])
            cur["first"].append(cur["grid"])
            cur["grid"] += it["wx"] * it["wy"] * it["slices"]
            cur["slab_at"] = (cur["slab_at"] + it["slab_bytes"] + 255) & ~255
            cur["ctr_at"] += it["counters"]
    return out


def pin_lines(entries):
    """Tuning-table lines `kind M N K C npos stride a b slices ms waves` of the pinned entries: kind 2, kind 3 in mode 1."""
    lines = {}
    for e in entries:
        if e.pin:
            key = (3 if e.mode == 1 else 2,) + _shape_key(e)
            assert lines.setdefault(key, e.pin) == e.pin, (e, "two pins for one shape")
    return ["%d %d %d %d %d %d %d %d %d %d 0.01 4" % (k + v) for k, v in sorted(lines.items())]


def _shape_key(e):
    d = dims(e)
    return d["M"], d["N"], d["K"], d["c"], d["taps"], d["stride"]


def unpinned_hits_a_pin(entries):
    """An entry without a pin whose shape another entry of the table pins (the default branch reads the kind-2 line): the tables have none."""
    pinned = {_shape_key(e) for e in entries if e.pin}
    return [e for e in entries if not e.pin and _shape_key(e) in pinned]


TABLE_HEADER = "# radnet tuned GEMM launch shapes v2\n"

# ---------------------------------------------------------------------------------------------------------------- the tables
_S = (64, 64)
_SEVENTEEN_CYCLE = ("w_s2_3x3", "w_pad_br", "w_1x3", "w_ragged_db")          # M = 84, 84, 90, 135: two slices of 32-row tiles each
_TABLES = [
    # the policy's own choice: 64x64 (seven problems), 64x128 (w_ragged_db), 128x64 (w_s2_1x1, w_1x3 -- the policy narrows a 128x128 tile
    # whose grid leaves CUs idle, so that shape is reached by the pinned table only); w_deep_m splits into 8
    Table("all_default", (entry("w_m1"), entry("w_ragged_db"), entry("w_s2_3x3", db=False), entry("w_s2_1x1"), entry("w_pad_br"),
                          entry("w_deep_m"), entry("w_1x3", db=False), entry("w_3x1_s2"), entry("b_3x3"), entry("b_1x1", mode=2)), WS_BIG),
    # four tile shapes; the 64x64 launch holds slices 1, 2, 3, 8, 1, 2 in that order
    Table("pinned_mixed", (entry("w_m1", pin=_S + (1,)), entry("w_ragged_db", mode=2, pin=(64, 128, 2)), entry("b_1x1", pin=_S + (2,)),
                           entry("w_s2_1x1", pin=(128, 128, 2)), entry("b_3x3", mode=2, pin=_S + (3,)), entry("w_1x3", pin=(128, 64, 3), db=False),
                           entry("w_deep_m", pin=_S + (8,)), entry("w_pad_br", mode=2, pin=(64, 128, 1), db=False),
                           entry("w_3x1_s2", pin=_S + (1,)), entry("w_s2_3x3", mode=2, pin=_S + (2,))), WS_BIG),
    Table("seventeen", tuple(entry(_SEVENTEEN_CYCLE[i % 4], mode=(0, 2)[i % 2], pin=_S + (2,)) for i in range(17)), WS_BIG),
    # slabs: b_1x1 33,280 bytes, w_ragged_db (two n tiles) 66,560: either fits 80,000 bytes, both do not
    Table("tight_two", (entry("b_1x1", pin=_S + (2,)), entry("w_ragged_db", pin=_S + (2,)), entry("w_m1")), 80000),
    # w_deep_m at 8 slices: 133,120 bytes; at 4: 66,560, beside b_1x1's 33,280 in 100,000
    Table("tight_halving", (entry("w_deep_m"), entry("b_1x1", mode=2, pin=_S + (2,))), 100000),
    Table("no_workspace", (entry("w_deep_m"), entry("b_3x3", mode=2, pin=_S + (3,)), entry("w_ragged_db")), 0),
    Table("one", (entry("w_ragged_db"),), WS_BIG),
    # one x, one geometry, one cached row table; dy + 16 columns and n = 20 in the second problem
    Table("shared_x", (entry("w_s2_3x3"), entry("w_s2_3x3", mode=2, cols=(16, 20))), WS_BIG),
    Table("zero_live", (entry("b_3x3", zero=True, pin=_S + (3,)), entry("w_s2_3x3", mode=2), entry("w_deep_m")), WS_BIG),
    # write mode 2 throughout (the engine's): also the table of the autotuning and of the refusal tests
    Table("mode2_three", (entry("w_s2_1x1", mode=2), entry("w_deep_m", mode=2), entry("b_3x3", mode=2)), WS_BIG),
    Table("modes", (entry("w_ragged_db", mode=1), entry("w_m1", db=False), entry("w_s2_3x3", mode=2), entry("w_1x3", mode=1, pin=(128, 64, 2), db=False),
                    entry("w_deep_m", mode=1), entry("b_3x3", mode=2, db=False), entry("b_1x1", pin=_S + (2,))), WS_BIG),
]
TABLES = collections.OrderedDict((t.name, t) for t in _TABLES)
assert len(TABLES) == len(_TABLES)
# name -> (launches, {index of a split problem: slices}) with ordered reductions
CLAIMS = {
    "all_default": (3, {5: 8}),
    "pinned_mixed": (4, {1: 2, 2: 2, 3: 2, 4: 3, 5: 3, 6: 8, 9: 2}),
    "seventeen": (2, {i: 2 for i in range(17)}),
    "tight_two": (2, {0: 2, 1: 2}),
    "tight_halving": (1, {0: 4, 1: 2}),
    "no_workspace": (2, {}),
    "one": (1, {}),
    "shared_x": (1, {}),
    "zero_live": (1, {0: 3, 2: 8}),
    "mode2_three": (2, {1: 8}),
    "modes": (3, {3: 2, 4: 8, 6: 2}),
}
OPT_TABLES = tuple(n for n, t in TABLES.items() if all(e.mode != 1 for e in t.entries))


# ---------------------------------------------------------------------------------------------------------------- gradients
@functools.lru_cache(maxsize=None)
def problem_inputs(e):
    """What the entry's descriptor points at: x, dy [M][ld_dy] (NaN padding; its first column is c0), gscale, the old dw / db of mode 1."""
    cs, d, dm = P.CASES[e.case], P.inputs(e.case), dims(e)
    c0, n = dm["c0"], dm["N"]
    dy = P.padded(np.zeros_like(d["dy"]) if e.zero else d["dy"], dm["ld_dy"])
    return E._frozen(dict(x=d["x"], dy=dy, gscale=None if d["gscale"] is None else np.ascontiguousarray(d["gscale"][c0:c0 + n]),
                          dw0=np.ascontiguousarray(d["dw0"][:, c0:c0 + n]), db0=np.ascontiguousarray(d["db0"][c0:c0 + n])))


MUTANTS = ("neighbour_dy", "db_added_in_mode0", "seventeenth_dropped", "dense_pitch", "pad_stepped", "tail_sweeps_from_0",
           "tail_steps_a_layer", "wino_from_old_p", "shift_from_old_p", "front_gap_swept")


@functools.lru_cache(maxsize=None)
def problem_ref(e):
    """dict(out [K][N], tol, db [N], db_tol) in float64: the entry's columns of fp32_edge_cases.compute."""
    r, dm = P.compute(e.case, "wgrad", e.mode), dims(e)
    sl = slice(dm["c0"], dm["c0"] + dm["N"])
    if e.zero:                                                                  # every product is a zero: the sums are exact
        z = np.zeros((dm["K"], dm["N"]))
        return E._frozen(dict(out=z, tol=z, db=np.zeros(dm["N"]), db_tol=np.zeros(dm["N"])))
    return E._frozen(dict(out=r["out"][:, sl], tol=r["tol"][:, sl], db=r["db"][sl], db_tol=r["db_tol"][sl]))


def table_refs(table, mut=None):
    """[dict(out, tol, db, db_tol)] per entry.  Mutants: `neighbour_dy` -- problem k > 0 reads problem k - 1's dy and gscale pointers (its own
    n and x); `db_added_in_mode0` -- db keeps what the buffer held (the mode-1 old values stand in for it); `seventeenth_dropped` -- the
    problem behind the sixteenth of a launch is never run: NaN, the sentinel, stays."""
    refs = [dict(problem_ref(e)) for e in table.entries]
    if mut == "neighbour_dy":
        for k in range(1, len(refs)):
            e, prev = table.entries[k], table.entries[k - 1]
            assert e.case == prev.case and dims(prev)["c0"] + dims(e)["N"] <= P.CASES[e.case].n
            r = P.compute(e.case, "wgrad", e.mode)
            sl = slice(dims(prev)["c0"], dims(prev)["c0"] + dims(e)["N"])
            refs[k].update(out=r["out"][:, sl], db=r["db"][sl])
    if mut == "db_added_in_mode0":
        for k, e in enumerate(table.entries):
            if e.mode == 0 and e.db:
                refs[k]["db"] = refs[k]["db"] + problem_inputs(e)["db0"]
    if mut == "seventeenth_dropped":
        shapes = [(s["bmk"], s["bn"]) for s in (launch_shape(e, table.ws) for e in table.entries)]
        for shape in set(shapes):
            for k in [i for i, s in enumerate(shapes) if s == shape][K_MULTI_MAX:]:
                refs[k].update(out=np.full_like(refs[k]["out"], np.nan), db=np.full_like(refs[k]["db"], np.nan))
    return refs


def loop_ref(e):
    """The same numbers from the definition, one multiply-add at a time (the CPU test runs it on the two smallest problems)."""
    cs, inp, dm = P.CASES[e.case], problem_inputs(e), dims(e)
    g = P.geometry(cs, "wgrad")
    x, dy = inp["x"], inp["dy"]
    dw, db = np.zeros((dm["K"], dm["N"])), np.zeros(dm["N"])
    for m in range(dm["M"]):
        img, r = divmod(m, g["oh"] * g["ow"])
        oy, ox = divmod(r, g["ow"])
        gm = [float(dy[m, dm["c0"] + j] * inp["gscale"][j]) if inp["gscale"] is not None else float(dy[m, dm["c0"] + j]) for j in range(dm["N"])]
        for j in range(dm["N"]):
            db[j] += gm[j]
        for ky in range(cs.kh):
            for kx in range(cs.kw):
                iy, ix = oy * cs.stride - cs.pad[0] + ky, ox * cs.stride - cs.pad[1] + kx
                if not (0 <= iy < cs.h and 0 <= ix < cs.w):
                    continue
                for ch in range(cs.c):
                    a = float(x[img, iy, ix, ch])
                    row = dw[(ky * cs.kw + kx) * cs.c + ch]
                    for j in range(dm["N"]):
                        row[j] += a * gm[j]
    if e.mode == 1:
        dw, db = dw + inp["dw0"], db + inp["db0"]
    return dw, db


# ---------------------------------------------------------------------------------------------------------------- the optimizer layout
GAPS = (0, 4, 1028)
OPT_BIAS_LEN, OPT_DENSE_LEN = 64, 256
OPT_STATES = ("random", "zero_moments")
# (t, grad_scale) of the two consecutive steps per state
OPT_STEPS = {"random": E.STEPS_FOUR[:2], "zero_moments": E.STEPS_FOUR[2:]}
Arena = collections.namedtuple("Arena", "n offs bias dense")


@functools.lru_cache(maxsize=None)
def arena_of(name):
    """Where the table's dw blocks lie: offs[i] = float offset of block i ([K][ldw], its pad columns and its last row's too)."""
    offs, at = [], 0
    for i, e in enumerate(TABLES[name].entries):
        at += GAPS[i % 3]
        offs.append(at)
        at += dims(e)["K"] * dims(e)["ldw"]
    return Arena(at + OPT_BIAS_LEN + OPT_DENSE_LEN, tuple(offs), (at, OPT_BIAS_LEN), (at + OPT_BIAS_LEN, OPT_DENSE_LEN))


@functools.lru_cache(maxsize=None)
def layer_index(name, pitch="own"):
    """Arena indices of the elements (k < K, j < n) of every block, block after block, row-major.  pitch = "dense": where an epilogue that
    addresses p with pitch n instead of ldw would put them (a mutant)."""
    ar, idx = arena_of(name), []
    for e, off in zip(TABLES[name].entries, ar.offs):
        d = dims(e)
        ld = d["ldw"] if pitch == "own" else d["N"]
        idx.append((off + np.arange(d["K"])[:, None] * ld + np.arange(d["N"])[None, :]).ravel())
    out = np.concatenate(idx)
    out.setflags(write=False)
    return out


def pad_index(name):
    """Arena indices of the pad columns (k < K - 1 or any k, n <= j < ldw) of every block."""
    ar, idx = arena_of(name), []
    for e, off in zip(TABLES[name].entries, ar.offs):
        d = dims(e)
        idx.append((off + np.arange(d["K"])[:, None] * d["ldw"] + np.arange(d["N"], d["ldw"])[None, :]).ravel())
    return np.concatenate(idx)


def opt_state(name, which):
    """fp32 p, m, v of the table's arena (no TAIL): update_edge_cases.adam_state, or its p with m = v = 0."""
    st = E.adam_state(arena_of(name).n)
    if which == "zero_moments":
        z = np.zeros(arena_of(name).n, F)
        return dict(p=st["p"], m=z, v=z)
    assert which == "random"
    return dict(p=st["p"], m=st["m"], v=st["v"])


def grads_flat(name, grads):
    """The per-entry [K][N] gradients (fp32, as the device gave them) in `layer_index` order."""
    return np.concatenate([np.asarray(g, F).reshape(-1) for g in grads])


def reference_grads(name):
    """The float64 gradients rounded to fp32: what the device-free checks use where the GPU test uses the device's own gradient."""
    return [problem_ref(e)["out"].astype(F) for e in TABLES[name].entries]


def epilogue_refs(name, state, grads, t, gs, mut=None):
    """-> {p, m, v: dict(prefill [n + TAIL] uint32 bits, inside, ref, tol)}: float64 Adam of `grads` at the blocks' elements, the old bits
    everywhere else.  Mutants: `dense_pitch` -- the new values land where pitch n puts them; `pad_stepped` -- the pad columns take a step
    with a zero gradient."""
    ar = arena_of(name)
    idx = layer_index(name)
    r = E.adam_refs(state["p"][idx], grads_flat(name, grads), state["m"][idx], state["v"][idx], t, gs)
    out = {}
    for k in "pmv":
        full = _arena(state[k], idx, r[k]["buf"][:idx.size], r[k]["tol"][:idx.size])
        if mut == "dense_pitch":
            m = state[k].astype(np.float64)
            m[layer_index(name, "dense")] = r[k]["buf"][:idx.size]
            full["mutant"] = m
        if mut == "pad_stepped":
            pad = pad_index(name)
            rp = E.adam_refs(state["p"][pad], np.zeros(pad.size, F), state["m"][pad], state["v"][pad], t, gs)
            m = np.where(full["inside"][:ar.n], full["ref"][:ar.n], state[k].astype(np.float64))
            m[pad] = rp[k]["buf"][:pad.size]
            full["mutant"] = m
        out[k] = full
    return out


def _arena(old, idx, ref, tol, zero_idx=None):
    """A full arena buffer: `old` fp32 [n] then TAIL sentinels; the elements `idx` must come within `tol` of `ref`, the elements `zero_idx`
    must be +0.0, every other one keeps its bits."""
    n = old.size
    prefill = np.concatenate([np.ascontiguousarray(old, F).view(np.uint32), np.full(TAIL, SENTINEL, np.uint32)])
    inside, zero = np.zeros(n + TAIL, bool), np.zeros(n + TAIL, bool)
    full_ref, full_tol = np.zeros(n + TAIL), np.zeros(n + TAIL)
    inside[idx] = True
    full_ref[idx], full_tol[idx] = ref, tol
    if zero_idx is not None:
        zero[zero_idx] = True
    return dict(prefill=prefill, inside=inside, ref=full_ref, tol=full_tol, zero=zero)


def verdict(res, got):
    """(elements outside their bound or no longer holding their bits, worst err / tol) of a full buffer `got` (fp32 or float64 values;
    NaN where the prefill is a NaN) -- the device-free twin of the GPU test's judge."""
    got = np.asarray(got)
    k = got.size
    ins, zero = res["inside"][:k], res["zero"][:k]
    g64 = got.astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = np.where(ins, np.abs(g64 - res["ref"][:k]), 0.0)
        bad = ins & ~(err <= res["tol"][:k])
        old = res["prefill"][:k].view(F).astype(np.float64)
        kept = (g64 == old) | (np.isnan(g64) & np.isnan(old))
        bad |= ~ins & ~zero & ~kept
        bad |= zero & ~(g64 == 0)
        ratio = np.where(err > 0, err / np.where(res["tol"][:k] > 0, res["tol"][:k], 1e-300), 0.0)
    return int(bad.sum()), float(np.nan_to_num(ratio, nan=np.inf).max()) if k else 0.0


# ---------------------------------------------------------------------------------------------------------------- the tail layouts
TailLayout = collections.namedtuple("TailLayout", "name n wino bias sweep_from steps")
_UNIT = 2304                              # floats of a [3][3][c][n] layer with c * n = 256
_CN = ((16, 16), (64, 4), (4, 64), (8, 32), (32, 8), (16, 16), (4, 64))


def _layers(gaps):
    """Layers of _UNIT floats with gaps[i] floats in front of layer i -> (layers, the end of the last one)."""
    out, at = [], 0
    for i, gap in enumerate(gaps):
        at += gap
        out.append((at,) + _CN[i % len(_CN)])
        at += _UNIT
    return tuple(out), at


def _tail(name, gaps, behind, sweep_len, bias, steps=None):
    """bias: "start", "middle", "end" (of the sweep) or None; behind: floats between the last layer and sweep_from."""
    wino, end = _layers(gaps)
    sweep_from = end + behind
    n = sweep_from + sweep_len
    at = dict(start=sweep_from, middle=sweep_from + (sweep_len // 2) // 4 * 4, end=n - 128).get(bias)
    return TailLayout(name, n, wino, None if bias is None else (at, 128), sweep_from, steps or E.STEPS_FOUR)


OVER_SWEEP = 4 * (E.SWEEP_CAP + 192)      # the whole excess over one pass of the flat sweep lies behind sweep_from
_TAILS = [
    _tail("one_layer_gaps", (512,), 256, 1024, "start"),
    _tail("three_gaps", (4, 1028, 512), 8, 1500, "middle"),
    _tail("three_adjacent_to_sweep", (0, 0, 0), 0, 1024, "end"),                # adjacent layers, the last ends exactly at sweep_from
    _tail("three_mixed", (256, 0, 4), 0, 640, "start"),
    _tail("seven_gaps", (4, 8, 1028, 4, 256, 12, 516), 260, 2048, "end"),       # 7 layers + 8 front ranges: 15 of the table's 16 ranges
    _tail("seven_adjacent", (0,) * 7, 0, 512, "middle"),
    _tail("sweep_at_n", (512,), 256, 0, None),                                  # nothing to sweep, no shift: the transforms alone
    _tail("over_cap", (0,), 256, OVER_SWEEP, "end", steps=E.STEPS_ONE),         # the bias range lies where only the second pass reaches
]
TAILS = collections.OrderedDict((t.name, t) for t in _TAILS)
assert len(TAILS) == len(_TAILS)
GAP_RANGES_MAX = 16                       # adam_fused refuses a front range when the table already holds 16 (kAdamGapMax = 17 gaps)


def tail_ranges(lay):
    """The ranges the tail's sweep leaves out, in arena order: the listed layers and every stretch in front of sweep_from between them."""
    out, at = [], 0
    for off, c, n in sorted(lay.wino) + [(lay.sweep_from, 0, 0)]:
        if off > at:
            out.append((at, off - at))
        if c:
            out.append((off, 9 * c * n))
        at = off + 9 * c * n
    return out


def tail_violations(lay):
    """What radnet_adam_step_tail's host checks refuse, as a list of strings (empty: inside the contract)."""
    bad = []
    if lay.sweep_from <= 0:
        bad.append("sweep_from must be positive")
    if lay.bias and lay.bias[0] < lay.sweep_from:
        bad.append("bias range in front of the sweep")
    if len(lay.wino) > E.WINO_MAX:
        bad.append("more than 12 layers")
    bad += ["layer %d" % off for off, c, n in lay.wino if c <= 0 or n <= 0 or n % 4 or (c * n // 4) % 64 or off % 4]
    if lay.sweep_from % 4 or lay.sweep_from > lay.n:
        bad.append("sweep_from must be a multiple of 4 inside the arena")
    at, nr = 0, len(lay.wino)
    for off, c, n in sorted(lay.wino) + [(lay.sweep_from, 0, 0)]:
        if c and (off < at or off + 9 * c * n > lay.sweep_from):
            bad.append("layer at %d overlaps another or reaches past sweep_from" % off)
        if off > at:
            if nr + 1 > GAP_RANGES_MAX:
                bad.append("too many layers for the gap table")
            nr += 1
        at = off + 9 * c * n
    if lay.n % 4 or (lay.bias and (lay.bias[0] % 4 or lay.bias[1] % 4 or lay.bias[0] + lay.bias[1] > lay.n)):
        bad.append("arena length / bias range")
    return bad


_BASE = TAILS["three_gaps"]
# name -> (the layout, a fragment of the message)
TAIL_REFUSALS = collections.OrderedDict([
    ("eight_layers_nine_gaps", (_tail("r", (4,) * 8, 4, 256, "start"), "too many layers for the gap table")),
    ("sweep_from_0", (_BASE._replace(sweep_from=0, bias=None), "sweep_from must be positive")),
    ("sweep_from_not_multiple_of_4", (_BASE._replace(sweep_from=_BASE.sweep_from + 2), "multiple of 4")),
    ("sweep_from_past_n", (_BASE._replace(sweep_from=_BASE.n + 4, bias=None), "inside the arena")),
    ("layer_past_sweep_from", (_BASE._replace(sweep_from=_BASE.wino[2][0] + 64, bias=None), "reaches past sweep_from")),
    ("bias_in_front_of_sweep_from", (_BASE._replace(bias=(_BASE.wino[1][0] + _UNIT, 128)), "bias range starts in front")),
])


@functools.lru_cache(maxsize=None)
def tail_state(name):
    lay = TAILS[name] if name in TAILS else TAIL_REFUSALS[name][0]
    return E.adam_state(lay.n)


def tail_refs(lay, state, t, gs, zero_grad, mut=None):
    """-> {p, m, v, g: the `_arena` dicts}: float64 Adam on [sweep_from, n), the old bits in front of it.  Mutants (their `mutant` entry is
    the full float64 buffer a tail with the defect would leave): `tail_sweeps_from_0` steps everything that is no listed layer,
    `front_gap_swept` the first stretch in front of sweep_from that is no layer, `tail_steps_a_layer` the first listed layer."""
    sw = np.arange(lay.sweep_from, lay.n)
    r = E.adam_refs(state["p"][sw], state["g"][sw], state["m"][sw], state["v"][sw], t, gs)
    out = {k: _arena(state[k], sw, r[k]["buf"][:sw.size], r[k]["tol"][:sw.size]) for k in "pmv"}
    out["g"] = _arena(state["g"], sw, np.zeros(sw.size), np.zeros(sw.size), zero_idx=sw) if zero_grad else _arena(state["g"], sw[:0], [], [])
    if mut in ("tail_sweeps_from_0", "front_gap_swept", "tail_steps_a_layer"):
        ranges = [(off, ln) for off, ln in tail_ranges(lay) if ((off, ln) in [(o, 9 * c * n) for o, c, n in lay.wino]) == (mut == "tail_steps_a_layer")]
        assert ranges, (lay.name, mut, "needs a range of that kind")
        if mut != "tail_sweeps_from_0":
            ranges = ranges[:1]
        extra = np.concatenate([np.arange(off, off + ln) for off, ln in ranges])
        rx = E.adam_refs(state["p"][extra], state["g"][extra], state["m"][extra], state["v"][extra], t, gs)
        for k in "pmv":
            m = np.where(out[k]["inside"][:lay.n], out[k]["ref"][:lay.n], state[k].astype(np.float64))
            m[extra] = rx[k]["buf"][:extra.size]
            out[k]["mutant"] = m
    return out
