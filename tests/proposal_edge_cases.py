"""Shared case tables, input builders, expected output buffers, branch tallies and NumPy kernel models of the edge tests of the fp64 glue
kernels: csrc/proposals.hip (radnet_nms, radnet_rpn_to_roi on both of its paths) and csrc/targets.hip (radnet_anchor_targets,
radnet_anchor_targets_pack, radnet_roi_targets, radnet_roi_batch_pack).  Device-free check of the tables, the models and their teeth:
tests/test_proposal_edge_cases_reference.py; the kernels: tests/test_gpu_proposal_edges.py.  NumPy and `oracle` only: no torch, no library.

Reference.  Every expected value comes from oracle/glue.py (greedy_nms, decode_all_anchors, rpn_to_roi, anchor_targets_dense,
to_train_layout, roi_targets), which tests/test_oracle_glue.py pins to the reference's own outputs.  The tie rule of greedy_nms -- stable
ascending sort walked from the end: among equal scores the higher index first, -0.0 equal to +0.0 -- is part of the reference.  Where the
reference asserts (a malformed box in NMS) the kernels' stated answer is count -1; where a decoded box has a non-finite coordinate (the
reference asserts as well) the stated answer is the oracle's result with exactly those boxes removed.

Comparison.  Bit for bit, except the components that pass through `log` (tw, th of the anchor and RoI regression targets), which carry
the tolerances tests/test_gpu_kernels.py states for these kernels: 4.5e-16 relative in fp64 with the fp32 casts bit-equal.  The pack
kernels are fed the oracle's own arrays here, so their outputs are bit-exact too.

Buffers.  Every `expected_*` function returns {name: Out}: the FULL buffer of an output -- the tensor the entry writes into and TAIL
elements behind it -- as the dtype the entry writes, every byte the contract does not write holding SBYTE, plus the mask of the `log`
components.  A driver prefills with SBYTE, launches once, and judges every element: written ones against the reference, all others against
the sentinel (rows at or past the returned count, the tails, the outputs of a refused call).  No expected value equals a sentinel (checked
by the CPU test).

Tallies.  `*_tally` walk a case with the oracle's own decisions and count the branches it reaches; every case names the branch it is
there for in its `branch` field and REACH maps that name to a predicate on the tally.

Models.  ChunkScan (the 64-candidate chunk scan: 16 waves striding over the pick list, the ballot matrix, the serial resolve), band_bounds
/ model_select (the radix select that cuts bands of at most 4096 keys, inside ties if need be) and model_anchor_targets (the
visiting-order atomicMax key and the fallback in ground-truth order) restate the kernels' schemes; model_roi_targets restates the RoI
labelling.  All must equal the oracle on every case; each mutant named in MUTANTS must differ on at least one."""
import collections
import functools

import numpy as np

from faster_rcnn.config import Config
from oracle import glue

TAIL = 64
SBYTE = 0xA5                              # every byte of every output buffer before a launch
F = np.float32
LOG_RTOL = 4.5e-16                        # tests/test_gpu_kernels.py: device log vs NumPy log, 1 ulp of fp64
STD_SCALING = 4.0
MAX_PICKS = 1024
BAND_CAP = 4096

Out = collections.namedtuple("Out", "buf loose")          # loose: the `log` components (None: everything bit for bit)
PACK_Y2_RTOL = 2e-7                       # tests/test_gpu_kernels.py: the packed fp32 coordinates when t comes from the device's own log

MUTANTS = ("ties_lower_index_first", "suppress_ge", "one_pick_too_many", "pick_slot_skipped", "matrix_lane_lt_j", "alive_not_trimmed",
           "band_cut_drops_tie", "last_best_anchor", "best_anchor_fp64", "fallback_reverse_order", "last_gt_wins_tie", "round_half_away")
# "the matrix without the lane > j restriction" taken literally sets bits at and below row j, which the serial resolve has already
# cleared when it reaches row j: that mutant cannot change a result.  It is kept (EQUIVALENT_MUTANTS) and shown to be equivalent; the one
# with teeth is the restriction turned round (lane < j).
EQUIVALENT_MUTANTS = ("matrix_no_lane_restriction",)


def sentinel(dtype, n):
    return np.full(n * np.dtype(dtype).itemsize, SBYTE, np.uint8).view(dtype)


def _out(dtype, shape, written=None, rows=None, loose=None):
    """Full buffer of an output of `shape`: `written` (array of `shape`, or of the first `rows` rows) where the contract writes."""
    n = int(np.prod(shape))
    buf = sentinel(dtype, n + TAIL)
    lo = np.zeros(n + TAIL, bool)
    if written is not None:
        w = np.ascontiguousarray(written, dtype=dtype).reshape(-1)
        buf[:w.size] = w
        if loose is not None:
            lo[:w.size] = np.asarray(loose, bool).reshape(-1)
    return Out(buf, lo if loose is not None else None)


def _masked(dtype, shape, values, mask):
    """Full buffer with `values` where `mask`, the sentinel elsewhere."""
    n = int(np.prod(shape))
    buf = sentinel(dtype, n + TAIL)
    m = np.asarray(mask, bool).reshape(-1)
    buf[:n][m] = np.asarray(values, dtype).reshape(-1)[m]
    return buf


# =================================================================================================================== NMS
def sortable(probs):
    """The kernels' order-preserving key of an fp32 score, -0.0 as +0.0."""
    u = np.asarray(probs, F).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000 != 0, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def _sup(pb, cb, thr, ge=False):
    """(P, C) suppression matrix of picks pb against candidates cb: rpn.py:429-447, the rounded quotient against thr."""
    pa = (pb[:, 2] - pb[:, 0]) * (pb[:, 3] - pb[:, 1])
    ca = (cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])
    ww = np.maximum(0, np.minimum(pb[:, None, 2], cb[None, :, 2]) - np.maximum(pb[:, None, 0], cb[None, :, 0]))
    hh = np.maximum(0, np.minimum(pb[:, None, 3], cb[None, :, 3]) - np.maximum(pb[:, None, 1], cb[None, :, 1]))
    inter = ww * hh
    ov = inter / (pa[:, None] + ca[None, :] - inter + 1e-6)
    return ov >= thr if ge else ov > thr


def stable_desc(probs, lower_first=False):
    o = np.argsort(np.asarray(probs), kind="stable")[::-1]
    if lower_first:
        o = np.argsort(-np.asarray(probs, np.float64), kind="stable")
    return o


def oracle_picks(boxes, probs, thr, mb):
    """Indices picked by glue.greedy_nms, in pick order: the oracle returns boxes and scores, the indices follow from its order rule (the
    walk from the end of the stable ascending sort): every returned pick is the next candidate in that walk with its box and score."""
    with np.errstate(all="ignore"):
        res = glue.greedy_nms(boxes, probs, overlap_thresh=thr, max_boxes=mb)
    if len(res) == 0:
        return np.zeros(0, np.int64)
    rb, rp = res
    order = stable_desc(probs)
    ib = np.asarray(boxes, np.float64).astype("int")
    picks, r = [], 0
    for b, p in zip(rb, rp):
        while not (np.array_equal(ib[order[r]], b) and F(probs[order[r]]).view(np.uint32) == F(p).view(np.uint32)):
            r += 1
        picks.append(order[r])
        r += 1
    return np.asarray(picks, np.int64)


class ChunkScan:
    """nms_kernel / the scan of select_nms_kernel: candidates arrive in order, 64 at a time; (1) lane = candidate, wave w tests the picks
    p = w, w + 16, ... made before this chunk; (2) mat[j] = the lanes > j that candidate j suppresses; (3) lane 0 resolves the chunk in
    candidate order and appends picks while fewer than max_boxes."""

    def __init__(self, boxes, thr, mb, mutant=None):
        self.boxes, self.thr, self.mb, self.mutant = np.asarray(boxes, np.float64), thr, mb, mutant
        self.picks = []
        self.cand = np.zeros(64, np.int64)                # the LDS slots: what an untrimmed alive mask would read
        self.examined = 0

    def feed(self, order):
        """One sorted run of candidates (the whole list, or one band); -> True when max_boxes is reached."""
        ge = self.mutant == "suppress_ge"
        limit = self.mb + 1 if self.mutant == "one_pick_too_many" else self.mb
        for base in range(0, len(order), 64):
            nc = min(64, len(order) - base)
            self.cand[:nc] = order[base:base + nc]
            cb = self.boxes[self.cand]
            npicks = len(self.picks)
            dead = np.zeros(64, bool)
            if npicks:
                S = _sup(self.boxes[np.asarray(self.picks)], cb, self.thr, ge)
                for wave in range(16):
                    first = wave + 16 if (self.mutant == "pick_slot_skipped" and wave == 5) else wave
                    ps = np.arange(first, npicks, 16)
                    if len(ps):
                        dead |= S[ps].any(0)
            dead[nc:] = False
            M = _sup(cb, cb, self.thr, ge)
            lane, j = np.arange(64)[None, :], np.arange(64)[:, None]
            if self.mutant == "matrix_lane_lt_j":
                M &= lane < j
            elif self.mutant != "matrix_no_lane_restriction":
                M &= lane > j
            M &= (lane < nc) & (j < nc)
            alive = ~dead
            if self.mutant != "alive_not_trimmed":
                alive[nc:] = False
            self.examined += nc
            while alive.any() and len(self.picks) < limit:
                jj = int(np.argmax(alive))
                self.picks.append(int(self.cand[jj]))
                alive &= ~M[jj]
                alive[jj] = False
            if len(self.picks) >= self.mb:
                return True
        return False


def model_nms(boxes, probs, thr, mb, mutant=None):
    keys = (sortable(probs) << np.uint64(32)) | np.arange(len(probs), dtype=np.uint64)
    order = np.argsort(keys, kind="stable")[::-1]
    if mutant == "ties_lower_index_first":
        order = stable_desc(probs, lower_first=True)
    cs = ChunkScan(boxes, thr, mb, mutant)
    cs.feed(order)
    return np.asarray(cs.picks, np.int64)


def _nms_case(name, boxes, probs, thr, mb, branch):
    return dict(name=name, boxes=np.ascontiguousarray(boxes, np.float64).reshape(-1, 4), probs=np.ascontiguousarray(probs, F), thr=float(thr),
                mb=int(mb), branch=branch)


def _deranged_scores(n, rs):
    """Distinct fp32 scores whose rank never equals the index (n > 1)."""
    order = rs.permutation(n)
    while n > 1 and (order == np.arange(n)).any():
        order = np.roll(order, 1)
    probs = np.zeros(n, F)
    probs[order] = (n - np.arange(n)).astype(F) / F(n + 1)
    return probs


def _grid_boxes(n, w=6.0, h=7.0, pitch=10.0, per_row=40, x0=0.0, y0=0.0):
    i = np.arange(n)
    x, y = x0 + pitch * (i % per_row), y0 + pitch * (i // per_row)
    return np.stack([x, y, x + w, y + h], 1)


NMS_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025)


@functools.lru_cache(maxsize=None)
def nms_cases():
    cases = []
    # ---- sizes and stops: disjoint boxes
    for n in NMS_SIZES:
        rs = np.random.RandomState(1000 + n)
        boxes, probs = _grid_boxes(n), _deranged_scores(n, rs)
        for mb in sorted({1, 63, 64, 65, min(n, MAX_PICKS), 1024}):
            if mb > n:
                branch = "stop_never"
            elif mb == n:
                branch = "stop_on_last"
            elif mb % 64 == 0:
                branch = "stop_on_chunk_end"
            else:
                branch = "stop_inside_chunk"
            cases.append(_nms_case("disjoint_n%d_max%d" % (n, mb), boxes, probs, 0.5, mb, branch))
    rs = np.random.RandomState(7)
    # ---- identical boxes
    cases.append(_nms_case("identical_130", np.tile([3.0, 4.0, 20.0, 30.0], (130, 1)), _deranged_scores(130, rs), 0.9, 300, "single_pick"))
    # ---- chain: one box apart holds rank 0, chain position p has rank p + 1 and suppresses only position p + 1: the suppressing pick is
    #      the last candidate of a chunk and its victim the first of the next at ranks 63 | 64, 127 | 128, 191 | 192
    n = 201
    perm = rs.permutation(n)
    pos = np.arange(n - 1)
    chain = np.stack([4.0 * pos, np.zeros(n - 1), 4.0 * pos + 10.0, np.full(n - 1, 5.0)], 1)
    chain = np.concatenate([[[0.0, 50.0, 10.0, 55.0]], chain])
    boxes, probs = np.zeros((n, 4)), np.zeros(n, F)
    boxes[perm], probs[perm] = chain, (n - np.arange(n)).astype(F) / F(n + 1)
    cases.append(_nms_case("chain_200", boxes, probs, 0.3, 300, "chain"))
    # ---- pick slots: 34 top boxes, 150 fillers, 34 near-copies each suppressed by exactly one pick
    top = _grid_boxes(34, w=20.0, h=20.0, pitch=30.0, per_row=34)
    fill = _grid_boxes(150, w=6.0, h=7.0, pitch=10.0, per_row=50, y0=100.0)
    near = top + np.array([1.0, 0.0, 1.0, 0.0])
    boxes = np.concatenate([top, fill, near])
    n = len(boxes)
    rank_scores = (n - np.arange(n)).astype(F) / F(n + 1)
    perm = rs.permutation(n)
    b2, p2 = np.zeros((n, 4)), np.zeros(n, F)
    b2[perm], p2[perm] = boxes, rank_scores
    cases.append(_nms_case("pick_slots", b2, p2, 0.7, 300, "pick_slots"))
    # ---- ties
    n = 150
    x = 3.0 * np.arange(n)
    tie_boxes = np.stack([x, np.zeros(n), x + 10.0, np.full(n, 8.0)], 1)
    cases.append(_nms_case("ties_all_equal", tie_boxes, np.full(n, 0.5, F), 0.5, 300, "ties"))
    cases.append(_nms_case("ties_blocks", tie_boxes[rs.permutation(n)], np.repeat(np.array([0.9, 0.5, 0.5, 0.1, 0.7], F), 30), 0.4, 300, "ties"))
    zeros = np.where(rs.uniform(size=n) < 0.5, F(0.0), F(-0.0)).astype(F)
    zeros[0], zeros[-1] = F(-0.0), F(0.0)
    cases.append(_nms_case("ties_signed_zero", tie_boxes, zeros, 0.5, 300, "signed_zero_tie"))
    cases.append(_nms_case("ties_signed_zero_disjoint", _grid_boxes(70), np.where(np.arange(70) % 3 == 0, F(-0.0), F(0.0)), 0.5, 64, "signed_zero_tie"))
    # ---- threshold: thr = q, just below, just above
    pairs = [np.array([[0.0, 0.0, 10.0, 10.0], [3.0, 1.0, 13.0, 11.0]]), np.array([[0.25, 0.5, 7.75, 9.125], [1.5, 2.25, 8.0, 12.5]]),
             np.array([[0.0, 0.0, 3.0, 3.0], [1.0, 1.0, 4.0, 4.0]]), np.array([[10.0, 10.0, 31.0, 17.0], [12.0, 9.0, 29.0, 19.0]])]
    for k, pb in enumerate(pairs):
        a, b = pb
        inter = max(0.0, min(a[2], b[2]) - max(a[0], b[0])) * max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
        q = inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter + 1e-6)
        pr = np.array([0.9, 0.8], F)
        cases.append(_nms_case("thr_eq_q_%d" % k, pb, pr, q, 300, "thr_margin_keep"))
        cases.append(_nms_case("thr_below_q_%d" % k, pb, pr, np.nextafter(q, 0.0), 300, "thr_margin_kill"))
        cases.append(_nms_case("thr_above_q_%d" % k, pb, pr, np.nextafter(q, 1.0), 300, "thr_margin_keep"))
    touch = np.array([[0.0, 0.0, 5.0, 5.0], [5.0, 0.0, 9.0, 5.0], [0.0, 5.0, 5.0, 9.0]])
    cases.append(_nms_case("thr_zero_touching", touch, np.array([0.3, 0.9, 0.6], F), 0.0, 300, "thr_zero_keep"))
    cases.append(_nms_case("thr_zero_overlapping", touch + np.array([0.0, 0.0, 1.0, 1.0]), np.array([0.3, 0.9, 0.6], F), 0.0, 300, "thr_zero_kill"))
    cases.append(_nms_case("thr_one_identical", np.tile([1.0, 2.0, 9.0, 11.0], (5, 1)), np.array([0.1, 0.5, 0.3, 0.2, 0.4], F), 1.0, 300, "thr_one"))
    frac = rs.uniform(0.0, 30.0, (90, 2))
    fb = np.concatenate([frac, frac + rs.uniform(0.5, 12.0, (90, 2))], 1)
    cases.append(_nms_case("fractional", fb, _deranged_scores(90, rs), 0.35, 300, "fractional"))
    # ---- malformed and empty
    base = _grid_boxes(300)
    for kind, edit in (("x1_eq_x2", lambda b: b.__setitem__(2, b[0])), ("y1_gt_y2", lambda b: b.__setitem__(3, b[1] - 1.0)),
                       ("nan", lambda b: b.__setitem__(1, np.nan))):
        for where in (0, 299, 256 + 17):
            bx = base.copy()
            edit(bx[where])
            cases.append(_nms_case("malformed_%s_at%d" % (kind, where), bx, _deranged_scores(300, rs), 0.5, 64, "malformed"))
    cases.append(_nms_case("empty", np.zeros((0, 4)), np.zeros(0, F), 0.5, 10, "empty"))
    return cases


def nms_expected(case):
    """-> {out_idx, out_count}: count -1 and out_idx untouched where the reference asserts."""
    try:
        picks = oracle_picks(case["boxes"], case["probs"], case["thr"], case["mb"])
        count = len(picks)
    except AssertionError:
        picks, count = None, -1
    return dict(out_idx=_out(np.int32, (case["mb"],), picks), out_count=_out(np.int32, (1,), [count]))


def nms_tally(boxes, probs, thr, mb, order=None):
    """Walk the candidates with the oracle's decisions (rank order, first killer of every suppressed candidate) and count what a chunked
    scan meets on the way.  `order`: the sorted candidate list (default: the stable descending order of probs)."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = len(boxes)
    t = dict(n=n, picks=0, malformed=False, ties=0, signed_zero_ties=0, scan_slots=set(), by_matrix=0, by_scan=0, margin=0, stop="never",
             stop_rank=-1, fractional=bool(n and (boxes != np.floor(boxes)).any()))
    if n == 0:
        return t
    if not (np.all(boxes[:, 0] < boxes[:, 2]) and np.all(boxes[:, 1] < boxes[:, 3])):
        t["malformed"] = True
        return t
    if order is None:
        order = stable_desc(probs)
    p = np.asarray(probs, F)[order]
    t["ties"] = int((p[1:] == p[:-1]).sum())
    t["signed_zero_ties"] = int(((p[1:] == p[:-1]) & (np.signbit(p[1:]) != np.signbit(p[:-1]))).sum())
    alive = np.ones(n, bool)
    pick_rank = []
    for r in range(n):
        if not alive[r]:
            continue
        pick_rank.append(r)
        if len(pick_rank) >= mb:
            t["stop_rank"] = r
            t["stop"] = "on_last" if r == n - 1 else ("on_chunk_end" if r % 64 == 63 else "inside_chunk")
            break
        rest = np.arange(r + 1, n)
        if not len(rest):
            break
        pb, cb = boxes[order[r]][None], boxes[order[rest]]
        kill = _sup(pb, cb, thr)[0]
        # the kernels' margin test: inside it they divide
        pa = (pb[0, 2] - pb[0, 0]) * (pb[0, 3] - pb[0, 1])
        ca = (cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])
        inter = np.maximum(0, np.minimum(pb[0, 2], cb[:, 2]) - np.maximum(pb[0, 0], cb[:, 0])) * np.maximum(0, np.minimum(pb[0, 3], cb[:, 3]) - np.maximum(pb[0, 1], cb[:, 1]))
        d = pa + ca - inter + 1e-6
        tt = thr * d
        t["margin"] += int((alive[rest] & ~(inter > tt * (1.0 + 2.0 ** -40)) & ~(inter < tt * (1.0 - 2.0 ** -40))).sum()) if thr > 0 else int(alive[rest].sum())
        newly = rest[kill & alive[rest]]
        pno = len(pick_rank) - 1
        for v in newly:
            if v // 64 == r // 64:
                t["by_matrix"] += 1
            else:
                t["by_scan"] += 1
                t["scan_slots"].add((pno % 16, pno // 16))
        alive[newly] = False
    t["picks"] = len(pick_rank)
    return t


NMS_REACH = {
    "stop_never": lambda t: t["stop"] == "never" and t["picks"] == t["n"],
    "stop_on_last": lambda t: t["stop"] == "on_last",
    "stop_on_chunk_end": lambda t: t["stop"] == "on_chunk_end",
    "stop_inside_chunk": lambda t: t["stop"] == "inside_chunk",
    "single_pick": lambda t: t["picks"] == 1 and t["by_matrix"] == 63 and t["by_scan"] == t["n"] - 64,
    "chain": lambda t: t["picks"] == 101 and t["by_scan"] == 3 and t["by_matrix"] == 97,
    "pick_slots": lambda t: t["scan_slots"] == {(p % 16, p // 16) for p in range(34)} and t["by_scan"] == 34 and t["by_matrix"] == 0,
    "ties": lambda t: t["ties"] >= 100 and t["by_matrix"] > 0,
    "signed_zero_tie": lambda t: t["signed_zero_ties"] > 0 and t["ties"] == t["n"] - 1,
    "thr_margin_keep": lambda t: t["margin"] == 1 and t["picks"] == 2,
    "thr_margin_kill": lambda t: t["margin"] == 1 and t["picks"] == 1,
    "thr_zero_keep": lambda t: t["picks"] == 3 and t["margin"] > 0,
    "thr_zero_kill": lambda t: t["picks"] == 1 and t["margin"] > 0,
    "thr_one": lambda t: t["picks"] == 5,
    "fractional": lambda t: t["fractional"] and t["by_matrix"] > 0 and t["by_scan"] > 0,
    "malformed": lambda t: t["malformed"],
    "empty": lambda t: t["n"] == 0,
}


# =================================================================================================================== rpn_to_roi
def _config(A):
    C = Config()
    if A == 1:
        C.anchor_box_scales, C.anchor_box_ratios = [48], [[1.0, 1.0]]
    elif A == 4:
        C.anchor_box_scales, C.anchor_box_ratios = [24, 40], [[1.0, 1.0], [1.0, 2.0]]
    elif A == 32:
        C.anchor_box_scales, C.anchor_box_ratios = [16, 24, 32, 48, 64, 96, 128, 256], [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0], [1.0, 3.0]]
    else:
        assert A == 12
    return C


def _wide_config():
    """One anchor 2001 wide and 3 high: every box spans its row band, so few picks are made and every candidate is examined."""
    C = Config()
    C.anchor_box_scales, C.anchor_box_ratios = [48], [[667.0, 1.0]]
    return C


def anchor_wh(C):
    return np.array(glue.anchor_shapes(C), np.float64)


def _scores(kind, n, rs):
    if kind == "distinct":
        return (rs.permutation(n).astype(F) + F(1)) / F(n + 1)
    if kind == "tie":
        return np.full(n, 0.5, F)
    if kind == "two_levels":
        return rs.choice(np.array([0.25, 0.75], F), n)
    if kind == "zeros":
        return np.zeros(n, F)
    assert kind == "denormal"
    return (rs.permutation(n).astype(np.uint32) + np.uint32(1)).view(F)


PLANTS = {            # kind -> [(delta index 0..3 = tx, ty, tw, th; the fp32 value written into pred)]
    "nan_tx": [(0, np.nan)], "nan_th": [(3, np.nan)], "pinf_tw": [(2, np.inf)], "ninf_tw": [(2, -np.inf)], "pinf_tx": [(0, np.inf)],
    "ninf_ty": [(1, -np.inf)], "overflow_tw": [(2, 3000.0)], "overflow_th": [(3, 2900.0)],
}


def _rpn_case(name, rows, cols, A, ld, scores, branch, regr="normal", use_regr=1, thr=0.7, mb=64, plant=None, C=None, seed=0):
    return dict(name=name, rows=rows, cols=cols, A=A, ld=ld, scores=scores, regr=regr, use_regr=use_regr, thr=float(thr), mb=mb, plant=plant,
                C=C if C is not None else _config(A), branch=branch, seed=seed)


@functools.lru_cache(maxsize=None)
def rpn_cases():
    W = _wide_config()
    c = [
        _rpn_case("one_row", 1, 2, 1, 5, "distinct", "all_degenerate"),
        _rpn_case("one_column", 2, 1, 1, 8, "distinct", "all_degenerate"),
        _rpn_case("two_by_two", 2, 2, 1, 5, "distinct", "some_valid"),
        _rpn_case("small_ld60", 3, 5, 12, 60, "distinct", "some_valid"),
        _rpn_case("small_ld64", 3, 5, 12, 64, "distinct", "some_valid"),
        _rpn_case("small_two_levels", 3, 5, 12, 64, "two_levels", "ties"),
        _rpn_case("max_anchors", 7, 9, 32, 160, "distinct", "some_valid"),
        _rpn_case("max_anchors_zeros", 7, 9, 32, 160, "zeros", "ties"),
        _rpn_case("max_anchors_denormal", 7, 9, 32, 160, "denormal", "denormal"),
        _rpn_case("one_block", 16, 16, 1, 5, "distinct", "one_block"),
        _rpn_case("one_block_max1", 16, 16, 1, 5, "distinct", "stop_at_max", mb=1),
        _rpn_case("one_block_max1024", 16, 16, 1, 5, "two_levels", "ties", mb=1024, thr=0.95),
        _rpn_case("one_block_denormal", 16, 16, 1, 5, "denormal", "denormal"),
        _rpn_case("second_block_one_row", 1, 257, 1, 5, "distinct", "all_degenerate"),
        _rpn_case("second_block", 2, 129, 1, 5, "distinct", "second_block"),
        _rpn_case("band_4095", 63, 65, 1, 5, "distinct", "one_band", regr="zero", thr=0.9, mb=1024, C=W),
        _rpn_case("band_4096", 64, 64, 1, 5, "distinct", "one_band", regr="zero", thr=0.9, mb=1024, C=W),
        _rpn_case("band_4097", 17, 241, 1, 5, "distinct", "two_bands", regr="zero", thr=0.9, mb=1024, C=W),
        _rpn_case("band_4097_max1", 17, 241, 1, 5, "distinct", "stop_at_max", regr="zero", thr=0.9, mb=1, C=W),
        _rpn_case("band_4097_max64_two_levels", 17, 241, 1, 5, "two_levels", "cut_in_tie", regr="zero", thr=0.9, mb=64, C=W),
        _rpn_case("single_tie_12293", 19, 647, 1, 5, "tie", "every_band_cut_in_tie", regr="zero", thr=0.9, mb=1024, C=W),
        _rpn_case("zeros_12293", 19, 647, 1, 5, "zeros", "every_band_cut_in_tie", regr="zero", thr=0.9, mb=1024, C=W),
        _rpn_case("no_regr", 7, 9, 4, 20, "distinct", "fractional", use_regr=0),
        _rpn_case("no_regr_ties", 7, 9, 4, 24, "two_levels", "fractional", use_regr=0, thr=0.5, mb=1024),
    ]
    for kind in PLANTS:
        c.append(_rpn_case("plant_" + kind, 9, 11, 4, 20, "distinct", "planted_finite" if kind in ("ninf_tw", "pinf_tx", "ninf_ty") else "nonfinite",
                           plant=(kind,), seed=3))
    c.append(_rpn_case("plant_mixed", 9, 11, 4, 20, "distinct", "nonfinite", plant=tuple(PLANTS), seed=3))
    return c


@functools.lru_cache(maxsize=None)
def rpn_inputs(i):
    """-> dict(pred [rows*cols][ld] fp32 (scores [0, A), deltas [A, 5A), 1e30 behind), planted: flat anchor-major indices)."""
    cs = rpn_cases()[i]
    rows, cols, A, ld = cs["rows"], cs["cols"], cs["A"], cs["ld"]
    rs = np.random.RandomState(500 + 31 * i + cs["seed"])
    hw = rows * cols
    pred = np.full((hw, ld), 1e30, F)
    scores = _scores(cs["scores"], hw * A, rs)                      # anchor-major flat order a * hw + pix
    pred[:, :A] = scores.reshape(A, hw).T
    pred[:, A:5 * A] = 0.0 if cs["regr"] == "zero" else (rs.standard_normal((hw, 4 * A)) * 0.4 * STD_SCALING).astype(F)
    planted = []
    if cs["plant"]:
        top = np.argsort(scores)[::-1]
        k = 0
        for kind in cs["plant"]:
            for q, v in PLANTS[kind]:
                for _ in range(3):                                     # three anchors per kind, the best-scoring ones
                    flat = int(top[k]); k += 1
                    a, pix = flat // hw, flat % hw
                    pred[pix, A + 4 * a + q] = F(v)
                    planted.append(flat)
    pred.setflags(write=False)
    return dict(pred=pred, planted=np.asarray(planted, np.int64))


@functools.lru_cache(maxsize=None)
def rpn_decoded(i):
    """The oracle's decode of case i: (boxes, probs, flat index) of the kept anchors, and which of them are non-finite boxes."""
    cs = rpn_cases()[i]
    rows, cols, A = cs["rows"], cs["cols"], cs["A"]
    pred = rpn_inputs(i)["pred"]
    cls = pred[:, :A].reshape(1, rows, cols, A)
    regr = pred[:, A:5 * A].reshape(1, rows, cols, 4 * A)
    with np.errstate(all="ignore"):
        boxes, probs, keep = glue.decode_all_anchors(cls, regr, cs["C"], bool(cs["use_regr"]))
    return boxes, probs, keep, ~np.isfinite(boxes).all(1)


def rpn_expected(i):
    cs = rpn_cases()[i]
    boxes, probs, keep, bad = rpn_decoded(i)
    mb = cs["mb"]
    res = glue.greedy_nms(boxes[~bad], probs[~bad], overlap_thresh=cs["thr"], max_boxes=mb)
    if len(res) == 0:
        rb, rp = None, None
        count = 0
    else:
        rb, rp = res[0].astype(np.int64), res[1].astype(F)
        count = len(rb)
        if not bad.any():                                             # the entry as a whole, where the reference does not assert
            assert np.array_equal(rb, _rpn_to_roi_oracle(i))
    return dict(out_boxes=_out(np.int64, (mb, 4), rb), out_probs=_out(F, (mb,), rp), out_count=_out(np.int32, (1,), [count]))


def _rpn_to_roi_oracle(i):
    cs = rpn_cases()[i]
    rows, cols, A = cs["rows"], cs["cols"], cs["A"]
    pred = rpn_inputs(i)["pred"]
    with np.errstate(all="ignore"):
        return glue.rpn_to_roi(pred[:, :A].reshape(1, rows, cols, A), pred[:, A:5 * A].reshape(1, rows, cols, 4 * A), cs["C"], bool(cs["use_regr"]),
                               cs["mb"], cs["thr"])


def rpn_keys(i):
    """64-bit keys of the decode kernel over the flat anchor order (0: dropped) and the boxes by flat index."""
    cs = rpn_cases()[i]
    boxes, probs, keep, bad = rpn_decoded(i)
    n = cs["rows"] * cs["cols"] * cs["A"]
    keys = np.zeros(n, np.uint64)
    k = keep[~bad]
    keys[k] = (sortable(probs[~bad]) << np.uint64(32)) | k.astype(np.uint64)
    full = np.zeros((n, 4))
    full[k] = boxes[~bad]
    return keys, full


def band_bounds(keys, upper, cap=BAND_CAP):
    """Radix select of select_nms_kernel: the lower bound `lo` of the best <= cap keys below `upper` (None: no bound yet), digits of 11 bits
    from the top (the last one 9), whole digits taken from the top while they fit, the digit that does not fit refined at the next level."""
    cand = keys != 0
    if upper is not None:
        cand &= keys < np.uint64(upper)
    lo, prefix, remaining = 0, 0, cap
    for level in range(6):
        hi_bit = 64 - 11 * level
        shift = max(hi_bit - 11, 0)
        width = hi_bit - shift
        todo = cand if level == 0 else cand & ((keys >> np.uint64(hi_bit)) == np.uint64(prefix))
        digit = ((keys[todo] >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)
        hist = np.bincount(digit, minlength=1 << width)
        if hist.sum() <= remaining:
            remaining -= int(hist.sum())
            lo = 0 if level == 0 else prefix << hi_bit
            break
        suffix = np.concatenate([np.cumsum(hist[::-1])[::-1], [0]])       # suffix[d] = keys with digit >= d
        d = int(np.argmax(suffix <= remaining))
        remaining -= int(suffix[d])
        base = 0 if level == 0 else prefix << width
        lo = (base + d) << shift
        prefix = base + d - 1
        if not (d > 0 and shift > 0 and remaining > 0):
            break
    return lo


def model_select(keys, boxes, thr, mb, mutant=None):
    """select_nms_kernel: band by band.  -> (picks, [lo of every band])."""
    cs = ChunkScan(boxes, thr, mb, mutant)
    upper, los = None, []
    while True:
        lo = band_bounds(keys, upper)
        take = (keys != 0) & (keys >= np.uint64(lo))
        if upper is not None:
            take &= keys < np.uint64(upper)
        band = np.sort(keys[take])[::-1]
        assert len(band) <= BAND_CAP
        if len(band) == 0:
            break
        los.append(lo)
        full = cs.feed((band & np.uint64(0xFFFFFFFF)).astype(np.int64))
        if full or lo == 0:
            break
        upper = lo
        if mutant == "band_cut_drops_tie":
            upper = (lo >> 32) << 32
    return np.asarray(cs.picks, np.int64), los


def _lower_first(keys):
    valid = np.nonzero(keys)[0]
    return valid[np.lexsort((valid, -(keys[valid] >> np.uint64(32)).astype(np.int64)))]


def model_full_sort(keys, boxes, thr, mb, mutant=None):
    order = np.argsort(keys, kind="stable")[::-1][:int((keys != 0).sum())]
    if mutant == "ties_lower_index_first":
        order = _lower_first(keys)
    cs = ChunkScan(boxes, thr, mb, mutant)
    cs.feed(order)
    return np.asarray(cs.picks, np.int64)


def rpn_model_outputs(i, path, mutant=None):
    """(boxes int64, fp32 scores) of a model of one of the two paths on case i."""
    cs = rpn_cases()[i]
    keys, boxes = rpn_keys(i)
    if path == "select" and cs["use_regr"] and cs["thr"] > 0:
        picks, _ = model_select(keys, boxes, cs["thr"], cs["mb"], mutant)
    else:
        picks = model_full_sort(keys, boxes, cs["thr"], cs["mb"], mutant)
    hw = cs["rows"] * cs["cols"]
    pred = rpn_inputs(i)["pred"]
    return boxes[picks].astype(np.int64), pred[picks % hw, picks // hw]


def rpn_tally(i):
    cs = rpn_cases()[i]
    boxes, probs, keep, bad = rpn_decoded(i)
    keys, full = rpn_keys(i)
    n = cs["rows"] * cs["cols"] * cs["A"]
    order = np.argsort(keys, kind="stable")[::-1][:int((keys != 0).sum())]
    t = nms_tally(full[order], probs=np.zeros(len(order)), thr=cs["thr"], mb=cs["mb"], order=np.arange(len(order))) if len(order) else dict(picks=0, stop="never", ties=0)
    sc = rpn_inputs(i)["pred"][order % (cs["rows"] * cs["cols"]), order // (cs["rows"] * cs["cols"])]
    t["ties"] = int((sc[1:] == sc[:-1]).sum())
    t.update(candidates=n, valid=len(order), blocks=-(-n // 256), nonfinite=int(bad.sum()), planted=len(rpn_inputs(i)["planted"]),
             planted_nonfinite=int(np.isin(rpn_inputs(i)["planted"], keep[bad]).sum()), denormal=bool(len(sc) and (np.abs(sc) < np.finfo(F).tiny).all() and (sc != 0).all()),
             fractional=bool((boxes != np.floor(boxes)).any()))
    if cs["use_regr"] and cs["thr"] > 0:
        _, los = model_select(keys, full, cs["thr"], cs["mb"])
        t["bands"] = len(los)
        t["cuts_in_tie"] = sum(1 for lo in los if lo & 0xFFFFFFFF)
    else:
        t["bands"], t["cuts_in_tie"] = 0, 0
    return t


RPN_REACH = {
    "all_degenerate": lambda t: t["valid"] == 0 and t["candidates"] > 0,
    "some_valid": lambda t: t["valid"] > 0 and t["picks"] > 0 and t["nonfinite"] == 0,
    "ties": lambda t: t["ties"] > 0 and t["picks"] > 0,
    "denormal": lambda t: t["denormal"] and t["picks"] > 0,
    "one_block": lambda t: t["candidates"] == 256 and t["blocks"] == 1,
    "second_block": lambda t: t["candidates"] == 258 and t["blocks"] == 2 and t["valid"] > 0,
    "stop_at_max": lambda t: t["stop"] in ("inside_chunk", "on_chunk_end", "on_last"),
    "one_band": lambda t: t["valid"] in (4095, 4096) and t["valid"] == t["candidates"] and t["bands"] == 1 and t["stop"] == "never",
    "two_bands": lambda t: t["valid"] == 4097 and t["bands"] == 2 and t["stop"] == "never",
    "cut_in_tie": lambda t: t["cuts_in_tie"] >= 1,
    "every_band_cut_in_tie": lambda t: t["valid"] == 3 * 4096 + 5 and t["bands"] == 4 and t["cuts_in_tie"] == 3 and t["stop"] == "never" and t["picks"] > 1,
    "fractional": lambda t: t["fractional"] and t["picks"] > 0 and t["bands"] == 0,
    "nonfinite": lambda t: t["nonfinite"] > 0 and t["planted_nonfinite"] == t["nonfinite"],
    "planted_finite": lambda t: t["nonfinite"] == 0 and t["planted"] == 3,
}

RPN_REFUSED = [      # (what, rows, cols, a, ld, max_boxes)
    ("a = 0", 3, 5, 0, 64, 64), ("a = 33", 3, 5, 33, 200, 64), ("max_boxes = 0", 3, 5, 12, 64, 0), ("max_boxes = 1025", 3, 5, 12, 64, 1025),
    ("ld_pred < 5a", 3, 5, 12, 59, 64),
]


# =================================================================================================================== anchor targets
AnchorMap = collections.namedtuple("AnchorMap", "fw fh scales ratios rw rh")
R1 = ((1.0, 1.0),)
R3 = ((1.0, 1.0), (1.0, 2.0), (2.0, 1.0))
ANCHOR_MAPS = [
    AnchorMap(1, 1, (16,), R1, 16, 16), AnchorMap(1, 7, (16,), R1, 16, 112), AnchorMap(7, 1, (16,), R1, 112, 16),
    AnchorMap(5, 3, (16,), R1, 80, 48), AnchorMap(5, 3, (16,), R1, 79, 47),          # the last column and row end one pixel beyond
    AnchorMap(5, 3, (18,), R1, 80, 48),                                                # the first column and row start at -1
    AnchorMap(16, 16, (16,), R1, 256, 256), AnchorMap(13, 20, (16, 18, 32, 48), R3, 208, 320),
]
GT_KINDS = ("none", "equal", "fallback", "no_overlap", "all_bg", "bg_and_fg", "degenerate", "identical_pair", "two_onto_one", "fallback_on_positive",
            "between_x", "between_y", "fp32_tie", "many")


def _cell(ix, jy):
    return np.array([16.0 * ix, 16.0 * jy, 16.0 * ix + 16.0, 16.0 * jy + 16.0])


def _gt(m, kind):
    """Ground truth of `kind` on map m in RESIZED pixels: (boxes (g, 4) x1 y1 x2 y2, is_bg (g,)), or None where the map has no room."""
    ix, jy = m.fw // 2, m.fh // 2
    c = _cell(ix, jy)
    small = c + np.array([4.0, 4.0, -4.0, -4.0])
    if kind == "none":
        return np.zeros((0, 4)), np.zeros(0, np.int32)
    if kind == "equal":
        return c[None], [0]
    if kind == "fallback":
        return small[None], [0]
    if kind == "no_overlap":
        return np.array([[m.rw + 10.0, 2.0, m.rw + 30.0, 12.0]]), [0]
    if kind == "all_bg":
        return np.stack([c, small]), [1, 1]
    if kind == "bg_and_fg":
        if m.fw * m.fh < 2:
            return None
        o = _cell(0, 0) if (ix, jy) != (0, 0) else _cell(m.fw - 1, m.fh - 1)
        return np.stack([c, o, small]), [1, 0, 1]
    if kind == "degenerate":
        return np.array([[c[0] + 3.0, c[1] + 2.0, c[0] + 3.0, c[3] - 1.0], small]), [0, 0]
    if kind == "identical_pair":
        return np.stack([small, small]), [0, 0]
    if kind == "two_onto_one":
        return np.stack([small, c + np.array([3.0, 5.0, -2.0, -4.0]), c + np.array([5.0, 3.0, -3.0, -3.0])]), [0, 0, 0]
    if kind == "fallback_on_positive":
        return np.stack([c, small]), [0, 0]
    if kind == "between_x":
        if m.fw < 2:
            return None
        i0 = max(ix - 1, 0)
        return (_cell(i0, jy) + np.array([8.0, 0.0, 8.0, 0.0]))[None], [0]
    if kind == "between_y":
        if m.fh < 2:
            return None
        j0 = max(jy - 1, 0)
        return (_cell(ix, j0) + np.array([0.0, 8.0, 0.0, 8.0]))[None], [0]
    if kind == "fp32_tie":
        if m.fw < 2:
            return None
        i0 = max(ix - 1, 0)
        return (_cell(i0, jy) + np.array([8.0 + 2.0 ** -30, 0.0, 8.0 + 2.0 ** -30, 0.0]))[None], [0]
    assert kind == "many"
    rs = np.random.RandomState(m.fw * 100 + m.fh)
    g = 1024
    xy = np.stack([rs.uniform(-4.0, m.rw - 4.0, g), rs.uniform(-4.0, m.rh - 4.0, g)], 1)
    wh = rs.choice([8.0, 12.0, 16.0, 17.0, 24.0, 40.0], (g, 2))
    b = np.concatenate([xy, xy + wh], 1)
    snap = np.arange(0, g, 7)                                   # every seventh box equals an anchor cell
    b[snap] = np.stack([_cell(rs.randint(m.fw), rs.randint(m.fh)) for _ in snap])
    return b, (rs.uniform(size=g) < 0.2).astype(np.int32)


@functools.lru_cache(maxsize=None)
def anchor_cases():
    cases = []
    for mi, m in enumerate(ANCHOR_MAPS):
        for kind in GT_KINDS:
            if kind == "many" and (m.fw, m.fh) not in ((5, 3), (13, 20)):
                continue
            if mi in (4, 5) and kind not in ("none", "equal", "fallback", "between_x", "many"):
                continue
            gt = _gt(m, kind)
            if gt is None:
                continue
            boxes, bg = gt
            # source image twice the resized one: the scale rw / width is exactly 0.5
            cases.append(dict(name="%dx%d_a%d_rw%d_s%d_%s" % (m.fw, m.fh, len(m.scales) * len(m.ratios), m.rw, m.scales[0], kind), map=m, kind=kind,
                              gt=np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4) * 2.0), bg=np.asarray(bg, np.int32),
                              width=2 * m.rw, height=2 * m.rh, branch=kind))
    return cases


def _anchor_config(m):
    C = Config()
    C.anchor_box_scales, C.anchor_box_ratios = list(m.scales), [list(r) for r in m.ratios]
    return C


@functools.lru_cache(maxsize=None)
def anchor_dense(i):
    cs = anchor_cases()[i]
    m = cs["map"]
    with np.errstate(all="ignore"):
        return glue.anchor_targets_dense(_anchor_config(m), cs["gt"], cs["bg"], cs["width"], cs["height"], m.rw, m.rh, m.fw, m.fh)


def _regr_loose(shape_hw, A):
    lo = np.zeros(shape_hw + (4 * A,), bool)
    lo[..., 2::4] = True
    lo[..., 3::4] = True
    return lo


def anchor_expected(i):
    """-> {valid [A][fh][fw] u8, overlap, regr [fh][fw][4A] f64, best_anchor [g][4] i32}.  n_for_gt is scratch of the fallback (the
    count of anchors above max_overlap per box), compared as well."""
    cs = anchor_cases()[i]
    m, d = cs["map"], anchor_dense(i)
    A, g = len(m.scales) * len(m.ratios), len(cs["gt"])
    out = dict(valid=_out(np.uint8, (A, m.fh, m.fw), d["valid"].transpose(2, 0, 1)), overlap=_out(np.uint8, (A, m.fh, m.fw), d["overlap"].transpose(2, 0, 1)),
               regr=_out(np.float64, (m.fh, m.fw, 4 * A), d["regr"], loose=_regr_loose((m.fh, m.fw), A)))
    out["best_anchor"] = _out(np.int32, (max(g, 1), 4), d["best_anchor"] if g else None)
    out["n_for_gt"] = _out(np.int32, (max(g, 1),), d["n_for_gt"] if g else None)
    return out


def anchor_pack_expected(i):
    """Inputs (the oracle's dense arrays in the kernel's layouts) and the packed fp32 tensors of to_train_layout."""
    cs = anchor_cases()[i]
    m, d = cs["map"], anchor_dense(i)
    A = len(m.scales) * len(m.ratios)
    va, ov = d["valid"].transpose(2, 0, 1)[None], d["overlap"].transpose(2, 0, 1)[None]
    rg = d["regr"].transpose(2, 0, 1)[None]
    y_cls, y_regr = glue.to_train_layout(np.concatenate([va, ov], 1), np.concatenate([np.repeat(ov, 4, axis=1), rg], 1), STD_SCALING)
    ins = dict(valid=np.ascontiguousarray(va[0], np.uint8), overlap=np.ascontiguousarray(ov[0], np.uint8), regr=np.ascontiguousarray(d["regr"], np.float64))
    return ins, dict(y_cls=_out(F, (m.fh, m.fw, 2 * A), y_cls[0].astype(F)), y_regr=_out(F, (m.fh, m.fw, 8 * A), y_regr[0].astype(F)))


def _visit(m):
    """Every anchor in visiting order o = ((si * nr + ri) * fw + ix) * fh + jy: (si, ri, ix, jy, box (n, 4), inside)."""
    ns, nr = len(m.scales), len(m.ratios)
    o = np.arange(ns * nr * m.fw * m.fh)
    jy, ix, ar = o % m.fh, (o // m.fh) % m.fw, o // (m.fh * m.fw)
    ri, si = ar % nr, ar // nr
    ax = np.asarray(m.scales, np.float64)[si] * np.asarray(m.ratios, np.float64)[ri, 0]
    ay = np.asarray(m.scales, np.float64)[si] * np.asarray(m.ratios, np.float64)[ri, 1]
    x1, x2 = 16.0 * (ix + 0.5) - ax / 2, 16.0 * (ix + 0.5) + ax / 2
    y1, y2 = 16.0 * (jy + 0.5) - ay / 2, 16.0 * (jy + 0.5) + ay / 2
    inside = ~((x1 < 0) | (x2 > m.rw)) & ~((y1 < 0) | (y2 > m.rh))
    return si, ri, ix, jy, np.stack([x1, y1, x2, y2], 1), inside


def _deltas(gx1, gx2, gy1, gy2, b):
    with np.errstate(all="ignore"):
        return np.array([((gx1 + gx2) / 2.0 - (b[0] + b[2]) / 2.0) / (b[2] - b[0]), ((gy1 + gy2) / 2.0 - (b[1] + b[3]) / 2.0) / (b[3] - b[1]),
                         np.log((gx2 - gx1) / (b[2] - b[0])), np.log((gy2 - gy1) / (b[3] - b[1]))])


def model_anchor_targets(i, mutant=None, max_overlap=0.7):
    """anchor_targets_kernel + anchor_fallback_kernel: one thread per anchor, best anchor per box by the maximum of
    (fp32 IoU bits << 32 | ~visiting index), the fallback applied afterwards by one thread in ground-truth order."""
    cs = anchor_cases()[i]
    m = cs["map"]
    ns, nr = len(m.scales), len(m.ratios)
    A, g = ns * nr, len(cs["gt"])
    valid, overlap, regr = np.zeros((m.fh, m.fw, A)), np.zeros((m.fh, m.fw, A)), np.zeros((m.fh, m.fw, 4 * A))
    best_anchor, n_for_gt = -np.ones((g, 4), int), np.zeros(g, int)
    if g == 0:
        return dict(valid=valid, overlap=overlap, regr=regr, best_anchor=best_anchor, n_for_gt=n_for_gt)
    si, ri, ix, jy, box, inside = _visit(m)
    sx, sy = m.rw / float(cs["width"]), m.rh / float(cs["height"])
    gx1, gx2, gy1, gy2 = cs["gt"][:, 0] * sx, cs["gt"][:, 2] * sx, cs["gt"][:, 1] * sy, cs["gt"][:, 3] * sy
    fg = cs["bg"] == 0
    n = len(box)
    gb = np.stack([gx1, gy1, gx2, gy2], 1)
    iou = glue.iou_pairs(np.broadcast_to(gb[None], (n, g, 4)), np.broadcast_to(box[:, None], (n, g, 4)))
    iou = np.where(inside[:, None], iou, 0.0)
    o = np.arange(n, dtype=np.uint64)
    if mutant == "best_anchor_fp64":
        bits = iou.view(np.uint64) >> np.uint64(1)                  # fp64 order, one bit of room for the comparison below
        lead = np.where((iou > 0) & inside[:, None] & fg[None, :], bits, 0)
        best_o = np.where(lead.max(0) > 0, np.argmax(lead, 0), -1)
    else:
        v32 = iou.astype(F)
        low = o if mutant == "last_best_anchor" else np.uint64(0xFFFFFFFF) - o
        key = np.where((v32 > 0) & inside[:, None] & fg[None, :], (v32.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[:, None], 0)
        kmax = key.max(0)
        lowbits = (kmax & np.uint64(0xFFFFFFFF)).astype(np.int64)
        best_o = np.where(kmax > 0, lowbits if mutant == "last_best_anchor" else 0xFFFFFFFF - lowbits, -1)
    pos = (iou > max_overlap) & fg[None, :] & inside[:, None]
    n_for_gt[:] = pos.sum(0)
    ch = ri + nr * si
    for a in np.nonzero(inside)[0]:
        valid[jy[a], ix[a], ch[a]] = 1
        if pos[a].any():
            k = int(np.argmax(np.where(pos[a], iou[a], -1.0)))
            overlap[jy[a], ix[a], ch[a]] = 1
            regr[jy[a], ix[a], 4 * ch[a]:4 * ch[a] + 4] = _deltas(gx1[k], gx2[k], gy1[k], gy2[k], box[a])
    ks = range(g - 1, -1, -1) if mutant == "fallback_reverse_order" else range(g)
    for k in ks:
        a = int(best_o[k])
        if a < 0:
            continue
        best_anchor[k] = [jy[a], ix[a], ri[a], si[a]]
        if n_for_gt[k] == 0:
            valid[jy[a], ix[a], ch[a]] = 1
            overlap[jy[a], ix[a], ch[a]] = 1
            regr[jy[a], ix[a], 4 * ch[a]:4 * ch[a] + 4] = _deltas(gx1[k], gx2[k], gy1[k], gy2[k], box[a]).astype(F)
    return dict(valid=valid, overlap=overlap, regr=regr, best_anchor=best_anchor, n_for_gt=n_for_gt)


def anchor_tally(i):
    cs = anchor_cases()[i]
    m, d = cs["map"], anchor_dense(i)
    g = len(cs["gt"])
    si, ri, ix, jy, box, inside = _visit(m)
    t = dict(g=g, anchors=len(box), blocks=-(-len(box) // 256), inside=int(inside.sum()), edge_on_zero=bool(((box[:, 0] == 0) & inside).any()),
             edge_on_rw=bool(((box[:, 2] == m.rw) & inside).any()), one_beyond=bool(((box[:, 0] == -1) | (box[:, 2] == m.rw + 1)).any()),
             positives=int(d["overlap"].sum()), valid=int(d["valid"].sum()), fallbacks=0, no_best=0, fp32_ties=0, fp64_disagrees=0, shared_fallback=0,
             fallback_on_positive=0, bg=int(cs["bg"].sum()), degenerate=0, exact_fp64_ties=0)
    if g == 0:
        return t
    sx, sy = m.rw / float(cs["width"]), m.rh / float(cs["height"])
    gb = np.stack([cs["gt"][:, 0] * sx, cs["gt"][:, 1] * sy, cs["gt"][:, 2] * sx, cs["gt"][:, 3] * sy], 1)
    t["degenerate"] = int(((gb[:, 0] >= gb[:, 2]) | (gb[:, 1] >= gb[:, 3])).sum())
    n = len(box)
    iou = np.where(inside[:, None], glue.iou_pairs(np.broadcast_to(gb[None], (n, g, 4)), np.broadcast_to(box[:, None], (n, g, 4))), 0.0)
    pos = iou > 0.7
    targets = collections.Counter()
    for k in range(g):
        if cs["bg"][k]:
            continue
        if d["best_anchor"][k, 0] < 0:
            t["no_best"] += 1
            continue
        v32 = iou[:, k].astype(F)
        top = np.nonzero(v32 == v32.max())[0]
        if len(top) > 1:
            t["fp32_ties"] += 1
            if len(np.unique(iou[top, k])) == 1:
                t["exact_fp64_ties"] += 1
            if int(np.argmax(iou[:, k])) != int(top[0]):
                t["fp64_disagrees"] += 1
        if d["n_for_gt"][k] == 0:
            t["fallbacks"] += 1
            a = int(top[0])
            targets[a] += 1
            if (pos[a] & (cs["bg"] == 0)).any():
                t["fallback_on_positive"] += 1
    t["shared_fallback"] = sum(1 for v in targets.values() if v > 1)
    return t


ANCHOR_REACH = {
    "none": lambda t: t["g"] == 0 and t["valid"] == 0,
    "equal": lambda t: t["positives"] >= 1 and t["fallbacks"] == 0 and t["no_best"] == 0,
    "fallback": lambda t: t["fallbacks"] == 1 and t["positives"] == 1,
    "no_overlap": lambda t: t["no_best"] == 1 and t["positives"] == 0 and t["valid"] == t["inside"] > 0,
    "all_bg": lambda t: t["bg"] == t["g"] and t["positives"] == 0 and t["valid"] == t["inside"] > 0,
    "bg_and_fg": lambda t: 0 < t["bg"] < t["g"] and t["positives"] == 1,
    "degenerate": lambda t: t["degenerate"] == 1 and t["no_best"] == 1,
    "identical_pair": lambda t: t["shared_fallback"] == 1 and t["fallbacks"] == 2,
    "two_onto_one": lambda t: t["shared_fallback"] == 1 and t["fallbacks"] == 3,
    "fallback_on_positive": lambda t: t["fallback_on_positive"] == 1,
    "between_x": lambda t: t["exact_fp64_ties"] == 1 and t["fallbacks"] == 1,
    "between_y": lambda t: t["exact_fp64_ties"] == 1 and t["fallbacks"] == 1,
    "fp32_tie": lambda t: t["fp32_ties"] == 1 and t["fp64_disagrees"] == 1 and t["exact_fp64_ties"] == 0,
    "many": lambda t: t["g"] == 1024 and t["fallbacks"] > 0 and t["positives"] > 0 and t["shared_fallback"] > 0 and t["fp32_ties"] > 0 and t["bg"] > 0,
}

ANCHOR_REFUSED = [("g = 1025", 1025, 4, 3), ("ns = 17", 2, 17, 3), ("nr = 17", 2, 4, 17)]           # (what, g, ns, nr)


# =================================================================================================================== RoI targets
ROI_W, ROI_H = 600, 1000                  # source image: new_img_size gives (600, 1000), the scale is exactly 1
ROI_COLS, ROI_ROWS = 37, 62


def _roi_config(nc=7):
    C = Config()
    if nc != 7:
        C.class_mapping = dict([("c%d" % k, k) for k in range(nc - 1)] + [("bg", nc - 1)])
    return C


@functools.lru_cache(maxsize=None)
def roi_cases():
    cases = []
    for n in (1, 255, 256, 257):
        for g in (0, 1, 40):
            for nd in ("null", "zero", "n_minus_1", "larger"):
                cases.append(dict(name="n%d_g%d_ndev_%s" % (n, g, nd), n=n, g=g, n_dev={"null": None, "zero": 0, "n_minus_1": n - 1, "larger": n + 7}[nd],
                                  nc=7, special=(n >= 255 and g == 40), branch="special" if (n >= 255 and g == 40 and nd in ("null", "larger")) else "rows"))
    return cases


@functools.lru_cache(maxsize=None)
def roi_inputs(i, nc=7):
    cs = roi_cases()[i]
    n, g = cs["n"], cs["g"]
    rs = np.random.RandomState(9000 + 17 * n + g)
    bg = nc - 1
    gx, gy = rs.randint(0, ROI_COLS - 6, g), rs.randint(0, ROI_ROWS - 6, g)
    gw, gh = rs.randint(2, 12, g), rs.randint(2, 12, g)
    gt = np.stack([16.0 * gx + rs.randint(-7, 8, g), 16.0 * gy + rs.randint(-7, 8, g), 16.0 * (gx + gw) + rs.randint(-7, 8, g),
                   16.0 * (gy + gh) + rs.randint(-7, 8, g)], 1).astype(np.float64).reshape(g, 4)
    gcls = rs.randint(0, nc - 1, g).astype(np.int32)
    x1, y1 = rs.randint(0, ROI_COLS - 2, n), rs.randint(0, ROI_ROWS - 2, n)
    rois = np.stack([x1, y1, np.minimum(x1 + rs.randint(1, 14, n), ROI_COLS), np.minimum(y1 + rs.randint(1, 14, n), ROI_ROWS)], 1).astype(np.int64)
    if g:                                    # two thirds of the RoIs near a ground-truth box
        k = rs.randint(0, g, n)
        near = np.stack([gx[k], gy[k], gx[k] + gw[k], gy[k] + gh[k]], 1) + rs.randint(-1, 2, (n, 4))
        near[:, 2:] = np.maximum(near[:, 2:], near[:, :2] + 1)
        use = rs.uniform(size=n) < 0.66
        rois[use] = np.maximum(near[use], 0)
    if cs["special"]:
        gt[0] = [40.0, 40.0, 168.0, 168.0]                   # 2.5, 10.5 after scaling: half to even gives 2, 10
        gt[1] = gt[2] = [320.0, 320.0, 480.0, 448.0]          # two boxes, equal IoU with everything: the first wins
        gcls[1], gcls[2] = nc - 2, 0
        gt[3] = [16.0 * 30, 16.0 * 50, 16.0 * 35, 16.0 * 58]  # a background-class box
        gcls[3] = bg
        gt[4] = [24.0, 600.0, 104.0, 744.0]                   # 1.5, 37.5, 6.5, 46.5 -> 2, 38, 6, 46
        rois[0] = [5, 7, 5, 12]                               # zero width
        rois[1] = [2, 2, 10, 10]                              # equal to box 0 after rounding
        rois[2] = [20, 20, 30, 28]                            # equal to boxes 1 and 2
        rois[3] = [30, 50, 35, 57]                            # best match is the background-class box
        rois[4] = [2, 38, 6, 46]
        rois[5] = [3, 38, 7, 47]                              # what half away from zero would match
        rois[6] = [21, 20, 30, 29]
    for a in (gt, gcls, rois):
        a.setflags(write=False)
    return dict(rois=rois, gt=gt, gt_cls=gcls)


def _round_half_away(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def model_roi_targets(rois, gt, gt_cls, C, mutant=None):
    """roi_targets_kernel, one RoI per thread -> per-row (keep, cls, box, t, iou) for EVERY row."""
    n, g = len(rois), len(gt)
    bg = C.class_mapping["bg"]
    rw, rh = glue.new_img_size(ROI_W, ROI_H, C.img_size)
    rnd = _round_half_away if mutant == "round_half_away" else np.rint
    G = np.zeros((g, 4))
    if g:
        G = np.stack([rnd(gt[:, 0] * (rw / float(ROI_W)) / C.rpn_stride), rnd(gt[:, 1] * (rh / float(ROI_H)) / C.rpn_stride),
                      rnd(gt[:, 2] * (rw / float(ROI_W)) / C.rpn_stride), rnd(gt[:, 3] * (rh / float(ROI_H)) / C.rpn_stride)], 1)
    keep, cls = np.zeros(n, np.uint8), -np.ones(n, np.int32)
    box, t, iou = np.zeros((n, 4), np.int32), np.zeros((n, 4)), np.zeros(n)
    std = C.classifier_regr_std
    for i, (x1, y1, x2, y2) in enumerate(np.asarray(rois, np.float64)):
        best, bk = 0.0, -1
        for k in range(g):
            v = float(glue.iou_pairs(G[k], [x1, y1, x2, y2]))
            if v > best or (mutant == "last_gt_wins_tie" and v >= best and v > 0):
                best, bk = v, k
        w, h = x2 - x1, y2 - y1
        box[i], iou[i] = [x1, y1, w, h], best
        if best < C.classifier_min_overlap:
            continue
        keep[i], cls[i] = 1, bg
        if not best < C.classifier_max_overlap:
            cls[i] = gt_cls[bk]
            if cls[i] != bg:
                t[i] = [std[0] * (((G[bk, 0] + G[bk, 2]) / 2.0 - (x1 + w / 2.0)) / w), std[1] * (((G[bk, 1] + G[bk, 3]) / 2.0 - (y1 + h / 2.0)) / h),
                        std[2] * np.log((G[bk, 2] - G[bk, 0]) / w), std[3] * np.log((G[bk, 3] - G[bk, 1]) / h)]
    return dict(keep=keep, cls=cls, box=box, t=t, iou=iou)


@functools.lru_cache(maxsize=None)
def roi_rows(i, nc=7):
    """Per-row (keep, cls, box, t, iou) of EVERY RoI of case i from glue.roi_targets: once as configured (which rows are kept, their
    class and targets) and once with classifier_min_overlap = 0, where the oracle keeps every row and so states the box and the IoU of
    the dropped ones as well."""
    d = roi_inputs(i, nc)
    n = len(d["rois"])
    C, C0 = _roi_config(nc), _roi_config(nc)
    C0.classifier_min_overlap = 0.0
    bg = C.class_mapping["bg"]
    X0, _, _, iou0 = glue.roi_targets(d["rois"], d["gt"], d["gt_cls"], ROI_W, ROI_H, C0)
    assert X0.shape[1] == n
    iou = np.asarray(iou0, np.float64)
    box = X0[0].astype(np.int32)
    keep = (~(iou < C.classifier_min_overlap)).astype(np.uint8)
    cls, t = -np.ones(n, np.int32), np.zeros((n, 4))
    X, Y1, Y2, ious = glue.roi_targets(d["rois"], d["gt"], d["gt_cls"], ROI_W, ROI_H, C)
    rows = np.nonzero(keep)[0]
    if X is None:
        assert len(rows) == 0
    else:
        assert X.shape[1] == len(rows) and np.array_equal(X[0], box[rows]) and np.array_equal(np.asarray(ious), iou[rows])
        c = Y1[0].argmax(-1)
        cls[rows] = c
        nreg = 4 * (nc - 1)
        for r, row in enumerate(rows):
            if c[r] != bg:
                t[row] = Y2[0, r, nreg + 4 * c[r]:nreg + 4 * c[r] + 4]
    return dict(keep=keep, cls=cls, box=box, t=t, iou=iou, X=X, Y1=Y1, Y2=Y2, kept=rows)


def roi_expected(i):
    cs = roi_cases()[i]
    n, r = cs["n"], roi_rows(i)
    live = np.arange(n) < (n if cs["n_dev"] is None else min(cs["n_dev"], n))
    keep, cls = np.where(live, r["keep"], 0), np.where(live, r["cls"], -1)
    loose = np.zeros((n, 4), bool)
    loose[:, 2:] = True
    t = Out(_masked(np.float64, (n, 4), r["t"], np.repeat(live, 4)), np.concatenate([loose.reshape(-1), np.zeros(TAIL, bool)]))
    return dict(keep=_out(np.uint8, (n,), keep), cls=_out(np.int32, (n,), cls), box=Out(_masked(np.int32, (n, 4), r["box"], np.repeat(live, 4)), None),
                t=t, iou=Out(_masked(np.float64, (n,), r["iou"], live), None))


def roi_tally(i):
    cs, d, r = roi_cases()[i], roi_inputs(i), roi_rows(i)
    n = cs["n"]
    live = n if cs["n_dev"] is None else min(cs["n_dev"], n)
    fgd = (r["cls"] >= 0) & (r["cls"] != 6)
    t = dict(n=n, g=cs["g"], blocks=-(-n // 256), live=live, kept=int(r["keep"].sum()), fg=int(fgd.sum()), hard_negative=int(((r["cls"] == 6) & (r["iou"] < 0.5)).sum()),
             dropped=int((r["keep"] == 0).sum()), zero_width=int((d["rois"][:, 0] == d["rois"][:, 2]).sum()), iou_one=int((r["iou"] > 0.999).sum()),
             bg_best=int(((r["cls"] == 6) & (r["iou"] >= 0.5)).sum()), half=0, tie_first=0)
    if cs["g"]:
        v = np.concatenate([d["gt"][:, [0, 2]] * (600 / 600.0) / 16.0, d["gt"][:, [1, 3]] * (1000 / 1000.0) / 16.0], 1)
        t["half"] = int((v - np.floor(v) == 0.5).sum())
        m_first = model_roi_targets(d["rois"], d["gt"], d["gt_cls"], _roi_config())
        m_last = model_roi_targets(d["rois"], d["gt"], d["gt_cls"], _roi_config(), "last_gt_wins_tie")
        t["tie_first"] = int((m_first["cls"] != m_last["cls"]).sum())
    return t


ROI_REACH = {
    "rows": lambda t: t["live"] <= t["n"] and (t["g"] > 0 or t["kept"] == 0) and (t["n"] == 1 or t["g"] == 0 or t["kept"] > 0) and t["blocks"] == (2 if t["n"] == 257 else 1),
    "special": lambda t: t["zero_width"] >= 1 and t["iou_one"] >= 2 and t["tie_first"] >= 1 and t["bg_best"] >= 1 and t["half"] >= 4 and t["fg"] > 0
    and t["hard_negative"] > 0 and t["dropped"] > 0,
}

PACK_CASES = [(r, nc) for r in (1, 4, 33) for nc in (2, 7, 21)]


@functools.lru_cache(maxsize=None)
def pack_inputs(k):
    """-> dict(sel, cls, box, t (the oracle's per-row arrays of the n = 257, g = 40 case relabelled for nc classes), r, nc, bg)."""
    r, nc = PACK_CASES[k]
    i = next(j for j, c in enumerate(roi_cases()) if c["n"] == 257 and c["g"] == 40 and c["n_dev"] is None)
    rows = roi_rows(i, nc)
    rs = np.random.RandomState(70 + k)
    kept = rows["kept"]
    bgs, fgs = kept[rows["cls"][kept] == nc - 1], kept[rows["cls"][kept] != nc - 1]
    assert len(bgs) and len(fgs)
    pool = np.concatenate([rs.choice(fgs, max(r // 2, 1)), rs.choice(bgs, r)])[:r]
    sel = pool[rs.permutation(r)]
    if r >= 4:
        sel[2] = sel[0]                                        # a repeat, and the order is not ascending
        sel[1] = bgs[-1]
        sel[3] = fgs[0]
    return dict(sel=sel.astype(np.int32), cls=rows["cls"], box=rows["box"], t=rows["t"], r=r, nc=nc, bg=nc - 1, rows=rows)


def pack_expected(k):
    d = pack_inputs(k)
    rows, r, nc = d["rows"], d["r"], d["nc"]
    pos = {int(row): j for j, row in enumerate(rows["kept"])}
    j = np.array([pos[int(s)] for s in d["sel"]])
    return dict(rois_out=_out(F, (r, 4), rows["X"][0][j].astype(F)), y1=_out(F, (r, nc), rows["Y1"][0][j].astype(F)),
                y2=_out(F, (r, 8 * (nc - 1)), rows["Y2"][0][j].astype(F)))


def pack_empty_expected(nc=7):
    return dict(rois_out=_out(F, (1, 4)), y1=_out(F, (1, nc)), y2=_out(F, (1, 8 * (nc - 1))))


# =================================================================================================================== judgement (host)
def judge(name, got, exp):
    """`got`: the full buffer read back (same dtype and length as exp.buf) -> list of complaints (empty: passes).  Bit for bit, except
    the `log` components: LOG_RTOL relative in fp64 with the fp32 casts bit-equal."""
    got = np.asarray(got)
    assert got.dtype == exp.buf.dtype and got.shape == exp.buf.shape, (name, got.dtype, got.shape, exp.buf.dtype, exp.buf.shape)
    u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    same = got.view(u) == exp.buf.view(u)
    if exp.loose is not None:
        s = sentinel(got.dtype, 1)[0]
        lo = exp.loose & (exp.buf.view(u) != s.view(u)) & ~same
        if lo.any():
            a, b = got[lo].astype(np.float64), exp.buf[lo].astype(np.float64)
            with np.errstate(all="ignore"):
                ok = (np.abs(a - b) <= LOG_RTOL * np.maximum(np.abs(b), 1e-300)) & (a.astype(F).view(np.uint32) == b.astype(F).view(np.uint32))
            same[np.nonzero(lo)[0][ok]] = True
    bad = np.nonzero(~same)[0]
    if len(bad) == 0:
        return []
    return ["%s: %d of %d elements differ, first at %d: got %r, expected %r" % (name, len(bad), got.size, bad[0], got[bad[0]], exp.buf[bad[0]])]
