"""Case tables and a NumPy model of the two device contracts of csrc/scan_tail.hip -- radnet_final_nms and radnet_scan_merge --,
written from include/radnet_hip.h.  The model shares no code with RADNet.final_nms or RADNet.predict: test_scan_tail_host.py holds
it against them (and against tests/golden/final_nms.npz), test_gpu_scan_tail.py holds the kernels against it.  Every model function
takes `mutant`, the name of one deliberate mistake (MUTANTS): the host tests show that the cases catch each of them."""
import os

import numpy as np

HEADER, RECORD = 8, 6                       # radnet_detect_tail's output: int32 words in front of / per record
MAX_COORD = 1 << 29                         # RADNET_SCAN_MAX_COORD
FN_MALFORMED, FN_EMPTY, FN_RANGE = -1, -2, -3
SM_BAD_SLOT, SM_MALFORMED, SM_EMPTY, SM_RANGE, SM_NMS_BOX = -1, -2, -3, -4, -5
SENTINEL = -7
MUTANTS = ("unstable_ties", "member_ge", "fp64_threshold", "first_n_obj_avg", "sequential_sum", "half_away", "class_order_by_index")
DEFAULTS = dict(obj_avg_threshold=0.2, obj_confidence_threshold=0.8, n_obj_avg=5)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "final_nms.npz")


# ---- the fp32 sum np.mean takes over a contiguous vector ---------------------------------------------------------------------
def np_sum_f32(a):
    a = np.asarray(a, dtype=np.float32)
    n = len(a)
    if n < 8:
        r = np.float32(0)
        for v in a:
            r = np.float32(r + v)
        return r
    if n <= 128:
        r = [np.float32(v) for v in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = np.float32(r[j] + a[i + j])
            i += 8
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3])) + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        while i < n:
            res = np.float32(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return np.float32(np_sum_f32(a[:n2]) + np_sum_f32(a[n2:]))


def mean_f32(a, mutant=None):
    a = np.asarray(a, dtype=np.float32)
    if mutant == "sequential_sum":
        s = np.float32(0)
        for v in a:
            s = np.float32(s + v)
    else:
        s = np.float32(np.float32(0) + np_sum_f32(a))
    return np.float32(s / np.float32(len(a)))


def round_mean(total, count, mutant=None):
    q = float(total) / float(count)
    if mutant == "half_away":
        return int(np.sign(q) * np.floor(abs(q) + 0.5))
    return int(round(q))                    # Python's round: half to even


# ---- radnet_final_nms on one group ---------------------------------------------------------------------------------------------
def final_nms_model(boxes, probs, obj_avg_threshold=0.2, obj_confidence_threshold=0.8, n_obj_avg=5, mutant=None):
    """(status, boxes int64 [k][4], probs float32 [k]); with a negative status the rest is None."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    probs = np.asarray(probs, dtype=np.float32).reshape(-1)
    n = len(probs)
    if n == 0:
        return 0, np.zeros((0, 4), np.int64), np.zeros(0, np.float32)
    x1, y1, x2, y2 = (boxes[:, q] for q in range(4))
    if np.any(x1 >= x2) or np.any(y1 >= y2):
        return FN_MALFORMED, None, None
    if np.any(boxes[:, :2] < -MAX_COORD) or np.any(boxes[:, 2:] > MAX_COORD) or np.any(np.isnan(probs)):
        return FN_RANGE, None, None
    conf = np.float32(obj_confidence_threshold)
    area = (x2 - x1) * (y2 - y1)
    tie = -1 if mutant == "unstable_ties" else 1
    live = sorted(range(n), key=lambda i: (float(probs[i]), tie * i))
    out_b, out_p, empty = [], [], False
    while live:
        order = np.array(live)
        top, rest = order[-1], order[:-1]
        iw = np.maximum(0, np.minimum(x2[top], x2[rest]) - np.maximum(x1[top], x1[rest]))
        ih = np.maximum(0, np.minimum(y2[top], y2[rest]) - np.maximum(y1[top], y1[rest]))
        inter = iw * ih
        overlap = inter.astype(np.float64) / ((area[top] + area[rest] - inter).astype(np.float64) + 1e-6)
        hit = overlap >= obj_avg_threshold if mutant == "member_ge" else overlap > obj_avg_threshold
        members = list(rest[hit]) + [top]
        mp = probs[members]
        if mutant == "fp64_threshold":
            below, above = float(mp[-1]) < float(obj_confidence_threshold), mp.astype(np.float64) > float(obj_confidence_threshold)
        else:
            below, above = mp[-1] < conf, mp > conf          # the maximum is top's
        if below:
            chosen = members[:n_obj_avg] if mutant == "first_n_obj_avg" else members[-n_obj_avg:]
        else:
            chosen = [m for m, a in zip(members, above) if a]
        if not chosen:
            empty = True
        else:
            out_b.append([round_mean(sum(int(boxes[m, q]) for m in chosen), len(chosen), mutant) for q in range(4)])
            out_p.append(mean_f32(probs[chosen], mutant))
        gone = set(members)
        live = [j for j in live if j not in gone]
    if empty:
        return FN_EMPTY, None, None
    return 0, np.array(out_b, np.int64).reshape(-1, 4), np.array(out_p, np.float32)


# ---- radnet_scan_merge ---------------------------------------------------------------------------------------------------------------
def greedy_nms_model(boxes, probs, thresh, max_boxes):
    """Indices picked, or None for a malformed box: fp64, stable ascending order walked from the end."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    if np.any(b[:, 0] >= b[:, 2]) or np.any(b[:, 1] >= b[:, 3]):
        return None
    live = sorted(range(len(b)), key=lambda i: (float(probs[i]), i))
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    picks = []
    while live and len(picks) < max_boxes:
        top = live.pop()
        picks.append(top)
        keep = []
        for j in live:
            ww = max(0.0, min(b[top, 2], b[j, 2]) - max(b[top, 0], b[j, 0]))
            hh = max(0.0, min(b[top, 3], b[j, 3]) - max(b[top, 1], b[j, 1]))
            inter = ww * hh
            if not inter / (area[top] + area[j] - inter + 1e-6) > thresh:
                keep.append(j)
        live = keep
    return picks


def scan_merge_out_words(nc, max_boxes):
    return HEADER + RECORD * nc * max_boxes


def scan_merge_model(pool, tiles, slot_rows, nc, nms_thresh=0.4, max_boxes=300, mutant=None, **fn):
    """The int32 words radnet_scan_merge leaves in an output prefilled with SENTINEL.  tiles: rows (slot, ox, oy, image)."""
    fn = dict(DEFAULTS, **fn)
    out = np.full(scan_merge_out_words(nc, max_boxes), SENTINEL, np.int32)
    status = 0
    groups, first = {}, {}                  # (image, class) -> ([boxes], [probs]) in insertion order; class -> first appearance
    for t, (slot, ox, oy, image) in enumerate(tiles):
        m = int(pool[slot])
        if m < 0 or m > slot_rows:
            status = min(status, SM_BAD_SLOT)
            continue
        rec = pool[slot + HEADER:slot + HEADER + RECORD * m].reshape(m, RECORD)
        for r in range(m):
            c = int(rec[r, 0])
            if c < 0 or c >= nc:
                status = min(status, SM_BAD_SLOT)
                continue
            first.setdefault(c, (t, r))
            g = groups.setdefault((int(image), c), ([], []))
            g[0].append([int(rec[r, 1]) + ox, int(rec[r, 2]) + oy, int(rec[r, 3]) + ox, int(rec[r, 4]) + oy])
            g[1].append(rec[r, 5:6].view(np.float32)[0])
    clusters = {}                           # class -> ([boxes], [probs]) over the images in image order
    for (image, c) in sorted(groups):
        st, b, p = final_nms_model(groups[(image, c)][0], groups[(image, c)][1], mutant=mutant, **fn)
        if st < 0:
            status = min(status, {FN_MALFORMED: SM_MALFORMED, FN_EMPTY: SM_EMPTY, FN_RANGE: SM_RANGE}[st])
            continue
        k = clusters.setdefault(c, ([], []))
        k[0].extend(b.tolist())
        k[1].extend(list(p))
    records = []
    if status == 0:
        order = sorted(first) if mutant == "class_order_by_index" else sorted(first, key=first.get)
        for c in order:
            b, p = np.array(clusters[c][0], np.int64), np.array(clusters[c][1], np.float32)
            picks = greedy_nms_model(b, p, nms_thresh, max_boxes)
            if picks is None:
                status = SM_NMS_BOX
                break
            for i in picks:
                records.append([c] + [int(v) for v in b[i]] + [int(p[i:i + 1].view(np.int32)[0])])
    if status < 0:
        records = []
    out[0], out[1] = len(records), status
    if records:
        out[HEADER:HEADER + RECORD * len(records)] = np.array(records, np.int64).astype(np.int32).reshape(-1)
    return out


# ---- building pools ------------------------------------------------------------------------------------------------------------------
def slot_words(slot_rows):
    return HEADER + RECORD * slot_rows


def make_pool(tile_records, slot_rows, slots=None, counts=None):
    """(pool int32, slots): tile_records[t] = [(class, x1, y1, x2, y2, prob), ...] written as radnet_detect_tail writes them, tile t
    at word slots[t] (default: one after the other); counts[t] overrides the count word.  Unused words hold SENTINEL."""
    sw = slot_words(slot_rows)
    slots = [t * sw for t in range(len(tile_records))] if slots is None else list(slots)
    pool = np.full(max([0] + [s + sw for s in slots]), SENTINEL, np.int32)
    for t, (recs, s) in enumerate(zip(tile_records, slots)):
        assert len(recs) <= slot_rows
        pool[s] = len(recs) if counts is None or counts[t] is None else counts[t]
        pool[s + 1] = slot_rows
        for r, (c, x1, y1, x2, y2, p) in enumerate(recs):
            at = s + HEADER + RECORD * r
            pool[at:at + 5] = (c, x1, y1, x2, y2)
            pool[at + 5:at + 6] = np.array([p], np.float32).view(np.int32)
    return pool, slots


# ---- cases for radnet_final_nms: name -> (boxes int64 [n][4], probs float32 [n][, other parameters]) ----------------------------------------------------
F08 = np.float32(0.8)
UP, DOWN = np.nextafter(F08, np.float32(1)), np.nextafter(F08, np.float32(0))


def _near(n, p_lo, p_hi, seed, x0=100, y0=100, size=60, jitter=3):
    """n near-identical boxes (one cluster) with probs spread over [p_lo, p_hi]."""
    rs = np.random.RandomState(seed)
    d = rs.randint(-jitter, jitter + 1, (n, 4))
    b = np.array([x0, y0, x0 + size, y0 + size]) + d
    return b.astype(np.int64), rs.uniform(p_lo, p_hi, n).astype(np.float32)


def _scatter(n, centres, seed, extent=4000):
    """n boxes scattered round `centres` common centres: a few hundred clusters."""
    rs = np.random.RandomState(seed)
    c = rs.randint(50, extent, (centres, 2))
    pick = rs.randint(0, centres, n)
    xy = c[pick] + rs.randint(-6, 7, (n, 2))
    wh = rs.randint(30, 50, (n, 2))
    b = np.concatenate([xy, xy + wh], axis=1).astype(np.int64)
    p = rs.uniform(0.7, 1.0, n).astype(np.float32)
    p[rs.randint(0, n, n // 10)] = p[0]                  # ties
    return b, p


def final_nms_cases():
    cases = {}
    B = lambda *rows: np.array(rows, np.int64).reshape(-1, 4)
    P = lambda *v: np.array(v, np.float32)
    cases["one"] = (B([3, 4, 10, 12]), P(0.9))
    cases["tie_overlapping"] = (B([0, 0, 10, 10], [1, 1, 11, 11]), P(0.9, 0.9))
    cases["tie_disjoint"] = (B([0, 0, 10, 10], [50, 50, 61, 63]), P(0.75, 0.75))
    cases["tie_three_mixed"] = (B([0, 0, 10, 10], [2, 0, 13, 10], [1, 1, 12, 11], [40, 40, 50, 50]), P(0.9, 0.95, 0.9, 0.9))
    for m in (4, 5, 6):                                   # below 0.8: the last n_obj_avg members
        b, p = _near(m, 0.70, 0.79, 10 + m)
        b[:, 0] += np.arange(m) * 2                       # the first and the last n_obj_avg members have different means
        cases["below_%d" % m] = (b, p)
    cases["just_above"] = (B([0, 0, 10, 10], [1, 0, 11, 10], [0, 1, 10, 11]), P(0.5, UP, 0.7))
    cases["just_below"] = (B([0, 0, 10, 10], [1, 0, 11, 10], [0, 1, 10, 11]), P(0.5, DOWN, 0.7))
    cases["exactly_threshold"] = (B([0, 0, 10, 10], [1, 0, 11, 10]), P(0.5, F08))           # status -2
    cases["threshold_and_above"] = (B([0, 0, 10, 10], [1, 0, 11, 10], [0, 1, 10, 11]), P(F08, UP, 0.5))
    # overlap exactly 1/5: 10x10 boxes shifted by x so that inter / union = (10 - x) * 10 / (200 - (10 - x) * 10)
    # a 6x1 and a 6x1 sharing 2: inter 2, union 10 -> exactly 0.2, not a member (the 1e-6); sharing 3 of 7+...: pairs round it
    cases["overlap_fifth"] = (B([0, 0, 6, 1], [4, 0, 10, 1]), P(0.9, 0.85))
    cases["overlap_above_fifth"] = (B([0, 0, 600, 1], [399, 0, 999, 1]), P(0.9, 0.85))      # 201 / 999
    cases["overlap_below_fifth"] = (B([0, 0, 600, 1], [401, 0, 1001, 1]), P(0.9, 0.85))     # 199 / 1001
    cases["mean_half_even"] = (B([0, 0, 10, 10], [1, 1, 11, 11]), P(0.9, 0.95))             # means 0.5, 0.5, 10.5, 10.5
    cases["mean_half_odd"] = (B([1, 1, 11, 11], [2, 2, 12, 12]), P(0.9, 0.95))              # means 1.5, 1.5, 11.5, 11.5
    cases["mean_half_negative"] = (B([-3, -3, 8, 8], [-2, -2, 9, 9], [-6, -5, 6, 7], [-5, -6, 7, 6]), P(0.9, 0.95, 0.85, 0.97))
    for m in (7, 8, 9, 16, 17, 128, 129, 136, 137, 300):
        cases["sum_%d" % m] = _near(m, 0.81, 0.999, 100 + m)
    cases["sum_mixed_300"] = _near(300, 0.5, 0.999, 77)   # part of the cluster above the threshold
    cases["scatter_1025"] = _scatter(1025, 260, 5)
    cases["scatter_2049"] = _scatter(2049, 420, 6)
    cases["malformed_x"] = (B([0, 0, 10, 10], [5, 5, 5, 9]), P(0.9, 0.8))
    cases["malformed_y"] = (B([0, 0, 10, 10], [5, 9, 8, 2]), P(0.9, 0.8))
    cases["negative_zero"] = (B([0, 0, 10, 10], [1, 1, 11, 11], [50, 50, 60, 60]), P(-0.0, 0.0, -0.0))
    cases["empty"] = (np.zeros((0, 4), np.int64), np.zeros(0, np.float32))
    # other parameters: overlap 0 against a threshold of 0 is not a member; n_obj_avg 1 and 2; a threshold no prob exceeds
    cases["threshold_zero_disjoint"] = (B([0, 0, 10, 10], [50, 50, 60, 60], [5, 5, 15, 15]), P(0.9, 0.95, 0.7), dict(obj_avg_threshold=0.0))
    cases["n_obj_avg_1"] = _near(6, 0.3, 0.5, 31) + (dict(n_obj_avg=1),)
    cases["n_obj_avg_2_conf_half"] = _near(9, 0.3, 0.7, 32) + (dict(n_obj_avg=2, obj_confidence_threshold=0.5),)
    if os.path.exists(GOLDEN):
        g = np.load(GOLDEN)
        for i in range(int(g["n_cases"])):               # the reference ran on fp64 probs; the product's are fp32
            cases["golden_c%d" % i] = (g["c%d_boxes" % i].astype(np.int64), g["c%d_probs" % i].astype(np.float32))
    return cases


def case_args(case):
    """(boxes, probs, parameters) of a final_nms case."""
    return case[0], case[1], dict(DEFAULTS, **(case[2] if len(case) > 2 else {}))


FINAL_NMS_BATCH = ("scatter_1025", "empty", "one", "sum_129", "malformed_x", "below_6", "exactly_threshold", "empty", "scatter_2049", "tie_three_mixed")


# ---- cases for radnet_scan_merge: name -> dict(records per tile, tiles (ox, oy, image), slot_rows, nc, [slots], [counts]) --------------
def _rec(c, x1, y1, w, h, p):
    return (c, x1, y1, x1 + w, y1 + h, np.float32(p))


def scan_merge_cases():
    cases = {}
    cases["zero_record_tiles"] = dict(records=[[], [_rec(1, 10, 10, 40, 40, 0.9), _rec(1, 12, 11, 40, 40, 0.85)], [], []],
                                      tiles=[(0, 0, 0), (100, 0, 0), (0, 100, 0), (0, 0, 0)], slot_rows=4, nc=3)
    cases["all_empty"] = dict(records=[[], []], tiles=[(0, 0, 0), (5, 5, 1)], slot_rows=2, nc=4)
    cases["class_in_later_tile"] = dict(records=[[_rec(2, 10, 10, 40, 40, 0.9)], [_rec(0, 300, 10, 40, 40, 0.95), _rec(2, 14, 12, 40, 40, 0.7)]],
                                        tiles=[(0, 0, 0), (0, 0, 0)], slot_rows=3, nc=4)
    # the first tile lists class 3 before class 1; index order would say 1, 3
    cases["class_order_in_tile"] = dict(records=[[_rec(3, 10, 10, 40, 40, 0.9), _rec(1, 200, 10, 40, 40, 0.95)]], tiles=[(0, 0, 0)], slot_rows=2, nc=5)
    cases["two_images_class_orders"] = dict(records=[[_rec(2, 10, 10, 40, 40, 0.9), _rec(0, 300, 10, 40, 40, 0.85)],
                                                     [_rec(0, 500, 500, 40, 40, 0.9), _rec(2, 700, 10, 40, 40, 0.95)]],
                                            tiles=[(0, 0, 0), (0, 0, 1)], slot_rows=2, nc=3)
    cases["class_only_in_second_image"] = dict(records=[[_rec(1, 10, 10, 40, 40, 0.9)], [_rec(0, 10, 10, 40, 40, 0.9), _rec(1, 500, 500, 40, 40, 0.99)]],
                                               tiles=[(0, 0, 0), (0, 0, 1)], slot_rows=2, nc=2)
    # the same object in two images: IoU 36*38 / (2*1600 - 36*38) = 0.747 > 0.4 across, and a second pair at IoU 0.33 that both stay
    cases["cross_image_suppression"] = dict(records=[[_rec(1, 100, 100, 40, 40, 0.9), _rec(1, 400, 400, 40, 40, 0.7)],
                                                     [_rec(1, 104, 102, 40, 40, 0.95), _rec(1, 420, 400, 40, 40, 0.75)]],
                                            tiles=[(0, 0, 0), (0, 0, 1)], slot_rows=2, nc=2)
    many = [_rec(1, 60 * (i % 20), 60 * (i // 20), 40, 40, 0.5 + 0.0009 * i) for i in range(301)]
    cases["max_boxes_cap"] = dict(records=[many[:151], many[151:]], tiles=[(0, 0, 0), (0, 0, 0)], slot_rows=151, nc=2)
    # one object seen by four tiles at the same scan position
    cases["cluster_over_four_tiles"] = dict(records=[[_rec(1, 190, 190, 50, 50, 0.9)], [_rec(1, 91, 189, 50, 50, 0.85)], [_rec(1, 189, 92, 50, 50, 0.95)],
                                                     [_rec(1, 92, 91, 50, 50, 0.7), _rec(0, 5, 5, 20, 20, 0.9)]],
                                            tiles=[(0, 0, 0), (100, 0, 0), (0, 100, 0), (100, 100, 0)], slot_rows=2, nc=2)
    cases["slot_count_minus_one"] = dict(records=[[_rec(1, 10, 10, 40, 40, 0.9)], [_rec(1, 10, 10, 40, 40, 0.9)]], tiles=[(0, 0, 0), (0, 0, 0)], slot_rows=2,
                                         nc=2, counts=[None, -1])
    cases["slot_count_too_large"] = dict(records=[[_rec(1, 10, 10, 40, 40, 0.9)]], tiles=[(0, 0, 0)], slot_rows=2, nc=2, counts=[3])
    cases["class_out_of_range"] = dict(records=[[_rec(1, 10, 10, 40, 40, 0.9), _rec(2, 10, 10, 40, 40, 0.9)]], tiles=[(0, 0, 0)], slot_rows=2, nc=2)
    cases["x1_equals_x2"] = dict(records=[[_rec(1, 10, 10, 40, 40, 0.9), _rec(1, 70, 10, 0, 40, 0.9)]], tiles=[(30, 0, 0)], slot_rows=2, nc=2)
    cases["empty_cluster"] = dict(records=[[_rec(1, 10, 10, 40, 40, F08)]], tiles=[(0, 0, 0)], slot_rows=2, nc=2)
    cases["coordinate_out_of_range"] = dict(records=[[_rec(1, 2 ** 30, 10, 40, 40, 0.9)]], tiles=[(MAX_COORD, 0, 0)], slot_rows=1, nc=2)
    # cluster means (1.5 -> 2, 2.5 -> 2) that collapse a one-pixel box at the final NMS
    cases["nms_box_collapses"] = dict(records=[[_rec(1, 1, 0, 1, 10, 0.9), _rec(1, 2, 0, 1, 10, 0.95)]], tiles=[(0, 0, 0)], slot_rows=2, nc=2,
                                      fn=dict(obj_avg_threshold=-1.0))
    cases["slots_not_ascending"] = dict(records=[[_rec(2, 10, 10, 40, 40, 0.9)], [_rec(0, 300, 10, 40, 40, 0.95)], [_rec(2, 14, 12, 40, 40, 0.7)]],
                                        tiles=[(0, 0, 0), (0, 0, 0), (0, 0, 1)], slot_rows=3, nc=3, slots=[2 * 26 + 4, 0, 26 + 2])
    rs = np.random.RandomState(11)
    recs, tiles = [], []
    for t in range(9):                                    # three images of three tiles, a few hundred boxes of 5 classes round common centres
        n = int(rs.randint(0, 120))
        centres = rs.randint(0, 300, (12, 2))
        cls = np.sort(rs.randint(0, 5, n)) if t % 2 else -np.sort(-rs.randint(0, 5, n))      # a class is one run, as the tile tail writes it
        recs.append([_rec(int(c), int(centres[i % 12, 0] + rs.randint(-5, 6)), int(centres[i % 12, 1] + rs.randint(-5, 6)), int(rs.randint(30, 45)),
                          int(rs.randint(30, 45)), rs.uniform(0.7, 1.0)) for i, c in enumerate(cls)])
        tiles.append((int(100 * (t % 3)), int(37 * (t % 2)), t // 3))
    cases["random_three_images"] = dict(records=recs, tiles=tiles, slot_rows=120, nc=6)
    # 2049 clusters of one class, beyond the NMS's LDS sort and two strides of its walk: disjoint boxes on a grid, 1025 in the first image and
    # 1024 in the second, shifted by (4, 2): IoU 36*38 / (2*1600 - 36*38) = 0.747 > 0.4 across the images; probs with ties
    rs = np.random.RandomState(12)
    p = rs.uniform(0.5, 1.0, 2049).astype(np.float32)
    p[rs.randint(0, 2049, 200)] = p[0]
    grid = lambda n, dx, dy, pr: [_rec(1, 60 * (i % 35) + dx, 60 * (i // 35) + dy, 40, 40, pr[i]) for i in range(n)]
    cases["class_nms_2049"] = dict(records=[grid(1025, 0, 0, p[:1025]), grid(1024, 4, 2, p[1025:])], tiles=[(0, 0, 0), (0, 0, 1)], slot_rows=1025, nc=2)
    return cases


def build_scan_case(case):
    """(pool, table rows (slot, ox, oy, image), keyword arguments of scan_merge_model) of one scan_merge case."""
    pool, slots = make_pool(case["records"], case["slot_rows"], case.get("slots"), case.get("counts"))
    tiles = [(s, ox, oy, im) for s, (ox, oy, im) in zip(slots, case["tiles"])]
    kw = dict(slot_rows=case["slot_rows"], nc=case["nc"], nms_thresh=case.get("nms_thresh", 0.4), max_boxes=case.get("max_boxes", 300))
    kw.update(case.get("fn", {}))
    return pool, tiles, kw
