"""Happens-before audit of TrainStep's pipelined schedule (tests/lane_audit.py), on the real radnet_hip.trainer.TrainStep, without a GPU.

Every scenario runs the real step / flush / losses / validate code on the recording stand-in and asserts that no two conflicting accesses
to one buffer are left unordered by the lanes' events and the host's waits.  The mutants then take the ordering edges away one at a time:
every after(...) of TrainStep.step, of the phases it is made of and of flush, and each of the three host waits is either NEEDED (some scenario reports a race without it) or
listed in REDUNDANT with the path that orders the same accesses anyway -- both directions are asserted, so the table cannot rot and a wait
that is not needed shows up as such."""
import ast
import collections
import inspect
import sys
import textwrap

import numpy as np
import pytest

import lane_audit as LA
from lane_audit import AuditEngine, Recorder, audit, describe

FAIL_W, SKIP_W = 13, 17          # source widths that script the host decisions: the labeller fails / no RoI is kept
SHAPE_A, SHAPE_B = (32, 48, 3), (48, 32, 3)


def _script(width, height):
    return "fail" if width == FAIL_W else "skip" if width == SKIP_W else "pick"


def _sample(width=1000, shape=SHAPE_A):
    return dict(img=np.zeros(shape, np.uint8), bboxes=[dict({"class": "fg"}, x1=0, x2=2, y1=0, y2=2)], width=width, height=600)


class Scenario:
    def __init__(self, name, nloc=1, lookahead=3, n_side=2, crop=True, deferred_ok=True, defer_update=False, stack=False, batched=True,
                 widths=None, shapes=None, silent=(), reannounce=(), validate_at=(), plain_at=(), timed_at=(), loss_log=False, capture=False, steps=None):
        self.name, self.nloc, self.lookahead, self.n_side, self.crop, self.deferred_ok = name, nloc, lookahead, n_side, crop, deferred_ok
        self.defer_update, self.stack, self.batched = defer_update, stack, batched
        self.widths = widths or {}            # (step, image) -> source width (FAIL_W / SKIP_W)
        self.shapes = shapes                  # step -> image shape
        self.silent = set(silent)             # steps that announce nothing (upcoming=[]): the next batch arrives un-announced
        self.reannounce = set(reannounce)     # steps whose announcement keeps only the next batch and replaces the ones behind it
        self.validate_at = set(validate_at)   # validate() before these steps
        self.plain_at = set(plain_at)         # flush(), then a non-pipelined call (upcoming=None)
        self.timed_at = set(timed_at)         # calls made while the engine's launch timing is on: no lanes, and no flush() before them
        self.loss_log, self.capture = loss_log, capture
        self.steps = steps

    def lanes(self):
        return ["main", "head"] + ["side%d" % k if k else "side" for k in range(self.n_side)]


def n_steps(scn):
    from radnet_hip.trainer import TrainStep
    return scn.steps or 2 * TrainStep.NBUF + TrainStep.LOOKAHEAD + 1 + 3


Result = collections.namedtuple("Result", "pairs examined trace eng ts sites_hit")


def trainstep_functions():
    """Every function defined in class TrainStep, found from the class (methods, static and class methods, property accessors), in source
    order: an ordering edge may live in any of them."""
    from radnet_hip.trainer import TrainStep
    fns = []
    for v in vars(TrainStep).values():
        if isinstance(v, (staticmethod, classmethod)):
            v = v.__func__
        fns += [f for f in ((v.fget, v.fset, v.fdel) if isinstance(v, property) else (v,)) if inspect.isfunction(f)]
    return sorted(fns, key=lambda f: f.__code__.co_firstlineno)


def _code_objects(code):
    """A function's code object and those of the functions nested in it."""
    yield code
    for c in code.co_consts:
        if inspect.iscode(c):
            yield from _code_objects(c)


def run(scn, skip_site=None, skip_wait=None):
    """One scenario on the real TrainStep.  skip_site: line in trainer.py of an after(...) that is left out; skip_wait: a host wait that does
    not join the host clock."""
    from radnet_hip import trainer as T
    np.random.seed(64)
    eng = AuditEngine(n_side_lanes=scn.n_side, script=_script, deferred_ok=scn.deferred_ok, crop_ahead=scn.crop)
    if skip_wait:
        eng.rec.skip_waits.add(skip_wait)
    sites_hit = set()
    real_after = eng.after

    codes = {c for fn in trainstep_functions() for c in _code_objects(fn.__code__)}

    def after(ev):                      # the ordering edges of TrainStep's methods, known by the caller's line
        f = sys._getframe(1)
        if f.f_code in codes:
            sites_hit.add(f.f_lineno)
            if f.f_lineno == skip_site:
                return
        real_after(ev)
    eng.after = after
    ts = eng.bind(T.TrainStep(eng, world_size=1, defer_head_update=scn.defer_update))
    ts.on_drop = lambda sample, exc: None
    ts.stack_base, ts.batched, ts.crop_ahead = scn.stack, scn.batched, scn.crop
    if scn.loss_log:
        ts.start_loss_log(64)
    if scn.capture:
        ts.capture = []
    n = n_steps(scn)
    batches = [[_sample(scn.widths.get((k, i), 1000), scn.shapes(k) if scn.shapes else SHAPE_A) for i in range(scn.nloc)] for k in range(n)]
    extra = [[_sample() for i in range(scn.nloc)] for _ in range(8)]
    val = [_sample(), _sample(SKIP_W), _sample(FAIL_W), _sample()]
    for b in batches + extra + [val]:   # ground truth is on the device before the run (a training run sees its samples again and again):
        for s in b:                     # the blocking upload would otherwise hide races behind a host wait
            ts._gt(s)
    for k, b in enumerate(batches):
        eng.rec.step = k
        if k in scn.validate_at:
            ts.validate(val)
        eng.ctx.timing_on = k in scn.timed_at
        if k in scn.plain_at:
            ts.flush()
            ts.step(b)
        elif k in scn.silent:
            ts.step(b, upcoming=[])
        elif k in scn.reannounce:
            ts.step(b, upcoming=(batches[k + 1:k + 2] + extra)[:scn.lookahead])
        else:
            ts.step(b, upcoming=batches[k + 1:k + 1 + scn.lookahead])
        if k == 12 or k == n - 1:       # losses() waits for the head lane: once in the middle, where it cannot stand in for every other edge
            ts.losses()
    eng.rec.step = "flush"
    ts.flush()
    ts.losses()
    pairs, examined = audit(eng.rec.trace)
    return Result(pairs, examined, eng.rec.trace, eng, ts, sites_hit)


def _ab(k):
    # pairs first, then lone batches (neighbours of different sizes never pair), then pairs again, then lone ones: a buffer set first used
    # by a pair is re-used by a lone batch and the reverse
    return SHAPE_A if (k < 9 or 17 <= k < 26) else (SHAPE_A, SHAPE_B)[k % 2]


SCENARIOS = [
    Scenario("lookahead 1", lookahead=1),
    Scenario("lookahead 3", lookahead=3, loss_log=True, capture=True),
    Scenario("lookahead 4", lookahead=4),
    Scenario("batch 2 stacked", nloc=2),
    Scenario("batch 2 image by image", nloc=2, batched=False),
    Scenario("stack_base pairs", stack=True, lookahead=4),
    Scenario("stack_base pairs and lone batches", stack=True, lookahead=4, shapes=_ab, steps=34),
    Scenario("one prefetch lane", n_side=1),
    Scenario("three prefetch lanes", n_side=3, lookahead=4),
    Scenario("no crop-ahead", crop=False),
    Scenario("no crop-ahead, batch 2 stacked", crop=False, nloc=2),
    Scenario("paired weight gradients", deferred_ok=False),
    Scenario("deferred head update", defer_update=True),
    Scenario("dropped image, current and announced", nloc=2, widths={(0, 1): FAIL_W, (9, 0): FAIL_W, (10, 1): FAIL_W, (18, 0): FAIL_W}, silent=[17]),
    Scenario("dropped image, image by image", nloc=2, batched=False, widths={(0, 0): FAIL_W, (11, 1): FAIL_W}),
    Scenario("skipped head step", widths={(3, 0): SKIP_W, (12, 0): SKIP_W, (13, 0): SKIP_W}),
    Scenario("skipped head step in a stacked batch", nloc=2, widths={(4, 0): SKIP_W, (12, 1): SKIP_W, (13, 0): SKIP_W, (13, 1): SKIP_W}),
    Scenario("whole batch dropped", widths={(0, 0): FAIL_W, (6, 0): FAIL_W, (15, 0): FAIL_W}),
    Scenario("whole stacked batch dropped", nloc=2, widths={(7, 0): FAIL_W, (7, 1): FAIL_W}),
    Scenario("un-announced batch", silent=[5, 14]),
    Scenario("un-announced batch, nothing prepared", lookahead=1, silent=[10, 15, 20]),
    # (with crop-ahead the feature map's last reader is on the main lane, behind a host wait: only here does the head lane read it)
    Scenario("un-announced batch, nothing prepared, no crop-ahead", lookahead=1, silent=[10, 15, 20], crop=False),
    Scenario("timed call in the middle", timed_at=[9, 18]),
    # regression: prepared batches that are dropped gave their buffer sets up for lost, and two replaced announcements in a row wrapped the
    # rotation around onto the set of the batch whose classifier phase was still to come
    Scenario("announcement replaced", lookahead=4, reannounce=[4, 13]),
    Scenario("announcement replaced, pairs and lone batches", stack=True, lookahead=4, shapes=_ab, steps=34, reannounce=[4, 8, 13, 18, 19, 27], silent=[11, 23]),
    Scenario("validate in the middle", validate_at=[6, 15], capture=True),
    Scenario("non-pipelined call in the middle", plain_at=[7, 8, 16]),
]
IDS = [s.name for s in SCENARIOS]


@pytest.fixture(scope="module")
def clean_runs():
    return {s.name: run(s) for s in SCENARIOS}


@pytest.mark.parametrize("scn", SCENARIOS, ids=IDS)
def test_scenario_has_no_unordered_conflicting_access(scn, clean_runs):
    from radnet_hip.trainer import TrainStep
    r = clean_runs[scn.name]
    print("%s: %d conflicting pairs examined, %d operations" % (scn.name, r.examined, len(r.trace)))
    assert n_steps(scn) >= 2 * TrainStep.NBUF + TrainStep.LOOKAHEAD + 1
    assert not r.pairs, describe(r.pairs)
    # ... and not vacuously
    assert r.examined > 0
    used = {o.lane for o in r.trace if o.reads or o.writes}
    assert set(scn.lanes()) | {LA.HOST} <= used, (scn.lanes(), used)
    writers = collections.defaultdict(set)
    for o in r.trace:
        if o.slot is not None:
            for res in o.writes:
                if res not in LA.GLOBALS:
                    writers[res].add(o.step)
    assert any(len(v) >= 3 for v in writers.values()), "no buffer set was re-used twice"


def test_scenarios_reach_what_they_are_named_for(clean_runs):
    def names(key):
        return collections.Counter(o.name for o in clean_runs[key].trace)
    r = clean_runs
    assert r["dropped image, current and announced"].ts.dropped_images == 4 and names("dropped image, current and announced")["rpn_loss_image: zero rows"] == 4
    assert r["dropped image, image by image"].ts.dropped_images == 2
    assert r["skipped head step"].ts.skipped_head_steps == 3
    assert r["skipped head step in a stacked batch"].ts.skipped_head_steps == 4 and names("skipped head step in a stacked batch")["idle_roi_group"] == 2
    assert names("skipped head step in a stacked batch")["head_forward: live mask"] >= 2
    assert r["whole batch dropped"].ts.dropped_images == 3 and names("whole batch dropped")["adam(rpn)"] == n_steps(SCENARIOS[0]) - 3
    assert r["whole stacked batch dropped"].ts.dropped_images == 2
    assert names("paired weight gradients")["head_update_deferred"] == 0 and names("lookahead 3")["head_update_deferred"] > 0
    assert names("deferred head update")["head_update_deferred"] == 0 and names("deferred head update")["adam(head)"] == n_steps(SCENARIOS[0])
    assert names("lookahead 3")["_copy"] > 0 and len(r["lookahead 3"].ts.capture) == n_steps(SCENARIOS[0])
    assert names("validate in the middle")["rpn_losses_only"] == 2 * 3
    assert names("no crop-ahead")["head_crop"] == n_steps(SCENARIOS[0])
    # a buffer set first used by a pair (an nb = 2 base program) is later used by a lone batch, and the reverse
    order = collections.defaultdict(list)
    for o in r["stack_base pairs and lone batches"].trace:
        if o.name in ("upload_image", "upload_images"):
            order[o.slot].append(2 if o.name == "upload_images" else 1)
    as_text = {s: "".join(map(str, v)) for s, v in order.items()}
    assert any("21" in t for t in as_text.values()) and any("12" in t for t in as_text.values()), as_text
    # the un-announced batch went through the side-lane branch of step(); the replaced announcement dropped prepared batches
    assert len([o for o in r["announcement replaced"].trace if o.name == "base_forward"]) > n_steps(SCENARIOS[0])


# ------------------------------------------------------------------------------------------------ mutants
def after_sites():
    """{site: line} of every after(...) call in the functions of class TrainStep (after(...), eng.after(...) or self._after(...), the
    accessor the phases of step go through), named by function and argument."""
    sites, seen = {}, collections.Counter()
    for fn in trainstep_functions():
        src, first = inspect.getsourcelines(fn)
        tree = ast.parse(textwrap.dedent("".join(src)))
        calls = [c for c in ast.walk(tree) if isinstance(c, ast.Call) and
                 ((isinstance(c.func, ast.Name) and c.func.id == "after") or (isinstance(c.func, ast.Attribute) and c.func.attr in ("after", "_after")))]
        for c in sorted(calls, key=lambda c: c.lineno):
            key = "%s: after(%s)" % (fn.__name__, ast.unparse(c.args[0]))
            seen[key] += 1
            sites[key if seen[key] == 1 else "%s #%d" % (key, seen[key])] = first + c.lineno - 1
    return sites


# the after(...) call sites of step, its phases and flush (a repeated argument is numbered within its function)
AFTER_SITES = [
    "_current_state: after(self._head_done.get(slot))",        # un-announced batch, on its prefetch lane or on the one lane: in front of _launch_a
    "step: after(st.get('done'))",                             # current batch: in front of _launch_b
    "_prefetch: after(self._head_done.get(slot))",             # announced batch, prefetch lane: in front of _launch_a / _launch_pair
    "_prefetch: after(self._head_done.get(slot_b))",           # ... the pair's second buffer set
    "_prefetch: after(self._head_last)",                       # one lane: the head phase runs on the main lane
    "step: after(nxt['done'])",                                # announced batch: in front of _launch_b
    "_crop_ahead: after(self._head_done.get(st['slot']))",     # in front of crop-ahead
    "_head_phase: after(crop_ev)",                             # head lane: behind crop-ahead
    "flush: after(self._head_last)",
]
# after(...) calls of TrainStep that the audit does not reach, and why (lane_audit.py, SCOPE): found by after_sites() like the others, so
# that none can be added unseen, but no scenario runs them and no mutant takes them away
NOT_MODELLED = {
    "_native_head_exchange: after(ready)": "on the head communicator's stream of the data-parallel step; the scenarios are world size 1",
}
HOST_WAITS = {"host wait: anchor_targets_finish": "anchor_targets_finish", "host wait: roi_targets_finish": "roi_targets_finish",
              "host wait: losses()": "event.synchronize"}

# Ordering edges whose removal leaves every scenario race-free, and why.
REDUNDANT = {
    "_crop_ahead: after(self._head_done.get(st['slot']))":
        "ordered through the prefetch lane: the launch of phase A into this buffer set waited for the same event (the after in front of "
        "_launch_a / _launch_pair), and the main lane waited for that launch's `done` before _launch_b, long before crop-ahead",
}


def _mutant(site, sites):
    return dict(skip_site=sites[site]) if site in sites else dict(skip_wait=HOST_WAITS[site])


def test_the_after_sites_are_the_ones_the_audit_knows():
    from radnet_hip import trainer as T
    sites = after_sites()
    lines = inspect.getsource(T).splitlines()
    for key, line in sites.items():
        assert "after(" in lines[line - 1], (key, line, lines[line - 1])
    assert sorted(sites) == sorted(AFTER_SITES + list(NOT_MODELLED)), sorted(sites)
    assert set(REDUNDANT) <= set(AFTER_SITES) | set(HOST_WAITS)


def test_every_after_site_is_reached_by_some_scenario(clean_runs):
    hit = set().union(*(r.sites_hit for r in clean_runs.values()))
    assert {line for site, line in after_sites().items() if site not in NOT_MODELLED} <= hit


@pytest.mark.parametrize("site", AFTER_SITES + sorted(HOST_WAITS))
def test_each_ordering_edge_is_needed_or_declared_redundant(site):
    kw = _mutant(site, after_sites())
    found = None
    for scn in SCENARIOS:
        r = run(scn, **kw)
        if r.pairs:
            found = (scn.name, r.pairs)
            break
    if site in REDUNDANT:
        assert found is None, "%s is listed as redundant (%s), but without it '%s' has a race:\n%s" % (site, REDUNDANT[site], found[0], describe(found[1]))
    else:
        assert found is not None, "no scenario needs %s: a superfluous wait, or a gap in the scenarios -- remove it or list it in REDUNDANT with the reason" % site
        print("without %s, scenario '%s': %s" % (site, found[0], describe(found[1], limit=2)))
        res, a, b = found[1][0]
        assert a.slot is not None or b.slot is not None or res in LA.GLOBALS       # the report names the operations and the buffer set


# ------------------------------------------------------------------------------------------------ checker self-test
def test_checker_write_then_read_across_lanes_without_an_event_is_a_race():
    rec = Recorder()
    rec.op("side", "base_forward", writes={"F"})
    rec.op("main", "rpn_forward", reads={"F"}, writes={"pred"})
    pairs, examined = audit(rec.trace)
    assert examined == 1 and [(r, a.name, b.name) for r, a, b in pairs] == [("F", "base_forward", "rpn_forward")]


def test_checker_mark_and_after_order_the_two():
    rec = Recorder()
    rec.op("side", "base_forward", writes={"F"})
    ev = rec.mark("side")
    rec.op("side", "next base_forward", writes={"G"})
    rec.after("main", ev)
    rec.after("main", None)
    rec.op("main", "rpn_forward", reads={"F"}, writes={"pred"})
    assert audit(rec.trace) == ([], 1)
    rec.op("main", "reads too early", reads={"G"})              # the event covers what was enqueued BEFORE it, nothing later
    pairs, examined = audit(rec.trace)
    assert examined == 2 and [(r, a.name, b.name) for r, a, b in pairs] == [("G", "next base_forward", "reads too early")]


def test_checker_a_host_wait_orders_what_the_host_enqueues_afterwards():
    rec = Recorder()
    rec.op("head", "head_forward", writes={"det_l"})
    ev = rec.mark("head")
    ev.synchronize()
    rec.host_op("host reads", reads={"det_l"})
    rec.op("main", "adam", reads={"det_l"}, writes={"det_l"})   # enqueued after the wait: behind the head lane's write and the host's read
    assert audit(rec.trace) == ([], 3)
    rec2 = Recorder()
    rec2.skip_waits.add("event.synchronize")
    rec2.op("head", "head_forward", writes={"det_l"})
    rec2.mark("head").synchronize()
    rec2.host_op("host reads", reads={"det_l"})
    pairs, examined = audit(rec2.trace)
    assert examined == 1 and len(pairs) == 1
    rec3 = Recorder()                                           # a device-wide synchronise joins every lane
    rec3.op("head", "w", writes={"a"})
    rec3.op("side", "w", writes={"b"})
    rec3.device_sync()
    rec3.op("main", "r", reads={"a", "b"})
    assert audit(rec3.trace) == ([], 2)
