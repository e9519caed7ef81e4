"""The audit's stand-in (tests/lane_audit.py) is the engine's: the host-side happens-before check of tests/test_lane_audit_host.py is only as
good as AuditEngine, so the real FasterRCNNEngine runs two pipelined schedules ONCE each under a pass-through recorder and

  * the same batches and host decisions replayed through TrainStep on AuditEngine give the same sequence of calls, element by element:
    method, lane, buffer set, event made, event waited for;
  * every library call was made with the context of the lane it was enqueued on, on that lane's stream (no context -- split-K workspace,
    arrival counters, tuning table -- is ever current on two lanes);
  * every tensor reachable from the engine's plans has a name in the model (lane_audit.PLAN_FIELDS), two storage ranges overlap only if they
    are one model resource, no storage is shared between two buffer sets, and the lanes' workspaces are pairwise disjoint.

Nothing here runs a code path that test_prefetched_next_batch_equals_back_to_back_steps does not run."""
import collections

import numpy as np
import pytest
import torch

import lane_audit as LA

pytestmark = pytest.mark.gpu

PROGRAM_FIELDS = {"ops", "fwd", "refwd", "bwd", "bwd_parts", "bwd_dgrad", "bwd_wgrad", "chain_sub", "b1", "_wgrad_arr"}      # launch lists and descriptors


def _batches(n, nloc):
    from radnet_hip import synth
    out = []
    for i in range(n):
        b = []
        for j in range(nloc):
            meta = synth.synthetic_gt(40 + i * nloc + j, n=6, src_w=1000, src_h=600, smin=60, smax=300)
            b.append(dict(img=synth.synthetic_panel(30 + i * nloc + j, 300, 500), bboxes=meta["bboxes"], width=1000, height=600))
        out.append(b)
    return out


def _drive(ts, batches, lookahead):
    for k, b in enumerate(batches):
        ts.step(b, upcoming=batches[k + 1:k + 1 + lookahead])
    ts.flush()
    ts.losses()


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors(v)


def _storage(t):
    s = t.untyped_storage()
    return (t.device.type, s.data_ptr(), s.nbytes())


def census(eng, nloc):
    """Walk the engine's plans: {storage: {(buffer set, plan key, model resource)}}, and what went wrong on the way."""
    problems = []
    plans = [(k, dict.__getitem__(eng._plans, k)) for k in list(eng._plans.keys())]
    base_of = {}
    for k, plan in plans:
        if k[0] == "base":
            base_of[_storage(plan["F"])] = k

    def buffer_set(k, plan):
        if k[0] == "base":
            return k[-1]
        if k[0] in ("atgt", "rtgt"):
            return k[-1] // nloc
        if k[0] in ("rpn", "head"):
            hit = LA._base_slot(eng, k[3] if k[0] == "rpn" else k[4])
            return hit[0] if hit is not None else None
        return None

    owners = collections.defaultdict(set)
    n_tensors = 0
    for k, plan in plans:
        table = LA.PLAN_FIELDS.get(k[0])
        if table is None:
            problems.append("plan kind %r has no entry in the model" % (k[0],))
            continue
        bset = buffer_set(k, plan)
        if bset is None:
            problems.append("plan %r belongs to no buffer set" % (k,))
        named = {}

        def give(t, name, weak):
            st = _storage(t)
            if name.startswith("@base."):
                if st not in base_of:
                    problems.append("%r: field declared a reference to a base plan's buffer, but it is no base plan's" % (k,))
                return
            if st in named and weak:
                return
            named[st] = name
        # direct fields first: a storage found again under a container (keep, blocks[..]) keeps the name its own field gave it
        for weak in (False, True):
            for f, v in plan.items():
                if f in PROGRAM_FIELDS or not any(True for _ in _tensors(v)):
                    continue
                if f not in table:
                    if not weak:
                        problems.append("%r: field %r holds tensors the model has no name for" % (k, f))
                    continue
                if isinstance(v, torch.Tensor):
                    if not weak:
                        give(v, table[f], False)
                        n_tensors += 1
                elif weak:
                    sub = table[f]
                    for item in (v if isinstance(v, (list, tuple)) else [v]):
                        if isinstance(sub, dict):
                            for ff, vv in item.items():
                                for t in _tensors(vv):
                                    if ff not in sub:
                                        problems.append("%r: %s[..][%r] holds a tensor the model has no name for" % (k, f, ff))
                                    else:
                                        give(t, sub[ff], True)
                                        n_tensors += 1
                        else:
                            for t in _tensors(item):
                                give(t, sub, True)
                                n_tensors += 1
        for st, name in named.items():
            owners[st].add((bset, k, name))
    return owners, n_tensors, problems


@pytest.fixture(scope="module")
def recorded():
    from faster_rcnn.config import Config
    from oracle import dense
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.trainer import TrainStep
    C = Config()
    C.img_size = 300
    eng = FasterRCNNEngine(C)
    eng.set_weights(dense.init_params(seed=3))
    streams = {"main": eng.main_stream}
    ctx_name = {id(eng.ctx): "main"}
    for name, (cx, st) in eng._lanes.items():
        ctx_name[id(cx)] = name
        streams[name] = st
    ctx_lanes = collections.defaultdict(set)          # context -> lanes it was current on when a library call went through it
    bad = []

    def guard(cx, fn):
        def wrapper(*a, **kw):
            lane = LA.current_lane(eng)
            ctx_lanes[ctx_name[id(cx)]].add(lane)
            rebinding = "radnet_set_stream" in a[:2]          # Context.set_stream (graph capture): the handle changes right behind this check
            if cx is not eng.ctx or (not rebinding and torch.cuda.current_stream(eng.dev).cuda_stream != cx.stream_handle):
                bad.append(("library call through context %s while lane %s is current, or off that context's stream" % (ctx_name[id(cx)], lane), a[:2]))
            return fn(*a, **kw)
        return wrapper
    for cx in eng.contexts():
        cx.call, cx.check = guard(cx, cx.call), guard(cx, cx.check)

    def on_call(name, lane):
        if not torch.cuda.is_current_stream_capturing() and torch.cuda.current_stream(eng.dev) != streams[lane]:
            bad.append(("%s enqueued on lane %s, but that lane's stream is not current" % (name, lane),))
    trace = LA.CallTrace(eng, on_call=on_call)
    out = {"eng": eng, "bad": bad, "ctx_lanes": ctx_lanes}
    for tag, n, nloc, lookahead in (("one image, lookahead 3", 2 * TrainStep.NBUF + 5, 1, 3), ("batch 2 stacked", 6, 2, 3)):
        batches = _batches(n, nloc)
        trace.reset()
        np.random.seed(64)
        ts = TrainStep(eng)
        _drive(ts, batches, lookahead)
        torch.cuda.synchronize()
        real = list(trace.calls)
        labeller, rois = list(trace.labeller), list(trace.rois)
        owners, n_tensors, problems = census(eng, nloc)
        # the same batches and decisions through the stand-in
        model = LA.AuditEngine(n_side_lanes=eng.n_side_lanes, crop_ahead=eng.CROP_AHEAD, deferred_ok=any(c[0] == "head_update_deferred" for c in real), C=C)
        model.labeller_queue, model.roi_queue = collections.deque(labeller), collections.deque(rois)
        mtrace = LA.CallTrace(model)
        mts = model.bind(TrainStep(model))
        mts.stack_base, mts.batched, mts.crop_ahead = ts.stack_base, ts.batched, ts.crop_ahead
        _drive(mts, [[dict(img=s["img"], bboxes=s["bboxes"], width=s["width"], height=s["height"]) for s in b] for b in batches], lookahead)
        pairs, examined = LA.audit(model.rec.trace)
        out[tag] = dict(real=real, model=list(mtrace.calls), decisions=(labeller, rois), owners=owners, n_tensors=n_tensors, problems=problems,
                        pairs=pairs, examined=examined, stacked=ts.batched and nloc > 1)
        for s in range(2 * TrainStep.NBUF):           # the next run starts from an empty plan cache: its buffer sets are its own
            eng.release_slot(s)
    return out


RUNS = ["one image, lookahead 3", "batch 2 stacked"]


@pytest.mark.parametrize("run", RUNS)
def test_the_stand_in_makes_the_engines_calls_on_the_engines_lanes(recorded, run):
    r = recorded[run]
    real, model = r["real"], r["model"]
    print("%s: %d calls recorded, decisions %s" % (run, len(real), [collections.Counter(d) for d in r["decisions"]]))
    assert len(real) > 100 and {c[1] for c in real} >= {"main", "side", "head"}
    if run == "batch 2 stacked":
        assert r["stacked"] and any(c[0] == "rpn_backward_batched" for c in real)
    for i, (a, b) in enumerate(zip(real, model)):
        assert a == b, "call %d differs (method, lane, buffer set, event made, event waited for): engine %r, stand-in %r; before it %r" % (i, a, b, real[max(0, i - 3):i])
    assert len(real) == len(model)
    assert not r["pairs"], LA.describe(r["pairs"])       # and the replayed schedule itself is race-free
    assert r["examined"] > 0


def test_every_library_call_ran_on_its_lanes_context_and_stream(recorded):
    assert not recorded["bad"], recorded["bad"][:5]
    lanes = recorded["ctx_lanes"]
    print("contexts and the lanes they served:", dict(lanes))
    assert set(lanes) >= {"main", "side", "head"}
    for ctx, seen in lanes.items():
        assert seen == {ctx}, "context of lane %s was used while lanes %s were current" % (ctx, sorted(seen))


@pytest.mark.parametrize("run", RUNS)
def test_plan_buffers_alias_only_where_the_model_says_so(recorded, run):
    r, eng = recorded[run], recorded["eng"]
    owners = r["owners"]
    print("%s: %d plan tensors mapped onto %d storages" % (run, r["n_tensors"], len(owners)))
    assert not r["problems"], r["problems"][:10]
    assert r["n_tensors"] > 100
    for st, who in owners.items():
        assert len(who) == 1, "one storage, several model resources: %r" % (sorted(who, key=repr),)     # incl. two buffer sets: nothing in the plans is global
    ws = [("ws", eng.ws), ("ws2", eng.ws2), ("ws3", eng.ws3)] + [("ws of extra lane %d" % i, e[2]) for i, e in enumerate(eng._extra_lanes)]
    ranges = [(st[0], st[1], st[1] + st[2], sorted(who, key=repr)[0]) for st, who in owners.items()]
    ranges += [("cuda", w.untyped_storage().data_ptr(), w.untyped_storage().data_ptr() + w.untyped_storage().nbytes(), name) for name, w in ws]
    ranges.sort(key=lambda x: (x[0], x[1]))
    for a, b in zip(ranges, ranges[1:]):
        assert a[0] != b[0] or a[2] <= b[1], "storage ranges overlap: %r and %r" % (a[3], b[3])
    assert len({w.untyped_storage().data_ptr() for _, w in ws}) == 2 + eng.n_side_lanes
