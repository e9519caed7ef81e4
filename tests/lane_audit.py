"""Happens-before audit of the pipelined train step (trainer.TrainStep.step(batch, upcoming=[...])): a recording stand-in for the engine and
a checker over what it records.  Device-free.

A missing event wait between two lanes is a data race; running the schedule shows it only when timing happens to.  Here nothing runs: the
stand-in (AuditEngine) has the surface TrainStep touches, launches no kernel and appends (lane, name, reads, writes) over NAMED resources to
a trace, each entry stamped with a vector clock; audit(trace) returns every pair of accesses to one resource, at least one of them a write,
that the clocks leave unordered.

Clocks: one per lane ('main' = no lane() active, 'side', 'side1', ..., 'head') and one for the host.
    an operation enqueued on lane L:  L = join(L, host), tick L, the operation keeps a copy (nothing starts before the host enqueued it)
    mark():                           is itself enqueued; the event it returns holds a copy of L
    after(ev):                        L = join(L, ev) for what L enqueues later; after(None) does nothing, as in the engine
    ev.synchronize(), the host waits  host = join(host, ev); anchor_targets_finish / roi_targets_finish wait for the event recorded when
                                      the matching *_launch was enqueued, on the lane current then (P["event"].record() / .synchronize())
    a blocking copy (.cpu(), .to(dev) an operation on the current lane, then host = join(host, that lane)
      of pageable memory)
    device-wide synchronise           host = join(host, every lane)

SCOPE.  World size 1, launch-by-launch base forward (no chain kernel), no RADNET_COPY_STREAM.  Not modelled: the exchange lanes of the
data-parallel step (communicator streams, _native_head_exchange), the staging-buffer events inside upload_image / upload_images (raw_free,
raw_read: the pinned staging buffer and its host wait), the per-context workspaces (each belongs to one lane; tests/test_gpu_lane_audit.py
checks that on the real engine).  Ground-truth uploads (upload_gt) block the host on the lane they are issued on, as torch's pageable
`.to(dev)` does: a scenario that wants the worst case uploads them before the run (a training run sees its samples again and again).

Resources are named at the granularity at which the engine allocates them and keyed the way it keys its plans -- by buffer-set slot for
base / label / RoI-label plans, by the feature map's POINTER and nb / groups for RPN and classifier plans -- so an alias the engine has
(the one-image views of an nb = 2 base plan, a head plan found again through the same feature-map pointer) is an alias here too.

tests/test_lane_audit_host.py runs TrainStep's scenarios through this; tests/test_gpu_lane_audit.py ties the stand-in to FasterRCNNEngine
(same calls on the same lanes with the same event edges; every plan tensor has a name here; no unmodelled aliasing)."""
import collections
import contextlib
import types

import numpy as np
import torch

HOST = "host"


# ------------------------------------------------------------------------------------------------ clocks
def join(a, b):
    out = dict(a)
    for k, v in b.items():
        if v > out.get(k, 0):
            out[k] = v
    return out


def leq(a, b):
    """a happened before (or is) b."""
    return all(v <= b.get(k, 0) for k, v in a.items())


class Op:
    __slots__ = ("idx", "step", "lane", "name", "reads", "writes", "stamp", "slot")

    def __init__(self, idx, step, lane, name, reads, writes, stamp, slot):
        self.idx, self.step, self.lane, self.name, self.stamp, self.slot = idx, step, lane, name, stamp, slot
        self.reads, self.writes = frozenset(reads), frozenset(writes)

    def where(self):
        return "step %s, slot %s, lane %s: %s  clock %s" % (self.step, self.slot, self.lane, self.name, dict(sorted(self.stamp.items())))


class Event:
    def __init__(self, rec, clock, index):
        self._rec, self.clock, self.index = rec, clock, index

    def synchronize(self):
        self._rec.host_wait(self, "event.synchronize")


class Recorder:
    """The clocks and the trace.  AuditEngine drives one; the checker's self-test drives one by hand."""

    def __init__(self):
        self.trace = []
        self.clocks = collections.defaultdict(dict)        # lane -> clock
        self.host = {}
        self.step = None
        self.n_events = 0
        self.skip_waits = set()        # names of host waits that do NOT join the host clock (mutants)

    def op(self, lane, name, reads=(), writes=(), slot=None):
        c = join(self.clocks[lane], self.host)
        c[lane] = c.get(lane, 0) + 1
        self.clocks[lane] = c
        o = Op(len(self.trace), self.step, lane, name, reads, writes, dict(c), slot)
        self.trace.append(o)
        return o

    def host_op(self, name, reads=(), writes=(), slot=None):
        self.host = dict(self.host)
        self.host[HOST] = self.host.get(HOST, 0) + 1
        o = Op(len(self.trace), self.step, HOST, name, reads, writes, dict(self.host), slot)
        self.trace.append(o)
        return o

    def mark(self, lane):
        o = self.op(lane, "mark")
        self.n_events += 1
        return Event(self, dict(o.stamp), self.n_events - 1)

    def after(self, lane, ev):
        if ev is not None:
            self.clocks[lane] = join(self.clocks[lane], ev.clock)

    def host_wait(self, ev, name):
        if name not in self.skip_waits:
            self.host = join(self.host, ev.clock)

    def host_join_lane(self, lane):
        self.host = join(self.host, self.clocks[lane])

    def device_sync(self):
        for c in list(self.clocks.values()):
            self.host = join(self.host, c)


def audit(trace):
    """(pairs, examined): every pair of operations that access one resource, at least one of them writing, neither stamp <= the other --
    (resource, first, second), the Ops carrying stamp, step, slot and lane -- and the number of conflicting pairs examined across lanes or
    between a lane and the host (pairs on one lane are ordered by the lane and not counted)."""
    by_res = collections.defaultdict(list)
    for o in trace:
        for r in o.writes:
            by_res[r].append((o, True))
        for r in o.reads - o.writes:
            by_res[r].append((o, False))
    pairs, examined = [], 0
    for r, acc in by_res.items():
        for j in range(len(acc)):
            b, bw = acc[j]
            for i in range(j):
                a, aw = acc[i]
                if not (aw or bw) or a.lane == b.lane:
                    continue
                examined += 1
                if not leq(a.stamp, b.stamp) and not leq(b.stamp, a.stamp):
                    pairs.append((r, a, b))
    return pairs, examined


def describe(pairs, limit=6):
    """The races, for an assertion message: resource (its name carries the plan key, i.e. the buffer set) and both operations."""
    out = ["%d unordered conflicting pair(s)" % len(pairs)]
    for r, a, b in pairs[:limit]:
        out.append("  %s\n    %s\n    %s" % (r, a.where(), b.where()))
    return "\n".join(out)


# ------------------------------------------------------------------------------------------------ named tensors
_REG = {}          # storage pointer -> (engine, name, elements per sub-resource, formatter)


class NamedTensor(torch.Tensor):
    """A tiny CPU tensor that stands for a device buffer of the engine: TrainStep slices it, passes it back and reads its pointer as it
    does with the real one; .cpu() is the blocking device-to-host copy (a read on the current lane, then the host waits for that lane)."""

    def cpu(self):
        plain = self.as_subclass(torch.Tensor)
        ent = _REG.get(plain.untyped_storage().data_ptr())
        if ent is not None:
            ent[0]._blocking_read(plain)
        return plain.clone()


def _plain(t):
    return t.as_subclass(torch.Tensor) if isinstance(t, NamedTensor) else t


class _Arena:
    def __init__(self, name):
        self.name = name
        self.p = torch.zeros(8, dtype=torch.float64)
        self.g = torch.zeros(8, dtype=torch.float64)
        self.n = 8
        self.t = 0


class Prog(list):
    """A layer program of a plan (the engine's launch lists): empty, known by identity."""

    def __init__(self, plan_key, kind):
        super().__init__()
        self.plan_key, self.kind = plan_key, kind


def _feat_len(n):
    from radnet_hip import engine as E
    return E.feat_len(n)


# the globals of the model: what is NOT owned by one buffer set
W_BASE, W_RPN, W_HEAD = "W_base (frozen)", "W_rpn (+ rpn_conv1 Winograd filter)", "W_head (+ folded shifts, Winograd filters)"
G_RPN, G_HEAD, M_RPN, M_HEAD = "G_rpn (gradient arena)", "G_head (gradient arena)", "Adam moments rpn", "Adam moments head"
RPN_LOSSES, DET_LOSSES, LOSS_SCRATCH = "rpn_losses", "det_losses", "loss_scratch"
GLOBALS = (W_BASE, W_RPN, W_HEAD, G_RPN, G_HEAD, M_RPN, M_HEAD, RPN_LOSSES, DET_LOSSES, LOSS_SCRATCH)

# Every tensor-bearing field of an engine plan -> the model's resource of that plan (the census of tests/test_gpu_lane_audit.py walks the real
# plans with this table; a field that is missing here is a failure there).  "@base.F" / "@base.x": a reference to the buffer of the base plan
# the plan was built on, not a buffer of its own.
PLAN_FIELDS = {
    "base": {"x": "x", "F": "F", "keep": "act", "raw": "raw", "h_raw": "raw", "raws": "raw", "h_raws": "raw"},
    "atgt": {"valid": "valid", "overlap": "overlap", "regr": "regr", "ycls": "y", "yregr": "y", "h_valid": "h_maps", "h_overlap": "h_maps",
             "best": "scratch", "nfor": "scratch", "scratch": "scratch"},
    "rtgt": {"keep": "dev", "cls": "dev", "box": "dev", "t": "dev", "iou": "dev", "h_cls": "h_codes", "h_n": "h_codes", "sel": "sel", "h_sel": "h_sel"},
    "rpn": {"h": "h", "pred": "pred", "dz": "dz", "dh": "dh", "wino_keep": "wino", "prop_ws": "prop", "R": "prop", "Rp": "prop", "Rn": "prop",
            "images": {"pred": "pred", "dz": "dz", "prop_ws": "prop", "R": "prop", "Rp": "prop", "Rn": "prop"}},
    "head": {"rois": "rois", "pooled": "pooled", "y1": "y", "y2": "y", "live": "live", "F": "@base.F",
             "feat": "act", "pcls": "act", "pregr": "act", "y5": "act", "tail_scratch": "act", "dz": "dz",
             "dfeat": "g", "g_last": "g", "wg_scratch": "g", "keep": "act|g",
             "blocks": {"x": "act", "a": "act", "b": "act", "out": "act", "wino_v": "act", "g_out": "g", "g_a": "g", "g_b": "g"}},
}


class LaneClocks:
    """lane() / mark() / after() of the engine (engine.py:774-799) over a Recorder: mixed into any stand-in engine, its pipelined runs leave a trace to audit."""

    def _init_lanes(self, n_side_lanes):
        self.rec = Recorder()
        self.n_side_lanes = n_side_lanes
        self._lane = "main"
        self._lanes = ["side"] + ["side%d" % k for k in range(1, n_side_lanes)] + ["head"]

    @contextlib.contextmanager
    def lane(self, name):
        if name not in self._lanes:
            raise KeyError(name)
        prev, self._lane = self._lane, name
        try:
            yield
        finally:
            self._lane = prev

    def mark(self):
        return self.rec.mark(self._lane)

    def after(self, ev):
        self.rec.after(self._lane, ev)

    def _op(self, name, reads=(), writes=(), slot=None):
        return self.rec.op(self._lane, name, reads, writes, slot)


class AuditEngine(LaneClocks):
    """Stand-in for FasterRCNNEngine with exactly the surface TrainStep touches (plus what validate() needs).  No kernels: every method
    appends its reads and writes to rec.trace.  Host decisions are parameters: `script(width, height)` -> "fail" (the labeller raises),
    "skip" (no RoI kept) or "pick", asked when the image's labelling / RoI labelling is launched; `labeller_queue` / `roi_queue`, when set,
    are consumed in call order by the *_finish calls instead (replay of a real run's decisions)."""

    CROP_AHEAD = True
    supports_batched = True

    def __init__(self, n_side_lanes=2, script=None, deferred_ok=True, crop_ahead=True, C=None):
        self._init_lanes(n_side_lanes)
        self.CROP_AHEAD = crop_ahead
        self.deferred_ok = deferred_ok
        self.script = script or (lambda width, height: "pick")
        self.labeller_queue = self.roi_queue = None
        self.ctx = types.SimpleNamespace(timing_on=False)
        self.dev = "cpu"
        self.C = C or types.SimpleNamespace(class_mapping={"fg": 0, "bg": 1}, img_size=600, n_rois=4)       # (a real Config when a real run is replayed)
        self.bg = self.C.class_mapping["bg"]
        self.rpn_arena, self.head_arena = _Arena("rpn"), _Arena("head")
        self._plans = {}
        self._keep = []            # named tensors stay alive: their storage pointers are the registry's keys
        self._n_gt = 0
        self._head_shift_fresh = False

    # ---- plumbing
    def tensor(self, name, shape, unit=1, fmt=None, dtype=torch.float32):
        t = torch.zeros(shape, dtype=dtype)
        _REG[t.untyped_storage().data_ptr()] = (self, name, unit, fmt)
        self._keep.append(t)
        return t.as_subclass(NamedTensor)

    def res(self, t):
        """Resources a tensor (or a view of one) stands for; a tensor the model did not make (validate()'s private loss rows) has none."""
        if t is None:
            return set()
        t = _plain(t)
        ent = _REG.get(t.untyped_storage().data_ptr())
        if ent is None or ent[0] is not self:
            return set()
        _, name, unit, fmt = ent
        off, n = t.storage_offset(), max(t.numel(), 1)
        total = t.untyped_storage().nbytes() // t.element_size() // unit
        if total <= 1:
            return {name}
        return {fmt(name, i) if fmt else "%s[%d]" % (name, i) for i in range(off // unit, (off + n - 1) // unit + 1)}

    def bind(self, ts):
        """Name TrainStep's own device buffers: the loss rows _rpn_l[slot][i] / _det_l[slot][row]."""
        def fmt(name, i):
            return "%s[%d][%d]" % (name, i // 64, i % 64)
        ts._rpn_l = self.tensor("_rpn_l", tuple(ts._rpn_l.shape), unit=2, fmt=fmt)
        ts._det_l = self.tensor("_det_l", tuple(ts._det_l.shape), unit=3, fmt=fmt)
        self._ts = ts
        return ts

    def _blocking_read(self, t):
        # torch's .cpu(): a copy on the current stream, then the host waits for that stream; then the host reads the copy
        r = self.res(t)
        self._op("copy to host", reads=r)
        self.rec.host_join_lane(self._lane)
        self.rec.host_op("host reads", reads=r)

    @staticmethod
    def _n(key, field):
        return "%s%r.%s" % (key[0], tuple(key[1:]), field)

    def _slot_of_F(self, F):
        """Buffer set (base plan slot) and image a feature-map pointer belongs to."""
        p = _plain(F).data_ptr()
        for k, v in self._plans.items():
            if k[0] == "base":
                f = _plain(v["F"])
                if f.data_ptr() <= p < f.data_ptr() + f.numel() * f.element_size():
                    return k[-1]
        return None

    # ---- targets
    def upload_gt(self, boxes, isbg, cls):
        # engine.py:1517-1524 upload_gt: torch.from_numpy(...).to(dev) of pageable memory -- fresh device tensors, a blocking copy on the current lane
        self._n_gt += 1
        name = "gt#%d" % self._n_gt
        self._op("upload_gt", writes={name})
        self.rec.host_join_lane(self._lane)
        return dict(g=len(boxes), name=name)

    def anchor_targets_launch(self, gt, width, height, rw, rh, slot=0):
        # engine.py:1526-1553 anchor_targets_launch: radnet_anchor_targets reads the boxes and writes valid / overlap / regr / best / nfor / scratch;
        # two _copy launches fill the pinned h_valid / h_overlap; P["event"].record() on the current lane.  Plan key ("atgt", fh, fw, slot)
        fw, fh = _feat_len(rw), _feat_len(rh)
        key = ("atgt", fh, fw, slot)
        if key not in self._plans:
            self._plans[key] = dict(key=key, ycls=self.tensor(self._n(key, "y"), (1,)), yregr=self.tensor(self._n(key, "y"), (1,)))
        P = self._plans[key]
        n = lambda f: self._n(key, f)
        self._op("anchor_targets_launch", reads={gt["name"]}, writes={n("valid"), n("overlap"), n("regr"), n("scratch"), n("h_maps")}, slot=slot)
        P["event"] = self.rec.mark(self._lane)
        P["decision"] = self.script(width, height)
        return P

    def anchor_targets_finish(self, P):
        # engine.py:1555-1564 anchor_targets_finish: P["event"].synchronize(); subsample_valid reads h_valid / h_overlap and rewrites h_valid in place
        # (KeyError raised there, before anything is enqueued); _copy(valid <- h_valid); radnet_anchor_targets_pack reads valid / overlap /
        # regr and writes ycls / yregr
        key = P["key"]
        n = lambda f: self._n(key, f)
        self.rec.host_wait(P["event"], "anchor_targets_finish")
        dec = self.labeller_queue.popleft() if self.labeller_queue is not None else P["decision"]
        self.rec.host_op("host subsamples label maps", reads={n("h_maps")}, writes={n("h_maps")}, slot=key[-1])
        if dec == "fail":
            raise KeyError(3)
        self._op("anchor_targets_finish", reads={n("h_maps"), n("overlap"), n("regr")}, writes={n("valid"), n("y")}, slot=key[-1])
        return P["ycls"], P["yregr"], 0

    def roi_targets_launch(self, R, Rn, gt, width, height, rw, rh, n_max=300, slot=0):
        # engine.py:1580-1602 roi_targets_launch: radnet_roi_targets reads R, *Rn and the boxes, writes keep / cls / box / t / iou; two _copy launches
        # fill the pinned h_cls / h_n; P["event"].record().  Plan key ("rtgt", slot)
        key = ("rtgt", slot)
        P = self._plans.setdefault(key, dict(key=key))
        n = lambda f: self._n(key, f)
        self._op("roi_targets_launch", reads=self.res(R) | self.res(Rn) | {gt["name"]}, writes={n("dev"), n("h_codes")}, slot=slot)
        P["event"] = self.rec.mark(self._lane)
        P["decision"] = self.script(width, height)
        return P

    def roi_targets_finish(self, P):
        # engine.py:1604-1610 roi_targets_finish: P["event"].synchronize(), then the host reads h_n and h_cls
        key = P["key"]
        self.rec.host_wait(P["event"], "roi_targets_finish")
        self.rec.host_op("host reads RoI class codes", reads={self._n(key, "h_codes")}, slot=key[-1])
        dec = self.roi_queue.popleft() if self.roi_queue is not None else P["decision"]
        if dec == "skip":
            return P, np.zeros(0, dtype=np.int32), 0
        return P, np.array([0, self.bg, 0, self.bg, self.bg, 0], dtype=np.int32), 6

    def roi_targets(self, R, Rn, gt, width, height, rw, rh, n_max=300):
        return self.roi_targets_finish(self.roi_targets_launch(R, Rn, gt, width, height, rw, rh, n_max))      # validate(): slot 0, as the engine

    # ---- base
    def _plan_base(self, nb, H, W, slot):
        key = ("base", nb, H, W, slot)
        if key not in self._plans:
            n = lambda f: self._n(key, f)
            self._plans[key] = dict(key=key, x=self.tensor(n("x"), (nb, 1)), F=self.tensor(n("F"), (nb, 1)), fh=_feat_len(H), fw=_feat_len(W), nb=nb,
                                    ops=Prog(key, "ops"))
        return self._plans[key]

    def upload_image(self, img, slot=0):
        # engine.py:871-909 upload_image: _copy(raw <- pinned staging), radnet_preprocess_bgr reads raw and writes x.  Plan key ("base", 1, H, W, slot)
        H, W = img.shape[:2]
        plan = self._plan_base(1, H, W, slot)
        self._op("upload_image", writes={self._n(plan["key"], "raw")} | self.res(plan["x"]), slot=slot)
        return plan

    def upload_images(self, imgs, slot=0):
        # engine.py:911-936 upload_images: per image _copy(raws[i] <- staging) and radnet_preprocess_bgr into x[i].  Plan key ("base", nb, H, W, slot)
        H, W = imgs[0].shape[:2]
        plan = self._plan_base(len(imgs), H, W, slot)
        self._op("upload_images", writes={self._n(plan["key"], "raw")} | self.res(plan["x"]), slot=slot)
        return plan

    def base_forward(self, plan):
        # engine.py:947-949 base_forward (program: _plan_base, 611-665): _run(plan["ops"]) -- reads x and the frozen weights, writes every intermediate buffer (keep) and F
        key = plan["key"]
        self._op("base_forward", reads=self.res(plan["x"]) | {W_BASE}, writes={self._n(key, "act")} | self.res(plan["F"]), slot=key[-1])
        return plan["F"]

    # ---- RPN
    def _plan_rpn(self, fh, fw, F, nb=1):
        key = ("rpn", fh, fw, _plain(F).data_ptr(), nb)          # engine.py:954 _plan_rpn: keyed by the feature map's pointer
        if key not in self._plans:
            n = lambda f: self._n(key, f)

            def props(tag):
                return dict(R=self.tensor(n("prop" + tag), (1,)), Rn=self.tensor(n("prop" + tag), (1,)))
            plan = dict(key=key, F=F, nb=nb, fh=fh, fw=fw, fwd=Prog(key, "fwd"), refwd=Prog(key, "refwd"), bwd=Prog(key, "bwd"),
                        pred=self.tensor(n("pred"), (nb,)), dz=self.tensor(n("dz"), (nb,)), **props(""))
            if nb > 1:          # engine: per-image views of pred / dz, own proposal buffers per image
                plan["images"] = [dict(key=key, pred=plan["pred"][i:i + 1], dz=plan["dz"][i:i + 1], fh=fh, fw=fw, **props("[%d]" % i)) for i in range(nb)]
            self._plans[key] = plan
        return self._plans[key]

    def _rpn_slot(self, rp):
        return self._slot_of_F(self._plans[rp["key"]]["F"])

    def _rpn_fwd(self, rp, name, first):
        # engine.py:964-965, 993-994 _plan_rpn fwd / refwd (run by rpn_forward, 1007-1010): rpn_conv1 (Winograd: the input transform V is written by fwd and only read by refwd) and the fused
        # heads read F, V and the RPN weights and write h and pred
        n = lambda f: self._n(rp["key"], f)
        reads = {W_RPN} | ({n("wino.V")} if not first else self.res(rp["F"]))
        self._op(name, reads=reads, writes={n("h")} | self.res(rp["pred"]) | ({n("wino.V")} if first else set()), slot=self._rpn_slot(rp))

    def rpn_forward(self, bplan):
        rp = self._plan_rpn(bplan["fh"], bplan["fw"], bplan["F"], bplan.get("nb", 1))
        self._rpn_fwd(rp, "rpn_forward", True)
        return rp

    @staticmethod
    def rpn_image(rp, i):
        return rp["images"][i] if rp.get("nb", 1) > 1 else rp

    def _rpn_loss(self, name, v, ycls, yregr, loss_out):
        # radnet_rpn_loss (engine.py:1045-1048 rpn_backward, 1017-1026 rpn_loss_image, 1031-1035 rpn_losses_only): reads pred and the packed targets, writes dz, the loss
        # row (rpn_losses when none is given) and loss_scratch
        out = self.res(loss_out) if loss_out is not None else {RPN_LOSSES}
        self._op(name, reads=self.res(v["pred"]) | self.res(ycls) | self.res(yregr), writes=self.res(v["dz"]) | out | {LOSS_SCRATCH},
                 slot=self._rpn_slot(v))

    def _rpn_bwd(self, rp, name):
        # engine.py:967-990 _plan_rpn bwd (run by rpn_backward 1049, rpn_backward_batched 1028-1029): wgrad / colsum / dgrad of the heads (read dz, h; write dh), Winograd-domain wgrad of rpn_conv1 (reads V, dh;
        # writes dZ, dU); every weight gradient goes into the RPN gradient arena
        n = lambda f: self._n(rp["key"], f)
        self._op(name, reads=self.res(rp["dz"]) | {n("h"), n("wino.V"), W_RPN, G_RPN}, writes={n("dh"), n("wino.dZdU"), G_RPN}, slot=self._rpn_slot(rp))

    def rpn_backward(self, rp, ycls, yregr, loss_out=None):
        self._rpn_loss("rpn_backward: loss", rp, ycls, yregr, loss_out)
        self._rpn_bwd(rp, "rpn_backward: program")

    def rpn_loss_image(self, rp, i, ycls, yregr, loss_out=None):
        v = self.rpn_image(rp, i)
        if ycls is None:      # engine.py:1022-1024 rpn_loss_image: radnet_fill_zero on the image's dz rows
            self._op("rpn_loss_image: zero rows", writes=self.res(v["dz"]), slot=self._rpn_slot(rp))
            return
        self._rpn_loss("rpn_loss_image", v, ycls, yregr, loss_out)

    def rpn_backward_batched(self, rp):
        self._rpn_bwd(rp, "rpn_backward_batched")

    def rpn_losses_only(self, rp, ycls, yregr, loss_out=None):
        self._rpn_loss("rpn_losses_only", rp, ycls, yregr, loss_out)

    def _run(self, ops):
        # trainer.py _rpn_phase / engine.py:801-834 _run: TrainStep runs one program itself, the re-prediction after Adam #1 (rp["refwd"], or rp["fwd"] without one)
        rp = self._plans[ops.plan_key]
        if ops.kind not in ("fwd", "refwd"):
            raise AssertionError("TrainStep ran a program the model does not expect: %s" % ops.kind)
        self._rpn_fwd(rp, "_run(%s)" % ops.kind, ops.kind == "fwd")

    def proposals(self, rp, overlap_thresh=0.7, max_boxes=300):
        # engine.py:1142-1149 proposals: radnet_rpn_to_roi reads pred (of the image) and writes R / Rp / Rn / prop_ws of that image
        self._op("proposals", reads=self.res(rp["pred"]), writes=self.res(rp["R"]), slot=self._rpn_slot(rp))
        return rp["R"], rp["Rn"]

    # ---- optimizer
    from radnet_hip.program import set_accumulate
    set_accumulate = staticmethod(set_accumulate)      # the real one: a host-side edit of the (here empty) launch list

    def adam(self, arena, grad_scale=1.0, zero_grad=True):
        # engine.py:1051-1099 adam / _adam_launch: reads and clears the gradient arena, updates weights and moments; in the same launch (or right behind it
        # on the same lane) the derived state -- rpn_conv1's Winograd filter; the head's folded shifts and 3x3 Winograd filters
        arena.t += 1
        if arena is self.head_arena:
            self._head_shift_fresh = True
            self._op("adam(head)", reads={W_HEAD, G_HEAD, M_HEAD}, writes={W_HEAD, G_HEAD, M_HEAD})
        else:
            self._op("adam(rpn)", reads={W_RPN, G_RPN, M_RPN}, writes={W_RPN, G_RPN, M_RPN})

    def refresh_head_shift(self, force=False):
        # engine.py:439-448 refresh_head_shift: nothing right after adam(head); else radnet_affine_vec reads the biases and rewrites the folded shifts
        fresh, self._head_shift_fresh = self._head_shift_fresh, False
        if not fresh or force:
            self._op("refresh_head_shift", reads={W_HEAD}, writes={W_HEAD})

    def _copy(self, dst, src):
        # engine.py:850-860 _copy: radnet_copy_bytes on the current lane (TrainStep._log_losses: loss rows into the loss log)
        if not self.res(dst):
            log = getattr(self._ts, "_loss_log", None)
            if log is not None and _plain(dst).untyped_storage().data_ptr() == log.untyped_storage().data_ptr():
                _REG[log.untyped_storage().data_ptr()] = (self, "_loss_log", 5, None)
                self._keep.append(log)
        if not self.res(dst) or not self.res(src):
            raise AssertionError("_copy between tensors the model has no name for")
        ent = _REG.get(_plain(src).untyped_storage().data_ptr())
        slot = _plain(src).storage_offset() // (64 * ent[2]) if ent[1] in ("_rpn_l", "_det_l") else None      # a loss row: [slot][64][unit]
        self._op("_copy", reads=self.res(src), writes=self.res(dst), slot=slot)

    # ---- classifier
    def _plan_head(self, R, fh, fw, F, training=True, groups=1):
        key = ("head", R, fh, fw, _plain(F).data_ptr(), groups)      # engine.py:1251 _plan_head: keyed by the feature map's pointer and groups
        if key not in self._plans:
            self._plans[key] = dict(key=key, F=F, R=R, groups=groups, bwd=Prog(key, "bwd"), live_host=[1] * groups)
        return self._plans[key]

    def _hn(self, hp, field, group=None):
        return self._n(hp["key"], field if group is None or hp["groups"] == 1 else "%s[%d]" % (field, group))

    def _hall(self, hp, field):
        return {self._hn(hp, field, g) for g in range(hp["groups"])}

    def _head_slot(self, hp):
        return self._slot_of_F(hp["F"])

    def pack_roi_batch(self, P, sel, hp, group=0):
        # engine.py:1612-1623 pack_roi_batch: the host writes the pinned h_sel; radnet_roi_batch_pack reads it (mapped) with cls / box / t of the RoI
        # plan and writes the group's rows of rois, y1, y2
        pk = P["key"]
        self.rec.host_op("host writes selection", writes={self._n(pk, "h_sel")}, slot=pk[-1])
        self._op("pack_roi_batch", reads={self._n(pk, "h_sel"), self._n(pk, "dev")}, writes={self._hn(hp, "rois", group), self._hn(hp, "y", group)},
                 slot=self._head_slot(hp))

    def idle_roi_group(self, hp, group):
        # engine.py:1625-1629 idle_roi_group: torch.tensor(..., device=dev) is a blocking upload on the current lane, then a device copy into the rows
        self._op("idle_roi_group", writes={self._hn(hp, "rois", group)}, slot=self._head_slot(hp))
        self.rec.host_join_lane(self._lane)

    def head_crop(self, hp):
        # engine.py:1402-1411 head_crop: radnet_roi_resize_fwd reads the feature map(s) and rois, writes pooled
        self._op("head_crop", reads=self.res(hp["F"]) | self._hall(hp, "rois"), writes={self._hn(hp, "pooled")}, slot=self._head_slot(hp))

    def head_forward(self, hp, training=False, loss_out=None, group_live=None, cropped=False):
        # engine.py:1413-1440 head_forward: head_crop unless cropped; _run(fwd) reads pooled and the head weights (kernels, folded shifts, Winograd filters)
        # and writes the stage-5 activations (with the kept V); the fused tail reads y1 / y2 / live and writes feat, pcls, pregr, dz, the loss
        # rows and tail_scratch; a changed live mask is a blocking host-to-device copy first
        if not cropped:
            self.head_crop(hp)
        slot = self._head_slot(hp)
        flags = [1] * hp["groups"] if group_live is None else [1 if f else 0 for f in group_live]
        if training and loss_out is not None and flags != hp["live_host"]:
            self._op("head_forward: live mask", writes={self._hn(hp, "live")}, slot=slot)
            self.rec.host_join_lane(self._lane)
            hp["live_host"] = flags
        out = self.res(loss_out) if loss_out is not None else set()
        self._op("head_forward", reads={self._hn(hp, "pooled"), W_HEAD, self._hn(hp, "live")} | self._hall(hp, "y"),
                 writes={self._hn(hp, "act"), self._hn(hp, "dz")} | out, slot=slot)

    def head_losses_only(self, hp, loss_out=None):
        self.head_forward(hp, training=True, loss_out=loss_out)

    def head_deferred_ok(self, hp):
        return self.deferred_ok      # engine.py:1442-1447: a property of the plan and the library's settings, no device work

    def head_backward(self, hp, accumulate=False, loss_out=None, on_part=None, defer_wgrad=False):
        # engine.py:1480-1514 head_backward (fused tail: no loss pass): radnet_dense_heads_bwd reads feat / dz and adds the dense gradients into the
        # arena, writes dfeat; radnet_avgpool_bwd_relu; then bwd (data + weight gradients into the arena, Winograd wgrad scratch) or, deferred,
        # bwd_dgrad (data gradients only)
        if on_part is not None:
            raise AssertionError("bucketed exchange: outside the model's scope (world size 1)")
        self._op("head_backward" + (" (data gradients)" if defer_wgrad else ""),
                 reads={self._hn(hp, "act"), self._hn(hp, "dz"), W_HEAD, G_HEAD}, writes={self._hn(hp, "g"), G_HEAD}, slot=self._head_slot(hp))

    def head_update_deferred(self, hp, grad_scale=1.0):
        # engine.py:1449-1478 head_update_deferred: radnet_conv_wgrad_multi reads the activations and every layer's dy and applies Adam #2 to the kernels;
        # radnet_adam_step_tail: Adam over the arena's tail, folded shifts, Winograd filters
        self.head_arena.t += 1
        self._op("head_update_deferred", reads={self._hn(hp, "act"), self._hn(hp, "g"), W_HEAD, G_HEAD, M_HEAD}, writes={W_HEAD, G_HEAD, M_HEAD},
                 slot=self._head_slot(hp))

    # ---- validate()
    def release_slot(self, slot):
        # engine.py:707-724 release_slot -> 750-764 _evict_plan: torch.cuda.synchronize, then the plans of the buffer set go
        self.rec.device_sync()
        fptrs = {_plain(v["F"]).data_ptr() for k, v in self._plans.items() if k[0] == "base" and k[-1] == slot}
        for k in [k for k in self._plans if (k[0] in ("base", "atgt", "rtgt") and k[-1] == slot) or (k[0] in ("rpn", "head") and k[-2] in fptrs)]:
            del self._plans[k]


def current_lane(eng):
    """Name of the lane whose context is current on a real engine ('main': none) -- or the stand-in's."""
    if isinstance(eng, LaneClocks):
        return eng._lane
    for name, (ctx, _) in eng._lanes.items():
        if ctx is eng.ctx:
            return name
    return "main"


# ------------------------------------------------------------------------------------------------ call traces (both engines)
TRAINSTEP_SURFACE = ("upload_gt", "anchor_targets_launch", "anchor_targets_finish", "upload_image", "upload_images", "base_forward", "rpn_forward",
                     "rpn_backward", "rpn_loss_image", "rpn_backward_batched", "adam", "refresh_head_shift", "_run", "_copy", "proposals",
                     "roi_targets_launch", "roi_targets_finish", "pack_roi_batch", "idle_roi_group", "head_crop", "head_forward", "head_backward",
                     "head_update_deferred", "mark", "after")


def _plan_items(eng):
    return [(k, dict.__getitem__(eng._plans, k)) for k in list(eng._plans.keys())]


def _base_slot(eng, ptr):
    for k, v in _plan_items(eng):
        if k[0] == "base":
            f = _plain(v["F"])
            if f.data_ptr() <= ptr < f.data_ptr() + f.numel() * f.element_size():
                return (k[-1], (ptr - f.data_ptr()) // (f[0].numel() * f.element_size()))
    return None


def call_slot(eng, args, kwargs):
    """Buffer set a call works on, by the same rule on both engines: the slot argument, or the plan among the arguments -- a label / RoI-label
    plan by its key, anything built on a feature map as (slot of the base plan, image) that the feature map's pointer lies in."""
    if "slot" in kwargs:
        return kwargs["slot"]
    for a in args:
        if not isinstance(a, dict):
            continue
        if "F" in a:
            return _base_slot(eng, _plain(a["F"]).data_ptr())
        for k, v in _plan_items(eng):
            if v is a or any(im is a for im in (v.get("images") or []) if k[0] == "rpn"):
                return _base_slot(eng, k[3]) if k[0] == "rpn" else k[-1]
    return None


class CallTrace:
    """Pass-through recorder over an engine's TrainStep-facing methods: (method, lane, slot, event made, event waited for) per top-level call,
    and the host decisions in call order.  Events are numbered in the order they are made (mark() and the *_launch calls)."""

    def __init__(self, eng, on_call=None):
        self.eng, self.on_call = eng, on_call
        self._depth = 0
        self.reset()
        for name in TRAINSTEP_SURFACE:
            setattr(eng, name, self._wrap(name, getattr(eng, name)))

    def reset(self):
        """A new run: empty trace, events numbered from 0."""
        self.calls, self.labeller, self.rois = [], [], []
        self._ev, self._alive, self._n_ev = {}, [], 0

    def _new_event(self, obj):
        self._ev[id(obj)] = self._n_ev
        self._alive.append(obj)
        self._n_ev += 1
        return self._n_ev - 1

    def _wrap(self, name, fn):
        def wrapper(*args, **kwargs):
            if self._depth:
                return fn(*args, **kwargs)
            made = waited = None
            if name == "after":
                waited = self._ev[id(args[0])] if args[0] is not None else None
            elif name.endswith("_finish"):
                waited = self._ev[id(args[0])]
            slot = call_slot(self.eng, args, kwargs)
            lane = current_lane(self.eng)
            if self.on_call is not None:
                self.on_call(name, lane)
            self._depth += 1
            try:
                out = fn(*args, **kwargs)
            except KeyError:
                if name == "anchor_targets_finish":
                    self.labeller.append("fail")
                    self.calls.append((name, lane, slot, made, waited))
                raise
            finally:
                self._depth -= 1
            if name == "mark" or name.endswith("_launch"):
                made = self._new_event(out)
            if slot is None:
                slot = call_slot(self.eng, args, kwargs)         # the plan was made by this call
            if name == "anchor_targets_finish":
                self.labeller.append("pick")
            elif name == "roi_targets_finish":
                self.rois.append("skip" if out[2] <= 0 or not (np.asarray(out[1]) >= 0).any() else "pick")
            self.calls.append((name, lane, slot, made, waited))
            return out
        return wrapper
