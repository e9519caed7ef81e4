"""Layer programs: the op vocabulary, the passes that rewrite a program, and its translation into `radnet_op[]`.

A program is a Python list of `(kind, payload)` pairs -- the static launch list the engine lays out once per input size.  The
payload of a conv kind is a `radnet_conv_desc` (lib.ConvDesc), of `chain` the handle of a built chain, of every other kind a
sequence whose fields KINDS names in order.  `compile` turns a program into the array that radnet_program_run and the composed
entry points (radnet_rpn_forward / radnet_predict_tile / radnet_train_step) execute; include/radnet_hip.h documents the slots.

Nothing here needs a device, torch or an engine: the module imports ctypes and radnet_hip.lib only (the bf16 kinds ask the
library's host-side radnet_*_pick_split functions for their splits when they are compiled).
"""
import collections
import ctypes as C

from . import lib as L

PRECISIONS = ("fp32", "bf16", "bf16-mixed", "bf16-train")     # FasterRCNNEngine(precision=...)
MIXED_PRECISIONS = ("bf16-mixed", "bf16-train")      # trainable bf16 modes: bf16 forward convs, fp32 masters and Adam

# ---------------------------------------------------------------------------------------------- the op vocabulary
DESC, HANDLE = "desc", "handle"       # payloads that are not sequences: a radnet_conv_desc (copied into op.conv) / a radnet_chain*
Kind = collections.namedtuple("Kind", "code fields p i mode")


def _kind(code, fields=DESC, p="", i="", mode=None):
    """One row of KINDS.  fields: the payload's field names in order; p / i: which of them go to p[0], p[1], ... / i[0], i[1], ... of
    the radnet_op.  mode: where the kind keeps its gradient write mode -- an attribute of the descriptor or a field of the sequence --
    or None for a kind that writes no parameter gradient.  Field names are kept as payload positions."""
    if fields in (DESC, HANDLE):
        return Kind(code, fields, (), (), mode)
    fields = tuple(fields.split())
    at = fields.index
    return Kind(code, fields, tuple(at(f) for f in p.split()), tuple(at(f) for f in i.split()), None if mode is None else at(mode))


_WINO = dict(fields="x nb h w c n V U M T scale shift act y ldy form", p="x V U M scale shift y", i="nb h w c n T act ldy form")
KINDS = {
    "conv": _kind(L.OP_CONV_FWD),
    "dgrad": _kind(L.OP_CONV_DGRAD),
    "wgrad": _kind(L.OP_CONV_WGRAD, mode="dw_accumulate"),            # followed by the dgrad of the same descriptor: OP_CONV_BWD
    "conv_pair_first": _kind(L.OP_CONV_FWD_PAIR),                     # branch2a + shortcut conv of a conv_block: one call, the second
    "conv_pair_second": _kind(L.OP_NOP),                              # descriptor rides in the following NOP slot
    "bneck_first": _kind(L.OP_CONV_BNECK),                            # 3x3 + 1x1 expand (+ next 1x1 reduce): one call, the other
    "bneck_second": _kind(L.OP_NOP),                                  # descriptors ride in the NOP slots behind; i[0] = a third follows
    "bneck_third": _kind(L.OP_NOP),
    "conv_bf16": _kind(L.OP_CONV_FWD_BF16),                           # p[0] / i[0]: the layer's bf16 image and its pitch, i[1]: the K split
    "dgrad_bf16": _kind(L.OP_CONV_DGRAD_BF16),                        # p[0] / i[0]: the layer's dgrad image, i[1]: the split of (tap, n)
    "wgrad_bf16": _kind(L.OP_CONV_WGRAD_BF16, mode="dw_accumulate"),  # i[1]: the split of the pixels
    "maxpool": _kind(L.OP_MAXPOOL, "x y nb h w c k stride", p="x y", i="nb h w c k stride"),
    "colsum": _kind(L.OP_COLSUM, "g m n ld gscale out accumulate", p="g gscale out", i="m n ld accumulate", mode="accumulate"),
    "wino": _kind(L.OP_WINO, **_WINO),
    "wino_reuse": _kind(L.OP_WINO_REUSE, **_WINO),                    # V already holds this input's transform
    "wino_wgrad": _kind(L.OP_WINO_WGRAD, "dy nb h w c n ld_dy V dZ dU T dw ldw form gscale mode", p="dy V dZ dU dw gscale",
                        i="nb h w c n ld_dy T ldw mode form", mode="mode"),
    "scatter": _kind(L.OP_SCATTER, "src nb oh ow c stride h w mask dst", p="src mask dst", i="nb oh ow c stride h w"),
    "roi_bwd": _kind(L.OP_ROI_BWD, "dy h w c rois r ps dF", p="dy rois dF", i="h w c r ps"),
    "fill0": _kind(L.OP_FILL0, "dst nbytes", p="dst"),                # i[0] / i[1]: the low / high 32 bits of nbytes
    "relu_mask": _kind(L.OP_RELU_MASK, "g act n", p="g act"),         # i[0] / i[1]: the low / high 32 bits of n
    "chain": _kind(L.OP_CHAIN, HANDLE),
}
MUTABLE = ("colsum", "wino_wgrad")     # their write mode is edited in place (set_accumulate): the payload is a list


def _constructor(kind):
    fields = KINDS[kind].fields
    record = list if kind in MUTABLE else collections.namedtuple(kind, fields)._make

    def make(**kw):
        if sorted(kw) != sorted(fields):
            raise TypeError("%s(%s) got %s" % (kind, ", ".join(fields), ", ".join(sorted(kw))))
        return kind, record([kw[f] for f in fields])
    make.__name__ = kind
    make.__doc__ = "The op (%r, payload) with the payload's fields in the order KINDS states: %s." % (kind, ", ".join(fields))
    return make


maxpool, colsum, wino, wino_wgrad, scatter, roi_bwd, fill0, relu_mask = (
    _constructor(k) for k in ("maxpool", "colsum", "wino", "wino_wgrad", "scatter", "roi_bwd", "fill0", "relu_mask"))


def wino_reuse(op):
    """The Winograd layer of `op` (a wino op) on the transformed input its run left in V."""
    return "wino_reuse", op[1]


# ---------------------------------------------------------------------------------------------- gradient write modes
def _kind_of(kind):
    try:
        return KINDS[kind]
    except KeyError:
        raise L.RadnetError("unknown op " + kind) from None


def write_mode(kind, p):
    """The gradient write mode of an op (0 overwrite, 1 add, 2 overwrite a slice the caller zeroed), None for a kind without one."""
    at = _kind_of(kind).mode
    if at is None:
        return None
    return getattr(p, at) if isinstance(at, str) else p[at]


def set_write_mode(kind, p, v):
    at = _kind_of(kind).mode
    if at is None:
        return
    if isinstance(at, str):
        setattr(p, at, v)
    else:                                  # radnet_colsum knows add / overwrite only: into a slice the caller zeroed it adds
        p[at] = (1 if v else 0) if kind == "colsum" else v


def set_accumulate(ops, flag, prezeroed=False):
    """Gradient write mode of a backward program: flag=False -> overwrite (self-contained; each split wgrad /
    colsum zeroes its own slice), flag=True -> add.  prezeroed=True with flag=False: the caller zeroed the whole
    arena with ONE memset, so the ~25 per-layer memsets disappear (dw_accumulate = 2)."""
    v = 1 if flag else (2 if prezeroed else 0)
    for kind, p in ops:
        set_write_mode(kind, p, v)


_MODE_AT = {kind: row.mode for kind, row in KINDS.items()}      # KINDS' mode column alone: mode_key runs once per program run


def mode_key(ops):
    """The write modes of a program, in order: with the list's identity, the key of its compiled array and of its recorded hipGraphs
    (set_accumulate edits the payloads in place; both hold copies).  A colsum's mode is a function of the flag pair set_accumulate
    also gives the weight gradients of its program, so it splits no two programs their weight gradients do not split already."""
    try:
        return tuple([getattr(p, at) if at.__class__ is str else p[at] for kind, p in ops for at in (_MODE_AT[kind],) if at is not None])
    except KeyError as e:
        raise L.RadnetError("unknown op %s" % e.args[0]) from None


# ---------------------------------------------------------------------------------------------- passes
def fuse_bottlenecks(ops):
    """3x3 conv (64 -> 64 channels) + the 1x1 expand on its output (+ the next block's 1x1 reduce on THAT output) -> one
    radnet_conv_bottleneck call: the 3x3's output and the expand's re-read never touch memory.  Only where the 3x3 output has no other
    reader in the list (it is not written any more) -- stage 2 of nn_base (resnet50.py:197-199)."""
    def conv(i):
        return ops[i][1] if i < len(ops) and ops[i][0] == "conv" else None

    def reads(d, ptr):
        return ptr in (getattr(d, "x", None), getattr(d, "addend", None))

    out, k = [], 0
    while k < len(ops):
        db, dc = conv(k), conv(k + 1)
        ok = (db is not None and dc is not None and db.kh == 3 and db.stride == 1 and db.n == 64 and db.c % 32 == 0 and not db.addend and db.act == 1
              and dc.kh == 1 and dc.stride == 1 and dc.x == db.y and dc.c == 64 and dc.n % 64 == 0 and dc.act == 1)
        if ok:                                  # nobody else may read the tensor that is no longer written
            ok = not any(reads(p, db.y) for j, (kind, p) in enumerate(ops) if j != k + 1 and kind in ("conv", "conv_pair_first", "conv_pair_second"))
            ok = ok and not any(kind in ("wino", "wino_reuse") and p[0] == db.y for kind, p in ops)
        if not ok:
            out.append(ops[k])
            k += 1
            continue
        da = conv(k + 2)
        if da is not None and not (da.kh == 1 and da.stride == 1 and da.x == dc.y and da.c == dc.n and da.n == 64 and not da.addend and da.act == 1):
            da = None
        out += [("bneck_first", db), ("bneck_second", dc)] + ([("bneck_third", da)] if da is not None else [])
        k += 3 if da is not None else 2
    return out


def fuse_bias_grads(ops):
    """A bias-gradient column sum right after the wgrad of the same layer (same dy, pitch and scale) moves into
    that wgrad launch (radnet_conv_desc.db): 12 launches of ~7 us less per train step."""
    out = []
    for kind, p in ops:
        if kind == "colsum" and out and out[-1][0] == "wgrad":
            d = out[-1][1]
            g, m, n, ld, gs, db, _ = p
            if d.dy == g and d.ld_dy == ld and d.n == n and (d.gscale or None) == (gs or None) and d.nb * d.oh * d.ow == m:
                d.db = db
                continue
        out.append((kind, p))
    return out


def bf16_forward(ops, precision, fwd_image):
    """bf16 / bf16-mixed / bf16-train: every direct forward conv whose input has a multiple of 8 channels -> ("conv_bf16", desc); the
    4-channel stem stays fp32.  fwd_image(weight pointer) makes the layer's bf16 image if it does not exist yet.  fp32: `ops` unchanged."""
    if precision == "fp32":
        return ops
    out = []
    for kind, p in ops:
        if kind == "conv" and p.c % 8 == 0:
            fwd_image(p.w)
            kind = "conv_bf16"
        out.append((kind, p))
    return out


def bf16_backward(ops, precision, dgrad_image):
    """bf16-train: every ("dgrad", d) / ("wgrad", d) of a backward program whose reduction operand qualifies -> ("dgrad_bf16", d) /
    ("wgrad_bf16", d) (radnet_conv_dgrad_bf16_split / radnet_conv_wgrad_bf16 with the splits of radnet_*_bf16_pick_split).
    dgrad: stride 1, n and ld_dy multiples of 4; wgrad: c and n multiples of 8, ld_dy of 4.  dgrad_image(weight pointer) makes the
    layer's dgrad image if it does not exist yet.  Every other precision: `ops` unchanged."""
    if precision != "bf16-train":
        return ops
    out = []
    for kind, p in ops:
        if kind == "dgrad" and p.stride == 1 and p.n % 4 == 0 and p.ld_dy % 4 == 0 and p.ld_dy >= (p.n + 7) // 8 * 8:
            dgrad_image(p.w)
            kind = "dgrad_bf16"
        elif kind == "wgrad" and p.c % 8 == 0 and p.n % 8 == 0 and p.ld_dy % 4 == 0:
            kind = "wgrad_bf16"
        out.append((kind, p))
    return out


# The order of the passes matters and is kept HERE, not at the call sites: the fusing passes and the pairing of `compile` look for
# the fp32 kinds only.  Forward: the bottleneck fusion runs on fp32 "conv" ops, so it comes before the bf16 rewrite (engines whose
# precision is not fp32 do not ask for it).  Backward: the bf16 rewrite comes FIRST, so that a bf16 weight gradient keeps its
# bias-gradient column sum as the launch of its own behind it (exact fp32 sums of the unrounded dy) and is never folded into
# radnet_conv_bwd.
def forward_program(ops, precision, fwd_image, bottlenecks=False):
    """A forward launch list as it runs: stage-2 bottleneck fusion where the caller asks for it, then the bf16 rewrite."""
    if bottlenecks:
        ops = fuse_bottlenecks(ops)
    return bf16_forward(ops, precision, fwd_image)


def backward_program(ops, precision, dgrad_image):
    """A backward launch list as it runs: the bf16-train rewrite, then the bias gradients folded into their fp32 weight gradients."""
    return fuse_bias_grads(bf16_backward(ops, precision, dgrad_image))


def deferred_wgrad_form(ops):
    """The second form of a backward program whose ops are fp32 ("wgrad", d) / ("dgrad", d) only (bias gradients already folded into
    the weight gradients, fuse_bias_grads): (the data gradients as a program of their own, in their order; the weight-gradient
    descriptors in program order, for ONE radnet_conv_wgrad_multi call behind it), or None for a program with any other op -- a
    Winograd-domain weight gradient, a column sum left on its own, a bf16 kind.  Valid where every dy and every forward input of the
    program has its own buffer that nothing rewrites before the program ends: the weight gradients then read what they read in place.
    The descriptors are the program's own objects, so set_accumulate on `ops` reaches both forms."""
    if not ops or any(kind not in ("wgrad", "dgrad") for kind, _ in ops):
        return None
    wgrads = [p for kind, p in ops if kind == "wgrad"]
    if not wgrads:
        return None
    for k, (kind, p) in enumerate(ops):         # a data gradient behind a weight gradient must not write what that one reads
        if kind == "wgrad" and any(q.dx in (p.dy, p.x) for kq, q in ops[k + 1:] if kq == "dgrad" and q.dx):
            return None
    return [op for op in ops if op[0] == "dgrad"], wgrads


def desc_array(descs):
    """Copies of the descriptors as one radnet_conv_desc[] (radnet_conv_wgrad_multi)."""
    arr = (L.ConvDesc * len(descs))()
    for i, d in enumerate(descs):
        arr[i] = d
    return arr


# ---------------------------------------------------------------------------------------------- compile
def _ptr(v):
    return v.data_ptr() if hasattr(v, "data_ptr") else v


def _split64(o, v):
    o.i[0], o.i[1] = C.c_int32(v & 0xFFFFFFFF).value, int(v) >> 32


def compile(ops, cache, precision="fp32", fwd_image=None, dgrad_image=None):
    """The launch list as a radnet_op array.  Cached in `cache` per list and gradient write modes (the array holds copies of the
    descriptors); the entry holds `ops`, so the list's identity stays unique while it is cached.  fwd_image / dgrad_image(weight
    pointer): the record (wt, ldk, ...) / (wd, ldkd, ...) of a layer's bf16 image, for programs with bf16 kinds."""
    key = (id(ops), mode_key(ops))
    ent = cache.get(key)
    if ent is not None:
        return ent[0]
    arr = (L.Op * max(len(ops), 1))()
    paired = False
    for k, (kind, p) in enumerate(ops):
        o = arr[k]
        if paired:                              # the dgrad half of a pair: issued by the entry before (stays a no-op slot)
            paired = False
            o.kind = L.OP_NOP
            continue
        K = _kind_of(kind)
        o.kind = K.code
        if K.fields == DESC:
            o.conv = p
        elif K.fields == HANDLE:
            o.p[0] = p.value
        else:
            for j, f in enumerate(K.p):
                o.p[j] = _ptr(p[f])
            for j, f in enumerate(K.i):
                o.i[j] = p[f]
        if kind == "wgrad":                     # weight gradient and data gradient of one layer (same descriptor) -> one launch
            if k + 1 < len(ops) and ops[k + 1][0] == "dgrad" and ops[k + 1][1] is p:
                o.kind = L.OP_CONV_BWD
                paired = True
        elif kind == "bneck_first":
            o.i[0] = 1 if k + 2 < len(ops) and ops[k + 2][0] == "bneck_third" else 0
        elif kind in ("fill0", "relu_mask"):
            _split64(o, p[1] if kind == "fill0" else p[2])
        elif kind == "conv_bf16":               # one pass in bf16 inference engines, radnet_conv_bf16_pick_split in the trainable modes
            img = fwd_image(p.w)
            o.p[0], o.i[0] = _ptr(img.wt), img.ldk
            o.i[1] = int(L.load_library().radnet_conv_bf16_pick_split(p.nb * p.oh * p.ow, p.n, p.kh * p.kw * p.c)) if precision in MIXED_PRECISIONS else 0
        elif kind == "dgrad_bf16":
            img = dgrad_image(p.w)
            o.p[0], o.i[0] = _ptr(img.wd), img.ldkd
            o.i[1] = int(L.load_library().radnet_dgrad_bf16_pick_split(p.nb * p.h * p.w_, p.c, p.kh * p.kw * ((p.n + 7) // 8 * 8)))
        elif kind == "wgrad_bf16":
            o.i[1] = int(L.load_library().radnet_wgrad_bf16_pick_split(p.nb * p.oh * p.ow, p.n, p.kh * p.kw * p.c))
    cache[key] = (arr, ops)
    return arr


def evict(cache, list_ids):
    """Forget what `cache` (of compile, or an engine's hipGraphs: both keyed by a list's identity first) holds for the lists whose id()
    is in `list_ids` -- their plan is gone, and a new list may get the same identity."""
    for key in [k for k in cache if k[0] in list_ids]:
        del cache[key]
