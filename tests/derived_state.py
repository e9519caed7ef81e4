"""One auditor for every device buffer an engine DERIVES from its trainable fp32 weights ('Derived copies of the trainable
weights', says who rewrites which and when):

  shift       the folded epilogue shift of a trainable conv, scale * bias + t0 (head_shift, ContEngine's s34_shift), or the bias itself
              where nothing is folded (the RPN convs, the VGG16 engine's fc layers: shift IS the bias, one storage)
  wino_u      the Winograd-transformed filter U = G g G^T of a layer that holds one, F(2x2,3x3) or F(4x4,3x3)
  bf16_fwd    the bf16 forward image [n][ldk] of a layer (Bf16Images.fwd)
  bf16_dgrad  the bf16 data-gradient image [cin][ldkd] of a layer (Bf16Images.dgrad)

audit(engine) discovers them from the engine -- every conv of engine.convs that holds a bias and a shift, every conv.wino_u that is not
None, every entry of engine.bf16.fwd / .dgrad -- never from a list of names, reads the master parameters through the convs' own views and
returns one Record per buffer.  The expected values import nothing of the product:

  shift       float64 scale * bias + t0 of the fp32 inputs, |got - ref| <= 2 * 2^-24 * (|scale * bias| + |t0|): one fp32 multiply and one
              add, contracted into an fma or not.  Without a fold (t0 is None) the bound is zero.  One Adam step moves a bias by about
              lr = 2e-5, orders of magnitude above the bound of a value of order one: a shift that lags by one step is seen.
  wino_u      winograd_edge_cases.stage_filter(arith="f64") with the form from conv.wino_m and the pitch from conv.ldw, under that
              module's bound for the filter stage (counted rounding steps * 2^-24 * |G| |g| |G|^T, as test_gpu_winograd_edges.py)
  bf16_*      bit for bit: round to nearest even, the layout statements below (the ones test_gpu_bf16_predict.py and
              test_gpu_bf16_train.py hold the cast kernels to), every padding element zero

A buffer of the wrong SIZE (a U in the other form, an image with another pitch) is wrong in every element.  Buffers that a set
engine._inference_filters_stale excuses -- what sync_inference_filters() would rewrite: the U of INFERENCE_WINOGRAD_LAYERS, the bf16
images -- keep their figures and are reported with excused=True; audit(engine, inference=True) calls sync_inference_filters() first,
the contract of every inference entry point, and then excuses nothing.

assert_same_as_fresh(engine, fresh) compares the same buffers bit for bit with those of an engine built anew and given the same weights
(both sets came out of the same kernels); a buffer the fresh engine has not made yet is made there first, through the engine's own
lazy path.  tests/test_derived_state_reference.py shows on a stand-in of CPU tensors that the auditor flags seven kinds of stale or
misplaced copy, each on its own record only."""
import collections

import numpy as np
import torch

import winograd_edge_cases as W

U = 2.0 ** -24
Record = collections.namedtuple("Record", "layer kind worst n_wrong excused")       # worst: max err / bound (inf: a wrong bit, a wrong size)
Buffer = collections.namedtuple("Buffer", "layer kind tensor conv meta")
KINDS = ("shift", "wino_u", "bf16_fwd", "bf16_dgrad")


# ---------------------------------------------------------------------------------------------------------------- bf16 statements
def bf16_bits(a):
    """NumPy round to nearest, ties to even, fp32 -> bf16 bit patterns (uint16); finite inputs."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def fwd_image_bits(w, n):
    """The [n][K] bf16 bit patterns of the forward image of w [K][ldw]: torch's CPU cast (round to nearest even) of the first n columns,
    transposed.  The image [n][ldk] holds them in its first K columns and zero behind."""
    return torch.from_numpy(np.ascontiguousarray(w[:, :n].T)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def fwd_image_ref(w, k, n, ldk):
    ref = np.zeros((n, ldk), np.uint16)
    ref[:, :k] = fwd_image_bits(w[:k], n)
    return ref


def dgrad_image_ref(w, taps, c, n, ldkd):
    """wd[i][t*n8 + j] = bf16(w[t*c + i][j]); zero elsewhere."""
    n8 = (n + 7) // 8 * 8
    ref = np.zeros((c, ldkd), np.uint16)
    b = bf16_bits(w[:, :n]).reshape(taps, c, n)
    for t in range(taps):
        ref[:, t * n8:t * n8 + n] = b[t]
    return ref


# ---------------------------------------------------------------------------------------------------------------- discovery
def _np(t):
    return t.detach().cpu().numpy()


def derived_buffers(eng):
    """Every derived buffer the engine holds NOW, in a fixed order: [Buffer(layer, kind, tensor, conv, meta)]."""
    out = []
    for name, c in eng.convs.items():
        if getattr(c, "bias", None) is not None and getattr(c, "shift", None) is not None:
            out.append(Buffer(name, "shift", c.shift, c, None))
    for name, c in eng.convs.items():
        if getattr(c, "wino_u", None) is not None:
            out.append(Buffer(name, "wino_u", c.wino_u, c, c.wino_m))
    bf = getattr(eng, "bf16", None)
    for kind, table in (("bf16_fwd", getattr(bf, "fwd", {})), ("bf16_dgrad", getattr(bf, "dgrad", {}))):
        for im in table.values():
            out.append(Buffer(im.conv.name, kind, im[0], im.conv, im))
    return out


def _excusable(eng, b):
    """What sync_inference_filters() rewrites when _inference_filters_stale is set."""
    if not getattr(eng, "_inference_filters_stale", False):
        return False
    return b.kind in ("bf16_fwd", "bf16_dgrad") or (b.kind == "wino_u" and b.layer in getattr(eng, "INFERENCE_WINOGRAD_LAYERS", ()))


# ---------------------------------------------------------------------------------------------------------------- references
_WINO_CACHE = {}      # (layer, form, cin, cout, ldw) -> (weights, ref, tol): a frozen layer's reference is computed once per weight load


def _wino_reference(c, w):
    key = (c.name, c.wino_m, c.cin, c.cout, c.ldw)
    ent = _WINO_CACHE.get(key)
    if ent is None or not np.array_equal(ent[0], w):
        res = W.stage_filter(w, c.cin, c.cout, c.ldw, c.wino_m, arith="f64")
        n = (c.wino_m + 2) ** 2 * c.cin * c.cout
        assert res["inside"][:n].all() and not res["inside"][n:].any()
        ent = _WINO_CACHE[key] = (w.copy(), res["buf"][:n], res["tol"][:n])
    return ent[1], ent[2]


def _judge(got, ref, tol):
    """(worst err / tol, number of elements outside tol); a zero bound asks for equality."""
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= tol)                                  # NaN counts as wrong
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / tol, 0.0)
    ratio = np.nan_to_num(ratio, nan=np.inf, posinf=np.inf)
    return (float(ratio.max()) if ratio.size else 0.0), int(bad.sum())


def _bits(got, ref):
    if got.shape != ref.shape:
        return float("inf"), int(max(got.size, ref.size))
    n = int((got != ref).sum())
    return (float("inf") if n else 0.0), n


def audit_buffer(b):
    """(worst, n_wrong) of one Buffer against its reference."""
    c = b.conv
    if b.kind == "shift":
        got, bias = _np(b.tensor).reshape(-1), _np(c.bias).reshape(-1).astype(np.float64)
        if got.size != bias.size:
            return float("inf"), int(max(got.size, bias.size))
        if getattr(c, "t0", None) is None:
            return _judge(got, bias, np.zeros_like(bias))
        scale, t0 = _np(c.scale).reshape(-1).astype(np.float64), _np(c.t0).reshape(-1).astype(np.float64)
        return _judge(got, scale * bias + t0, 2 * U * (np.abs(scale * bias) + np.abs(t0)))
    w = _np(c.weight).reshape(c.kh * c.kh * c.cin, c.ldw)
    if b.kind == "wino_u":
        got = _np(b.tensor).reshape(-1)
        ref, tol = _wino_reference(c, w)
        if got.size != ref.size:
            return float("inf"), int(max(got.size, ref.size))
        return _judge(got, ref, tol)
    im = b.meta
    got = _np(b.tensor).view(np.uint16)
    if b.kind == "bf16_fwd":
        return _bits(got, fwd_image_ref(w, c.kh * c.kh * c.cin, im.n, im.ldk))
    return _bits(got, dgrad_image_ref(w, c.kh * c.kh, c.cin, im.n, im.ldkd))


def audit(eng, inference=False, kinds=KINDS, layers=None):
    """One Record(layer, kind, worst err / bound, elements wrong, excused) per derived buffer the engine holds (of `kinds`, of `layers`)."""
    if inference:
        eng.sync_inference_filters()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    out = []
    for b in derived_buffers(eng):
        if b.kind not in kinds or (layers is not None and b.layer not in layers):
            continue
        worst, n_wrong = audit_buffer(b)
        out.append(Record(b.layer, b.kind, worst, n_wrong, bool(n_wrong) and _excusable(eng, b)))
    return out


def wrong(records):
    """The records that are over their bound or hold a wrong bit and have no excuse."""
    return [r for r in records if (r.n_wrong or r.worst > 1.0) and not r.excused]


def assert_clean(records, what=""):
    bad = wrong(records)
    assert not bad, "%s: %d of %d derived buffers are stale or misplaced: %s" % (what, len(bad), len(records), bad[:6])
    return records


# ---------------------------------------------------------------------------------------------------------------- against a fresh engine
def _materialize(fresh, b):
    """Make buffer `b` of another engine in `fresh`, through the engine's own lazy path."""
    c = fresh.convs[b.layer]
    if b.kind == "wino_u" and c.wino_u is None:
        fresh._refresh_winograd([b.layer])
    elif b.kind == "bf16_fwd":
        fresh.bf16.weights(c)
    elif b.kind == "bf16_dgrad":
        fresh.bf16.dgrad_weights(c)


def assert_same_as_fresh(eng, fresh):
    """Every derived buffer of `eng` equals, bit for bit, the one of `fresh` (built anew, same weights, same kernels)."""
    mine = derived_buffers(eng)
    for b in mine:
        _materialize(fresh, b)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    theirs = {(b.layer, b.kind): b for b in derived_buffers(fresh)}
    bad = []
    for b in mine:
        o = theirs.get((b.layer, b.kind))
        if o is None or o.tensor.shape != b.tensor.shape:
            bad.append((b.layer, b.kind, "missing or another size"))
        elif not torch.equal(b.tensor.view(torch.int16 if b.tensor.dtype == torch.int16 else torch.int32).cpu(),
                             o.tensor.view(torch.int16 if o.tensor.dtype == torch.int16 else torch.int32).cpu()):
            bad.append((b.layer, b.kind, int((b.tensor.cpu() != o.tensor.cpu()).sum())))
    assert not bad, "%d of %d derived buffers differ from a freshly loaded engine's: %s" % (len(bad), len(mine), bad[:6])
    return len(mine)
