"""radnet_hip.program.compile without a GPU: for every op kind, one op with stand-in pointers and distinct small integers in every
field, compiled, and every slot of the radnet_op compared with the layout include/radnet_hip.h and csrc/program.hip document --
written out here by hand, not computed by the code under test.  Then the wgrad + dgrad pairing, the cache key and the write modes.

Everything up to `# ---- new behaviour` ran unchanged against the engine-bound `_compile` this module replaced (only the three
adapters below differed): the translation did not move."""
import collections
import ctypes as C
import os

import pytest

from radnet_hip import lib as L
from radnet_hip import program as P

# ---- adapters: the only lines that name the code under test ---------------------------------------------------------------
Image = collections.namedtuple("Image", "wt ldk")
DgradImage = collections.namedtuple("DgradImage", "wd ldkd")


def _compiler(precision="fp32", fwd=None, dgrad=None):
    """compile(ops) on one cache.  fwd / dgrad: weight pointer -> bf16 image record."""
    cache = {}
    return lambda ops: P.compile(ops, cache, precision, (fwd or {}).__getitem__, (dgrad or {}).__getitem__)


set_accumulate = P.set_accumulate


# ---- stand-ins ---------------------------------------------------------------------------------------------------------------
class Ptr:
    """What the engine puts where a pointer goes: a tensor (anything with data_ptr)."""

    def __init__(self, v):
        self.v = v

    def data_ptr(self):
        return self.v


def _lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _desc(seed, **kw):
    """A descriptor with a distinct value in every field."""
    d = L.ConvDesc()
    for k, (name, _) in enumerate(L.ConvDesc._fields_):
        setattr(d, name, seed * 1000 + k + 1)
    for name, v in kw.items():
        setattr(d, name, v)
    return d


def _slots(o):
    return o.kind, list(o.i), list(o.p)


def _expect(kind, i=(), p=()):
    return kind, list(i) + [0] * (11 - len(i)), list(p) + [None] * (8 - len(p))


def _same_desc(o, d):
    return bytes(o.conv) == bytes(d)


ZERO_DESC = bytes(C.sizeof(L.ConvDesc))


# ---- the slot layout, kind by kind ----------------------------------------------------------------------------------------------
def test_descriptor_kinds():
    """CONV_FWD / CONV_DGRAD / CONV_WGRAD: the descriptor, nothing else.  CONV_FWD_PAIR: the second descriptor in the NOP slot behind."""
    ds = [_desc(s) for s in range(1, 6)]
    ops = [("conv", ds[0]), ("dgrad", ds[1]), ("wgrad", ds[2]), ("conv_pair_first", ds[3]), ("conv_pair_second", ds[4])]
    arr = _compiler()(ops)
    assert [_slots(arr[k]) for k in range(5)] == [_expect(1), _expect(2), _expect(3), _expect(15), _expect(0)]
    assert all(_same_desc(arr[k], ds[k]) for k in range(5))
    assert (L.OP_CONV_FWD, L.OP_CONV_DGRAD, L.OP_CONV_WGRAD, L.OP_CONV_FWD_PAIR, L.OP_NOP) == (1, 2, 3, 15, 0)
    ds[0].n = 77                                                          # the array holds copies
    assert arr[0].conv.n == 1018


def test_bottleneck_kinds():
    """CONV_BNECK: conv = the 3x3, i[0] = 1 when a third descriptor follows; the others ride in NOP slots."""
    ds = [_desc(s) for s in range(1, 6)]
    ops = [("bneck_first", ds[0]), ("bneck_second", ds[1]), ("bneck_third", ds[2]), ("bneck_first", ds[3]), ("bneck_second", ds[4])]
    arr = _compiler()(ops)
    assert [_slots(arr[k]) for k in range(5)] == [_expect(16, [1]), _expect(0), _expect(0), _expect(16, [0]), _expect(0)]
    assert all(_same_desc(arr[k], ds[k]) for k in range(5))


def test_maxpool():
    """MAXPOOL  p: x, y   i: nb, h, w, c, k, s"""
    arr = _compiler()([("maxpool", (Ptr(0x100), Ptr(0x200), 1, 2, 3, 4, 5, 6))])
    assert _slots(arr[0]) == _expect(4, [1, 2, 3, 4, 5, 6], [0x100, 0x200])
    assert bytes(arr[0].conv) == ZERO_DESC


def test_colsum():
    """COLSUM  p: g, gscale|0, out   i: m, n, ld, accumulate"""
    arr = _compiler()([("colsum", [0x100, 1, 2, 3, 0x200, 0x300, 1]), ("colsum", [0x400, 4, 5, 6, None, 0x500, 0])])
    assert _slots(arr[0]) == _expect(5, [1, 2, 3, 1], [0x100, 0x200, 0x300])
    assert _slots(arr[1]) == _expect(5, [4, 5, 6, 0], [0x400, None, 0x500])


def test_wino_and_wino_reuse():
    """WINO / WINO_REUSE  p: x, v, u, m, scale|0, shift|0, y   i: nb, h, w, c, n, tiles, act, ldy, form"""
    #          x      nb h  w  c  n  V      U      M      T  scale  shift  act y     ldy form
    payload = (0x100, 1, 2, 3, 4, 5, 0x200, 0x300, 0x400, 6, 0x500, 0x600, 7, 0x700, 8, 9)
    arr = _compiler()([("wino", payload), ("wino_reuse", payload), ("wino", payload[:10] + (None, None) + payload[12:])])
    want_i, want_p = [1, 2, 3, 4, 5, 6, 7, 8, 9], [0x100, 0x200, 0x300, 0x400, 0x500, 0x600, 0x700]
    assert _slots(arr[0]) == _expect(6, want_i, want_p)
    assert _slots(arr[1]) == _expect(7, want_i, want_p)
    assert _slots(arr[2]) == _expect(6, want_i, [0x100, 0x200, 0x300, 0x400, None, None, 0x700])


def test_wino_wgrad():
    """WINO_WGRAD  p: dy, v, dz, du, dw, gscale|0   i: nb, h, w, c, n, ld_dy, tiles, ldw, accumulate mode, form"""
    #          dy     nb h  w  c  n  ld_dy V      dZ     dU     T  dw     ldw form gscale mode
    payload = [0x100, 1, 2, 3, 4, 5, 6,    0x200, 0x300, 0x400, 7, 0x500, 8,  9,   0x600, 2]
    arr = _compiler()([("wino_wgrad", payload)])
    assert _slots(arr[0]) == _expect(8, [1, 2, 3, 4, 5, 6, 7, 8, 2, 9], [0x100, 0x200, 0x300, 0x400, 0x500, 0x600])


def test_scatter_and_roi_bwd():
    """SCATTER  p: src, mask|0, dst   i: nb, oh, ow, c, stride, h, w.     ROI_BWD  p: dy, rois, dfmap   i: h, w, c, r, ps"""
    #                      src    nb oh ow c  st h  w  mask   dst
    ops = [("scatter", (0x100, 1, 2, 3, 4, 5, 6, 7, 0x200, 0x300)), ("scatter", (0x100, 1, 2, 3, 4, 5, 6, 7, None, 0x300)),
           #               dy     h  w  c  rois   r  ps dF
           ("roi_bwd", (0x400, 1, 2, 3, 0x500, 4, 5, 0x600))]
    arr = _compiler()(ops)
    assert _slots(arr[0]) == _expect(9, [1, 2, 3, 4, 5, 6, 7], [0x100, 0x200, 0x300])
    assert _slots(arr[1]) == _expect(9, [1, 2, 3, 4, 5, 6, 7], [0x100, None, 0x300])
    assert _slots(arr[2]) == _expect(12, [1, 2, 3, 4, 5], [0x400, 0x500, 0x600])


def test_fill0_and_relu_mask_split_their_64_bit_count():
    """FILL0  p: dst   i: bytes (low 32 bits), bytes (high).     RELU_MASK  p: g, act   i: n (low), n (high).  The low word travels as
    the int32 with the same bits (program.hip reads it back through uint32_t)."""
    big = (5 << 32) | 0x80000007                                          # low word has its top bit set: -2147483641 as int32
    ops = [("fill0", (0x100, 1234)), ("fill0", (0x100, big)), ("relu_mask", (0x200, 0x300, 4321)), ("relu_mask", (0x200, 0x300, big))]
    arr = _compiler()(ops)
    assert _slots(arr[0]) == _expect(10, [1234, 0], [0x100])
    assert _slots(arr[1]) == _expect(10, [-2147483641, 5], [0x100])
    assert _slots(arr[2]) == _expect(11, [4321, 0], [0x200, 0x300])
    assert _slots(arr[3]) == _expect(11, [-2147483641, 5], [0x200, 0x300])


def test_chain():
    """CHAIN  p: radnet_chain*"""
    arr = _compiler()([("chain", C.c_void_p(0xABC0))])
    assert _slots(arr[0]) == _expect(14, [], [0xABC0])


def test_bf16_kinds():
    """CONV_FWD_BF16  conv, p[0] = wt, i[0] = ldk, i[1] = ksplit (0 in bf16 inference engines, radnet_conv_bf16_pick_split in the
    trainable modes).  CONV_DGRAD_BF16  conv, p[0] = wd, i[0] = ldkd, i[1] = ksplit.  CONV_WGRAD_BF16  conv, i[1] = msplit.
    The shapes and their splits are rows of the tables in tests/test_bf16_train_abi.py (the forward rule is the weight gradient's on
    (rows = K, cols = N, reduction = M))."""
    _lib()
    fwd = _desc(1, w=0x1000, nb=1, oh=16, ow=32, n=64, kh=1, kw=1, c=2394)               # M 512, N 64, K 2394: split 8
    dg = _desc(2, w=0x2000, nb=20, h=7, w_=7, c=512, kh=1, kw=1, n=2048)                 # P 980, C 512, kd 2048: split 2
    wg = _desc(3, w=0x3000, nb=1, oh=38, ow=63, n=64, kh=1, kw=1, c=512)                 # M 2394, N 64, K 512: split 8
    images = {0x1000: Image(Ptr(0xAAA0), 2400)}
    dimages = {0x2000: DgradImage(Ptr(0xBBB0), 2048)}
    ops = [("conv_bf16", fwd), ("dgrad_bf16", dg), ("wgrad_bf16", wg)]
    for precision, fwd_split in (("bf16", 0), ("bf16-mixed", 8), ("bf16-train", 8)):
        arr = _compiler(precision, images, dimages)(ops)
        assert _slots(arr[0]) == _expect(17, [2400, fwd_split], [0xAAA0]), precision
        assert _slots(arr[1]) == _expect(18, [2048, 2], [0xBBB0])
        assert _slots(arr[2]) == _expect(19, [0, 8])
        assert _same_desc(arr[0], fwd) and _same_desc(arr[1], dg) and _same_desc(arr[2], wg)


def test_unknown_kind_raises():
    with pytest.raises(L.RadnetError):
        _compiler()([("conv", _desc(1)), ("convolve", _desc(2))])


# ---- pairing ---------------------------------------------------------------------------------------------------------------
def test_wgrad_and_dgrad_of_one_descriptor_become_one_launch():
    d1, d2, d3 = _desc(1), _desc(2), _desc(3)
    ops = [("wgrad", d1), ("dgrad", d1), ("wgrad", d2), ("dgrad", d3), ("wgrad", d3), ("colsum", [1, 2, 3, 4, None, 5, 1]), ("dgrad", d3), ("wgrad", d2)]
    arr = _compiler()(ops)
    # CONV_BWD + NOP (the NOP slot carries nothing); another descriptor's dgrad, or a dgrad not right behind, stays a launch of its own
    assert [arr[k].kind for k in range(8)] == [13, 0, 3, 2, 3, 5, 2, 3]
    assert _same_desc(arr[0], d1) and bytes(arr[1].conv) == ZERO_DESC
    assert _same_desc(arr[2], d2) and _same_desc(arr[3], d3) and _same_desc(arr[6], d3)
    same_values = L.ConvDesc.from_buffer_copy(d1)                         # equal fields, another object: not "the same descriptor"
    assert [o.kind for o in _compiler()([("wgrad", d1), ("dgrad", same_values)])[0:2]] == [3, 2]


def test_a_bf16_weight_gradient_is_never_paired():
    _lib()
    d = _desc(1, w=0x2000, nb=20, h=7, w_=7, oh=7, ow=7, c=512, kh=1, kw=1, n=2048)
    dimages = {0x2000: DgradImage(Ptr(0xBBB0), 2048)}
    for ops in ([("wgrad_bf16", d), ("dgrad", d)], [("wgrad_bf16", d), ("dgrad_bf16", d)]):
        arr = _compiler("bf16-train", None, dimages)(ops)
        assert [arr[0].kind, arr[1].kind] == [19, 2 if ops[1][0] == "dgrad" else 18]
    arr = _compiler("bf16-train", None, dimages)([("wgrad", d), ("dgrad_bf16", d)])     # nor an fp32 one with a bf16 data gradient
    assert [arr[0].kind, arr[1].kind] == [3, 18]


# ---- the cache key ------------------------------------------------------------------------------------------------------------
def test_key_changes_when_and_only_when_set_accumulate_changes_a_mode():
    """One compiled array per (list, write modes): the same array comes back while the modes stand, another one when set_accumulate
    changed one, the first again when it is changed back; each holds the modes it was compiled with."""
    _lib()
    d1, d2 = _desc(1, dw_accumulate=1), _desc(2, dw_accumulate=1, nb=1, oh=38, ow=63, n=64, kh=1, kw=1, c=512)
    wino_wg = [0x100, 1, 2, 3, 4, 5, 6, 0x200, 0x300, 0x400, 7, 0x500, 8, 9, None, 1]
    col = [0x100, 1, 2, 3, None, 0x300, 1]
    ops = [("wgrad", d1), ("colsum", col), ("dgrad", d1), ("wgrad_bf16", d2), ("wino_wgrad", wino_wg), ("conv", _desc(3))]
    compile_ = _compiler("bf16-train")

    def modes(arr):
        return arr[0].conv.dw_accumulate, arr[1].i[3], arr[3].conv.dw_accumulate, arr[4].i[8]

    a_add = compile_(ops)
    assert compile_(ops) is a_add and modes(a_add) == (1, 1, 1, 1)
    set_accumulate(ops, True)                                             # already adding: nothing changes
    assert compile_(ops) is a_add
    set_accumulate(ops, False, prezeroed=True)
    assert (d1.dw_accumulate, col[6], d2.dw_accumulate, wino_wg[15]) == (2, 1, 2, 2)
    a_pre = compile_(ops)
    assert a_pre is not a_add and modes(a_pre) == (2, 1, 2, 2) and modes(a_add) == (1, 1, 1, 1)
    set_accumulate(ops, False)
    assert (d1.dw_accumulate, col[6], d2.dw_accumulate, wino_wg[15]) == (0, 0, 0, 0)
    a_over = compile_(ops)
    assert a_over is not a_add and a_over is not a_pre and modes(a_over) == (0, 0, 0, 0)
    set_accumulate(ops, False)
    assert compile_(ops) is a_over
    set_accumulate(ops, True)
    assert compile_(ops) is a_add
    other = list(ops)                                                     # an equal list is another program
    assert compile_(other) is not a_add
    for one in (("wgrad", d1), ("wgrad_bf16", d2), ("wino_wgrad", wino_wg), ("colsum", col)):     # each kind alone moves the key
        prog = [one]
        set_accumulate(prog, True)
        first = compile_(prog)
        set_accumulate(prog, False)
        assert compile_(prog) is not first, one[0]


# ---- new behaviour ------------------------------------------------------------------------------------------------------------
def test_every_kind_states_its_write_mode_and_unknown_kinds_raise():
    """The write mode is a column of the one table: a kind cannot be added without saying where it keeps it (or None: it writes no
    parameter gradient), and set_accumulate / write_mode / the key refuse a kind the table does not hold instead of skipping it."""
    assert {k for k, row in P.KINDS.items() if row.mode is not None} == {"wgrad", "wgrad_bf16", "wino_wgrad", "colsum"}
    with pytest.raises(TypeError):
        P.Kind(L.OP_CONV_WGRAD, P.DESC, (), ())                           # a row without the mode column
    d = _desc(1, dw_accumulate=1)
    for call in (lambda: P.set_accumulate([("wgrad", d), ("wgrad_fused", d)], False), lambda: P.write_mode("wgrad_fused", d),
                 lambda: P.set_write_mode("wgrad_fused", d, 0), lambda: P.mode_key([("wgrad_fused", d)])):
        with pytest.raises(L.RadnetError):
            call()
    assert P.write_mode("dgrad", d) is None and P.write_mode("wgrad", d) == 0          # (the first call above reached the known op)
    assert P.mode_key([("wgrad", d), ("dgrad", d), ("colsum", [0, 0, 0, 0, None, 0, 1]), ("conv", d)]) == (0, 1)


def test_this_file_covers_every_kind():
    import re
    with open(__file__) as f:
        used = set(re.findall(r'\("([a-z0-9_]+)", ', f.read()))
    assert set(P.KINDS) <= used, sorted(set(P.KINDS) - used)


def test_constructors_state_the_field_order_once():
    """The keyword constructors build today's payloads: same positions, a list where set_accumulate edits the mode in place."""
    kind, p = P.wino(x=0x100, nb=1, h=2, w=3, c=4, n=5, V=0x200, U=0x300, M=0x400, T=6, scale=0x500, shift=0x600, act=7, y=0x700, ldy=8, form=9)
    assert kind == "wino" and tuple(p) == (0x100, 1, 2, 3, 4, 5, 0x200, 0x300, 0x400, 6, 0x500, 0x600, 7, 0x700, 8, 9) and p[7] == p.U == 0x300
    x, nb, hh, ww, c, n, V, U, M, T, scale, shift, act, y, ldy, form = p                  # unpacks as the plain tuple did
    assert P.wino_reuse((kind, p)) == ("wino_reuse", p)
    kind, p = P.wino_wgrad(dy=0x100, nb=1, h=2, w=3, c=4, n=5, ld_dy=6, V=0x200, dZ=0x300, dU=0x400, T=7, dw=0x500, ldw=8, form=9, gscale=None, mode=1)
    assert kind == "wino_wgrad" and p == [0x100, 1, 2, 3, 4, 5, 6, 0x200, 0x300, 0x400, 7, 0x500, 8, 9, None, 1] and type(p) is list
    kind, p = P.colsum(g=0x100, m=1, n=2, ld=3, gscale=None, out=0x200, accumulate=1)
    assert kind == "colsum" and p == [0x100, 1, 2, 3, None, 0x200, 1] and type(p) is list
    assert P.maxpool(x=1, y=2, nb=3, h=4, w=5, c=6, k=7, stride=8) == ("maxpool", (1, 2, 3, 4, 5, 6, 7, 8))
    assert P.scatter(src=1, nb=2, oh=3, ow=4, c=5, stride=6, h=7, w=8, mask=None, dst=9) == ("scatter", (1, 2, 3, 4, 5, 6, 7, 8, None, 9))
    assert P.roi_bwd(dy=1, h=2, w=3, c=4, rois=5, r=6, ps=7, dF=8) == ("roi_bwd", (1, 2, 3, 4, 5, 6, 7, 8))
    assert P.fill0(dst=1, nbytes=2) == ("fill0", (1, 2)) and P.relu_mask(g=1, act=2, n=3) == ("relu_mask", (1, 2, 3))
    with pytest.raises(TypeError):
        P.colsum(g=1, m=2, n=3, ld=4, gscale=None, out=5)                                 # a field left out


def test_module_loads_without_torch():
    import subprocess
    import sys
    code = "import sys; import radnet_hip.program; assert 'torch' not in sys.modules"
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(P.__file__))))
    subprocess.check_call([sys.executable, "-c", code], env=env)
