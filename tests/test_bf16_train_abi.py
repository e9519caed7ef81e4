"""bf16-train mode, host side (no GPU needed): the backward entry points and the dgrad-image registry struct are declared, exported
and bound with the header's layout, the program ops are 18 / 19 and documented, the split rules are the documented fixed functions,
and precision="bf16-train" passes the argument checks of FasterRCNNEngine / build_models before any device is touched -- while
VGG16, the cont_train.py mode and NativeTrainStep refuse it.  The op passes (radnet_hip.program) need no device and no engine."""
import ctypes as C
import os
import re
import types

import pytest

from radnet_hip import lib as L

NEW = ("radnet_weights_to_bf16_dgrad", "radnet_weights_to_bf16_dgrad_arena", "radnet_conv_dgrad_bf16", "radnet_conv_dgrad_bf16_split",
       "radnet_conv_wgrad_bf16", "radnet_dgrad_bf16_pick_split", "radnet_wgrad_bf16_pick_split")


def _lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _header():
    with open(L.HEADER_PATH) as f:
        return f.read()


def test_header_declares_and_library_exports_bf16_train_entry_points():
    names = L.declared_symbols()
    lib = _lib()
    for n in NEW:
        assert n in names, "include/radnet_hip.h does not declare %s" % n
        assert hasattr(lib, n), "libradnet_hip.so does not export %s" % n
        assert getattr(lib, n).argtypes is not None, "%s has no ctypes binding" % n
    assert lib.radnet_weights_to_bf16_dgrad_arena.argtypes[-2] == C.POINTER(L.Bf16DgradImage)
    assert len(lib.radnet_conv_dgrad_bf16.argtypes) == 4 and len(lib.radnet_conv_wgrad_bf16.argtypes) == 3


def test_dgrad_image_struct_matches_header():
    m = re.search(r"typedef struct radnet_bf16_dgrad_image \{(.*?)\} radnet_bf16_dgrad_image;", _header(), re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r"(int64_t|int32_t|uint16_t\s*\*)\s*(.*)", decl).groups()
        for nm in names.split(","):
            fields.append((nm.strip(), ctype.replace(" ", "")))
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint16_t*": C.c_void_p}
    assert [(f[0], kinds[f[1]]) for f in fields] == list(L.Bf16DgradImage._fields_)
    # natural C alignment: off 0, taps 8, c 12, n 16, ldw 20, wd 24, ldkd 32, size 40
    assert [getattr(L.Bf16DgradImage, n).offset for n in ("off", "taps", "c", "n", "ldw", "wd", "ldkd")] == [0, 8, 12, 16, 20, 24, 32]
    assert C.sizeof(L.Bf16DgradImage) == 40


def test_op_numbers_and_documentation():
    text = _header()
    assert L.OP_CONV_FWD_BF16 == 17 and L.OP_CONV_DGRAD_BF16 == 18 and L.OP_CONV_WGRAD_BF16 == 19
    assert re.search(r"RADNET_OP_CONV_FWD_BF16 = 17, RADNET_OP_CONV_DGRAD_BF16 = 18, RADNET_OP_CONV_WGRAD_BF16 = 19", text)
    assert re.search(r"CONV_DGRAD_BF16 conv, p\[0\] = wd .*i\[0\] = ldkd, i\[1\] = ksplit", text)
    assert re.search(r"CONV_WGRAD_BF16 conv, i\[1\] = msplit", text)


# (M = output pixels, N, K = kh*kw*c) of the weight gradients of the 600x1000 training plans (38 x 63 feature map, 20 RoIs of 14x14 ->
# 7x7 per image), per-GPU batch 1 and 2, and the split radnet_wgrad_bf16_pick_split gives them
WGRAD_600x1000 = {
    # batch 1
    (2394, 64, 512): 8,         # rpn_heads: 8 output tiles of 64x64; 75 pixel tiles: 16 slices would keep fewer than 8 each
    (2394, 512, 9216): 1,       # rpn_conv1: 288 tiles of 128x128 already
    (980, 512, 1024): 2,        # res5a_branch2a: 128 tiles
    (980, 2048, 1024): 1,       # res5a_branch1: 256 tiles of 128x64
    (980, 512, 4608): 1,        # res5[abc]_branch2b: 288 tiles of 128x64
    (980, 2048, 512): 1,        # res5[abc]_branch2c: 256 tiles
    (980, 512, 2048): 1,        # res5[bc]_branch2a: 256 tiles
    # batch 2
    (4788, 64, 512): 16,
    (4788, 512, 9216): 1,
    (1960, 512, 1024): 2,
    (1960, 2048, 1024): 1,
    (1960, 512, 4608): 1,
    (1960, 2048, 512): 1,
    (1960, 512, 2048): 1,
}
# (P = input pixels, C, kd = kh*kw*n8) of the data gradients
DGRAD_600x1000 = {
    (2394, 512, 64): 1,         # rpn_heads: two reduction tiles only
    (980, 512, 2048): 2,        # res5[abc]_branch2c
    (980, 512, 4608): 2,        # res5[abc]_branch2b
    (980, 2048, 512): 1,        # res5[bc]_branch2a: 512 tiles
    (4788, 512, 64): 1,
    (1960, 512, 2048): 2,       # 248 tiles of 64x64
    (1960, 512, 4608): 2,
    (1960, 2048, 512): 1,
}


def _tiles(rows, cols):
    cd = lambda a, b: (a + b - 1) // b
    if cols > 64 and cd(rows, 128) * cd(cols, 128) >= 256:
        return cd(rows, 128) * cd(cols, 128), 128 * 128
    if cd(rows, 128) * cd(cols, 64) >= 256:
        return cd(rows, 128) * cd(cols, 64), 128 * 64
    return cd(rows, 64) * cd(cols, 64), 64 * 64


def test_split_rules():
    lib = _lib()
    wg, dg, fwd = lib.radnet_wgrad_bf16_pick_split, lib.radnet_dgrad_bf16_pick_split, lib.radnet_conv_bf16_pick_split
    for (M, N, K), s in WGRAD_600x1000.items():
        assert wg(M, N, K) == s, (M, N, K, wg(M, N, K))
    for (P, Cc, kd), s in DGRAD_600x1000.items():
        assert dg(P, Cc, kd) == s, (P, Cc, kd, dg(P, Cc, kd))
    for M, N, K in list(WGRAD_600x1000) + [(1, 8, 8), (49, 64, 64), (200000, 8, 8), (70, 2048, 18432), (0, 5, 5), (1 << 40, 64, 64)]:
        s = wg(M, N, K)
        assert 1 <= s <= 16 and s & (s - 1) == 0                         # a power of two, capped
        assert s == 1 or (M + 31) // 32 >= 8 * s                         # every slice keeps >= 8 pixel tiles
        assert s == fwd(K, N, min(M, 1 << 30))                           # the forward's rule on (rows = K, cols = N, reduction = M)
        tiles, elems = _tiles(K, N)
        bm, bn = C.c_int32(), C.c_int32()
        if M > 0:                                                        # the exported rule is the one the launchers use
            assert lib.radnet_conv_bf16_tile_shape(K, N, C.byref(bm), C.byref(bn)) == tiles and bm.value * bn.value == elems
        assert s == 1 or tiles * (s // 2) < 256                          # the smallest that reaches 256 workgroups
        # the slabs of every training shape fit the 256 MB workspace of a lane (rpn_conv1's 18.9 MB gradient is not split at all)
        if (M, N, K) in WGRAD_600x1000:
            assert s == 1 or tiles * s * elems * 4 <= 256 << 20
    for P, Cc, kd in list(DGRAD_600x1000) + [(5, 8, 32), (100000, 64, 64)]:
        assert dg(P, Cc, kd) == fwd(P, Cc, kd)
    assert wg(100000, 64, 64) == 16                                      # the cap


class _Stop(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to select a device ends the constructor: what ran before it are the argument checks."""
    import torch

    def stop(*a, **k):
        raise _Stop()
    monkeypatch.setattr(torch.cuda, "set_device", stop)


def test_bf16_train_passes_argument_checks_before_device(no_device):
    from faster_rcnn import models as M
    from faster_rcnn.config import Config
    from radnet_hip import engine as E
    assert E.PRECISIONS == ("fp32", "bf16", "bf16-mixed", "bf16-train")
    with pytest.raises(_Stop):
        E.FasterRCNNEngine(Config(), precision="bf16-train")
    with pytest.raises(_Stop):
        M.build_models(Config(), precision="bf16-train")
    for bad in ("bf16_train", "train", "fp16-train"):
        with pytest.raises(ValueError):
            E.FasterRCNNEngine(Config(), precision=bad)
        with pytest.raises(ValueError):
            M.build_models(Config(), precision=bad)


def test_bf16_train_refused_for_vgg16_cont_and_native(no_device):
    from faster_rcnn import models as M
    from faster_rcnn.config import Config
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.engine_cont import ContEngine
    from radnet_hip.engine_vgg import VGG16Engine
    from radnet_hip.native import NativeTrainStep
    Cv = Config()
    Cv.network = "vgg16"
    with pytest.raises(NotImplementedError):
        M.build_models(Cv, precision="bf16-train")
    with pytest.raises(NotImplementedError):
        VGG16Engine(Cv, precision="bf16-train")
    with pytest.raises(NotImplementedError):
        ContEngine(Config(), precision="bf16-train")
    with pytest.raises(NotImplementedError):
        FasterRCNNEngine(Config(), workload="cont", precision="bf16-train")
    with pytest.raises(NotImplementedError):
        M.build_models(Config(), workload="cont", precision="bf16-train")
    with pytest.raises(NotImplementedError):
        NativeTrainStep(types.SimpleNamespace(precision="bf16-train"))


def _desc(**kw):
    d = L.ConvDesc()
    for k, v in dict(dict(nb=1, h=7, w_=7, c=512, oh=7, ow=7, kh=1, kw=1, stride=1, n=2048, ld_dy=2048, w=0x1000), **kw).items():
        setattr(d, k, v)
    return d


def test_bwd_op_pass_bias_fusion_pairing_and_accumulate_keys():
    """program.bf16_backward: which ops become bf16, that fuse_bias_grads leaves their column sums alone, that set_accumulate
    reaches them, and that every other precision keeps its list."""
    from radnet_hip import program as E
    made = []                                             # the weight pointers a dgrad image was asked for
    d1, d2, d3 = _desc(), _desc(stride=2, h=14, w_=14), _desc(c=4, n=64, ld_dy=64)
    ops = [("wgrad", d1), ("colsum", [1, 49, 2048, 2048, None, 2, 1]), ("dgrad", d1), ("wgrad", d2), ("dgrad", d2), ("wgrad", d3), ("dgrad", d3),
           ("colsum", [1, 49, 64, 64, None, 3, 1])]
    for precision in ("fp32", "bf16", "bf16-mixed"):
        assert E.bf16_backward(ops, precision, made.append) is ops
    out = E.bf16_backward(ops, "bf16-train", made.append)
    assert [k for k, _ in out] == ["wgrad_bf16", "colsum", "dgrad_bf16", "wgrad_bf16", "dgrad", "wgrad", "dgrad_bf16", "colsum"]
    assert made == [0x1000, 0x1000]                       # a dgrad image per bf16 data gradient; the stride-2 dgrad and the 4-channel wgrad stay fp32
    fused = E.fuse_bias_grads(out)
    assert [k for k, _ in fused] == [k for k, _ in out] and not d1.db, "a bf16 weight gradient keeps its exact fp32 column sum launch"
    E.set_accumulate(out, False, prezeroed=True)
    assert d1.dw_accumulate == 2 and d2.dw_accumulate == 2 and d3.dw_accumulate == 2 and out[1][1][6] == 1
    E.set_accumulate(out, False)
    assert d1.dw_accumulate == 0 and out[1][1][6] == 0
