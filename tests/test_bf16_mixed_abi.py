"""bf16-mixed training mode, host side (no GPU needed): the new entry points and struct are declared, exported and bound with the
header's layout, program op CONV_FWD_BF16 documents its K split in i[1], the split rule is the documented fixed function of
(M, N, K), and precision="bf16-mixed" passes the argument checks of FasterRCNNEngine / build_models before any device is
touched -- while VGG16, the cont_train.py mode and NativeTrainStep refuse it."""
import ctypes as C
import os
import re
import types

import pytest

from radnet_hip import lib as L

NEW = ("radnet_adam_step_bf16", "radnet_conv_fwd_bf16_split", "radnet_conv_bf16_pick_split", "radnet_conv_bf16_tile_shape")


def _lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def _header():
    with open(L.HEADER_PATH) as f:
        return f.read()


def test_header_declares_and_library_exports_bf16_mixed_entry_points():
    names = L.declared_symbols()
    lib = _lib()
    for n in NEW:
        assert n in names, "include/radnet_hip.h does not declare %s" % n
        assert hasattr(lib, n), "libradnet_hip.so does not export %s" % n
        assert getattr(lib, n).argtypes is not None, "%s has no ctypes binding" % n
    assert lib.radnet_adam_step_bf16.argtypes[-2] == C.POINTER(L.AdamBf16)
    assert lib.radnet_conv_bf16_tile_shape.restype == C.c_int64
    assert lib.radnet_conv_bf16_tile_shape.argtypes == [C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]


def test_adam_bf16_struct_matches_header():
    m = re.search(r"typedef struct radnet_adam_bf16 \{(.*?)\} radnet_adam_bf16;", _header(), re.S)
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
    assert [f[0] for f in L.AdamBf16._fields_] == [f[0] for f in fields]
    kinds = {"int64_t": C.c_int64, "int32_t": C.c_int32, "uint16_t*": C.c_void_p}
    assert [f[1] for f in L.AdamBf16._fields_] == [kinds[f[1]] for f in fields]
    # natural C alignment: off 0, k 8, n 12, ldw 16, wt 24, ldk 32, size 40
    assert [getattr(L.AdamBf16, n).offset for n in ("off", "k", "n", "ldw", "wt", "ldk")] == [0, 8, 12, 16, 24, 32]
    assert C.sizeof(L.AdamBf16) == 40


def test_op_documents_k_split_in_i1():
    text = _header()
    assert re.search(r"CONV_FWD_BF16 conv, p\[0\] = wt .*i\[0\] = ldk, i\[1\] = ksplit", text)
    assert L.OP_CONV_FWD_BF16 == 17


def test_pick_split_rule():
    lib = _lib()
    pick = lib.radnet_conv_bf16_pick_split
    # stage-5 training shapes at 20 RoIs (M = 980): 64x64 tiles, 128 workgroups -> two slices
    assert pick(980, 512, 1024) == 2
    assert pick(980, 512, 4608) == 2
    assert pick(980, 2048, 512) == 1              # 512 workgroups already
    assert pick(2394, 512, 9216) == 1             # rpn_conv1 at 600x1000: 304 workgroups
    assert pick(2394, 64, 512) == 2               # rpn_heads: 38 workgroups, 16 K tiles -> 8 per slice at most
    assert pick(100, 64, 256) == 1                # 8 K tiles: no slice may hold fewer than 8
    for M, N, K in [(1, 1, 1), (49, 2048, 65536), (98, 32, 200000), (5000, 512, 9216), (0, 5, 5)]:
        s = pick(M, N, K)
        assert 1 <= s <= 16 and s & (s - 1) == 0
        assert s == 1 or (K + 31) // 32 >= 8 * s
    assert pick(49, 64, 65536) == 16              # the cap


class _Stop(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to select a device ends the constructor: what ran before it are the argument checks."""
    import torch

    def stop(*a, **k):
        raise _Stop()
    monkeypatch.setattr(torch.cuda, "set_device", stop)


def test_bf16_mixed_passes_argument_checks_before_device(no_device):
    from faster_rcnn import models as M
    from faster_rcnn.config import Config
    from radnet_hip.engine import FasterRCNNEngine
    with pytest.raises(_Stop):
        FasterRCNNEngine(Config(), precision="bf16-mixed")
    with pytest.raises(_Stop):
        M.build_models(Config(), precision="bf16-mixed")
    for bad in ("bf16_mixed", "mixed", "fp16-mixed"):
        with pytest.raises(ValueError):
            FasterRCNNEngine(Config(), precision=bad)
        with pytest.raises(ValueError):
            M.build_models(Config(), precision=bad)


def test_bf16_mixed_refused_for_vgg16_cont_and_native(no_device):
    from faster_rcnn import models as M
    from faster_rcnn.config import Config
    from radnet_hip.engine import FasterRCNNEngine
    from radnet_hip.engine_cont import ContEngine
    from radnet_hip.engine_vgg import VGG16Engine
    from radnet_hip.native import NativeTrainStep
    Cv = Config()
    Cv.network = "vgg16"
    with pytest.raises(NotImplementedError):
        M.build_models(Cv, precision="bf16-mixed")
    with pytest.raises(NotImplementedError):
        VGG16Engine(Cv, precision="bf16-mixed")
    with pytest.raises(NotImplementedError):
        ContEngine(Config(), precision="bf16-mixed")
    with pytest.raises(NotImplementedError):
        FasterRCNNEngine(Config(), workload="cont", precision="bf16-mixed")
    with pytest.raises(NotImplementedError):
        M.build_models(Config(), workload="cont", precision="bf16-mixed")
    with pytest.raises(NotImplementedError):
        NativeTrainStep(types.SimpleNamespace(precision="bf16-mixed"))
