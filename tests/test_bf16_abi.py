"""The bf16 inference entry points are declared, exported and bound (no GPU needed), and the engine's precision argument is
checked before anything touches a device."""
import os
import re

import pytest

from radnet_hip import lib as L

NEW = ("radnet_weights_to_bf16", "radnet_conv_fwd_bf16")


def _lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load_library()


def test_header_declares_and_library_exports_bf16_entry_points():
    names = L.declared_symbols()
    lib = _lib()
    for n in NEW:
        assert n in names, "include/radnet_hip.h does not declare %s" % n
        assert hasattr(lib, n), "libradnet_hip.so does not export %s" % n
        assert getattr(lib, n).argtypes is not None, "%s has no ctypes binding" % n


def test_op_kind_matches_header():
    with open(L.HEADER_PATH) as f:
        text = f.read()
    m = re.search(r"RADNET_OP_CONV_FWD_BF16\s*=\s*(\d+)", text)
    assert m is not None
    assert L.OP_CONV_FWD_BF16 == int(m.group(1)) == 17
    kinds = [v for k, v in vars(L).items() if k.startswith("OP_")]
    assert kinds.count(L.OP_CONV_FWD_BF16) == 1


def test_precision_argument_checked_first():
    from faster_rcnn import models as M
    from faster_rcnn.config import Config
    from radnet_hip.engine import FasterRCNNEngine
    with pytest.raises(ValueError):
        FasterRCNNEngine(Config(), precision="fp16")
    with pytest.raises(ValueError):
        M.build_models(Config(), precision="tf32")
    C = Config()
    C.network = "vgg16"
    with pytest.raises(NotImplementedError):
        M.build_models(C, precision="bf16")
