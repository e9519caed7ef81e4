"""Host side of the device-resident detection tail (csrc/detect_tail.hip), no GPU needed:

  * libradnet_hip.so exports the new entry points and radnet_hip.lib binds them with the header's argument lists;
  * a RADNet driven by duck-typed models ignores `device_tail` (there is nothing to launch on): same predict() either way;
  * the float floor division the tail restates on the device (npy_divmod: fmod-based) is pinned against `np.int64(v) // ratio`
    itself, for the ratios the GPU tests use -- and differs from floor(v / ratio) for ratio 0.1, which is why it matters;
  * the fp32 form of the score threshold."""
import ctypes as C

import numpy as np

RATIOS = (300 / 2048, 600 / 700, 1.0, 0.1)


def floor_divide_restated(a, b):
    """NumPy's / Python's float `a // b` (npy_divmod) written out with fmod, elementwise on float64 arrays; b != 0."""
    a = np.asarray(a, dtype=np.float64)
    mod = np.fmod(a, b)
    div = (a - mod) / b
    div = np.where((mod != 0) & ((b < 0) != (mod < 0)), div - 1.0, div)
    fl = np.floor(div)
    fl = np.where(div - fl > 0.5, fl + 1.0, fl)
    return np.where(div != 0, fl, np.copysign(0.0, a / b))


def test_library_exports_the_tail_with_the_bound_signatures():
    from radnet_hip import lib as L
    lib = L.load_library()
    i32, vp = C.c_int32, C.c_void_p
    want = {
        "radnet_detect_tail_out_bytes": (C.c_uint64, [i32]),
        "radnet_detect_tail": (C.c_int, [vp, C.POINTER(L.DetectTailDesc)]),
        "radnet_rois_from_proposals": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
        "radnet_predict_tile_detect": (C.c_int, [vp, C.POINTER(L.TileDesc), C.POINTER(L.DetectTailDesc)]),
    }
    declared = L.declared_symbols()
    for name, (res, args) in want.items():
        assert name in declared
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    # the size query needs no device: header + one record of 6 words per row
    assert lib.radnet_detect_tail_out_bytes(300) == 4 * (L.DETECT_HEADER + L.DETECT_RECORD * 300)
    assert lib.radnet_detect_tail_out_bytes(1) == 4 * (L.DETECT_HEADER + L.DETECT_RECORD)
    # the descriptor mirrors the header's layout (8-byte pointers and doubles, natural alignment)
    d = L.DetectTailDesc
    assert (d.rows.offset, d.bbox_threshold.offset, d.regr_std.offset, d.rpn_stride.offset, d.max_boxes.offset, d.out.offset) == (32, 48, 52, 72, 96, 104)
    assert C.sizeof(d) == 112


def test_fake_models_take_the_host_path_whatever_device_tail_says(monkeypatch):
    from faster_rcnn import rpn
    from faster_rcnn.config import Config
    from faster_rcnn.RADNet import RADNet
    from oracle import glue
    from test_oracle_glue import fake_detector

    class FakeDet:
        def __init__(self):
            self._f = fake_detector(7, 2, [])

        def predict(self, inputs):
            return self._f(inputs[1])

    class FakeRPN:
        def predict(self, X):
            h, w = glue.resnet50_feat_len(X.shape[1]), glue.resnet50_feat_len(X.shape[2])
            rs = np.random.RandomState(8 + int(abs(float(X.sum()))) % 1000)
            n = h * w * 12
            cls = (rs.permutation(n).astype(np.float32) / np.float32(n)).reshape(1, h, w, 12)
            return [cls, (rs.standard_normal((1, h, w, 48)) * 2.0).astype(np.float32), rs.standard_normal((1, h, w, 8)).astype(np.float32)]

    # the two device calls of the host path, restated by the oracle: this test runs without a GPU
    monkeypatch.setattr(rpn, "rpn_to_roi", lambda Y1, Y2, Cc, overlap_thresh=0.7: glue.rpn_to_roi(Y1, Y2, Cc, True, 300, overlap_thresh))
    monkeypatch.setattr(rpn, "non_max_suppression_fast", lambda b, p, overlap_thresh=0.9, max_boxes=300: glue.greedy_nms(b, p, overlap_thresh, max_boxes))
    Cc = Config()
    Cc.img_size, Cc.tile_size, Cc.tile_overlap = 160, 160, 80          # tiles arrive at network size: no resize
    img = np.random.RandomState(4).randint(0, 256, (240, 240, 3)).astype(np.uint8)
    assert RADNet.device_tail in (True, False) and RADNet.device_resident is True
    out = []
    for flag in (True, False):
        net = RADNet(Cc, FakeRPN(), FakeDet(), lambda x: x - np.float32(100.0))
        net.device_tail = flag
        assert not net._tail_on_device()
        out.append(net.predict([img]))
    assert len(out[0]) > 0
    assert out[0] == out[1]


def test_float_floor_division_restatement_is_numpy_s():
    v = np.arange(0, 5001)
    for ratio in RATIOS:
        ref = np.array([np.int64(x) // ratio for x in v])
        assert ref.dtype == np.float64
        assert np.array_equal(floor_divide_restated(v, ratio), ref), ratio
        assert np.array_equal(floor_divide_restated(-v, ratio), np.array([np.int64(-x) // ratio for x in v])), ratio
        assert [int(round(x // ratio)) for x in (7.0, 480.0)] == [int(round(x)) for x in floor_divide_restated([7.0, 480.0], ratio)]
    # ... and it is not floor(v / ratio): for 0.1 the two differ wherever v / 0.1 rounds up to an integer
    naive = np.floor(v / 0.1)
    assert np.int64(1) // 0.1 == 9.0 and naive[1] == 10.0
    assert np.count_nonzero(naive != floor_divide_restated(v, 0.1)) >= 4000
    for ratio in RATIOS[:3]:
        assert np.array_equal(np.floor(v / ratio), floor_divide_restated(v, ratio))


def test_threshold_in_fp32():
    from radnet_hip.engine import threshold_f32
    s = np.float32(0.7)
    below, above = np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(1))
    for t in (0.7, 0.0, 0.5, np.float64(0.7), np.float32(0.7), 1):
        u = np.float32(threshold_f32(t))
        assert float(u) == threshold_f32(t)
        for x in (below, s, above, np.float32(0), np.float32(1)):
            assert bool(x < t) == bool(x < u), (t, x)
