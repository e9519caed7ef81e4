"""bench.py --dump-outputs: the files a run writes -- names, dtypes, the fixed sample of a large array, the size limit (no GPU:
the helpers only)."""
import os

import numpy as np
import pytest


@pytest.fixture
def bench(monkeypatch):
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", os.environ.get("GPU_MAX_HW_QUEUES", "4"))     # bench sets a default on import
    import bench as B
    return B


def test_train_outputs_are_written_with_their_dtypes_and_a_fixed_sample(bench, tmp_path):
    big = np.random.RandomState(0).standard_normal(bench.DUMP_SAMPLE * 3 + 7).astype(np.float32)
    losses = {"rpn_cls": 1.5, "det_acc": 0.25, "n_head": 1}
    weights = {"rpn_conv1": {"kernel": big.reshape(-1, 1), "bias": np.arange(5, dtype=np.float32)}}
    state = np.random.get_state()[1].copy()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bench.train_outputs(losses, weights))
    assert np.array_equal(np.random.get_state()[1], state)           # the step's global stream is left alone
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["loss_det_acc.npy", "loss_n_head.npy", "loss_rpn_cls.npy", "weight_rpn_conv1_bias.npy", "weight_rpn_conv1_kernel.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == (np.float64 if n.startswith("loss_") else np.float32)
        assert np.array_equal(a, b)                                   # same sample on every run
    assert np.load(tmp_path / "a" / "loss_rpn_cls.npy").tolist() == [1.5]
    assert np.array_equal(np.load(tmp_path / "a" / "weight_rpn_conv1_bias.npy"), np.arange(5, dtype=np.float32))
    k = np.load(tmp_path / "a" / "weight_rpn_conv1_kernel.npy")
    assert k.shape == (bench.DUMP_SAMPLE,) and np.isin(k, big).all()


def test_dump_refuses_more_than_the_limit(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path), {"x": np.zeros(300, np.float64)})
    assert not (tmp_path / "x.npy").exists()


def test_detections_are_one_sorted_array(bench):
    dets = {"human": ([[1, 2, 3, 4], [0, 0, 9, 9]], [0.5, 0.9]), "boat": ([[5, 5, 6, 6]], [0.7])}
    a = bench.detection_outputs(dets, {"boat": 0, "human": 1, "bg": 6})["detections"]
    assert a.dtype == np.float64 and a.shape == (3, 6)
    assert a.tolist() == [[0, 5, 5, 6, 6, 0.7], [1, 0, 0, 9, 9, 0.9], [1, 1, 2, 3, 4, 0.5]]
    assert bench.detection_outputs({}, {"bg": 6})["detections"].shape == (0, 6)
