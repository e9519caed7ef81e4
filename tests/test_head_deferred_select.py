"""Where TrainStep selects the deferred weight-gradient form of the classifier's backward (head_backward(defer_wgrad=True) followed by
engine.head_update_deferred) and where it keeps the paired program + Adam #2: only a step whose gradient is complete inside one backward
program and goes straight into the optimizer may use it.  Step logic only, on the recording stand-in of test_dp_deferred (no kernels)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_dp_deferred import FakeEngine, _free_port


class DeferrableEngine(FakeEngine):
    """The stand-in with the deferred form on offer: records which of the two updates a step took."""

    def head_deferred_ok(self, hp):
        return True

    def head_backward(self, hp, accumulate=True, loss_out=None, on_part=None, defer_wgrad=False):
        self.log.append(("head_bwd", self.k, bool(defer_wgrad)))
        super().head_backward(hp, accumulate, loss_out, on_part)

    def head_update_deferred(self, hp, grad_scale=1.0):
        self.log.append(("deferred_update", self.k, float(self.head_arena.g[0]) * grad_scale))
        self.head_arena.p -= grad_scale * self.head_arena.g
        self.head_arena.g.zero_()


def _batch(n=1):
    return [dict(img=np.zeros((4, 4, 3), np.uint8), bboxes=[dict({"class": "fg"}, x1=0, x2=2, y1=0, y2=2)], width=8, height=8) for _ in range(n)]


def _steps(eng, n_images=1, **kw):
    from radnet_hip.trainer import TrainStep
    np.random.seed(64)
    ts = TrainStep(eng, **kw)
    for _ in range(3):
        ts.step(_batch(n_images))
    ts.flush()
    return [e[0] for e in eng.log if e[0] in ("adam_head", "deferred_update")], [e[2] for e in eng.log if e[0] == "head_bwd"]


def test_one_rank_one_image_takes_the_deferred_form():
    eng = DeferrableEngine(0)
    updates, deferred = _steps(eng)
    assert updates == ["deferred_update"] * 3 and deferred == [True] * 3
    assert np.allclose(eng.head_arena.p.numpy(), -(1 + 2 + 3))          # every step's gradient applied once


def test_an_engine_without_the_form_keeps_adam():
    eng = FakeEngine(0)
    updates, _ = _steps(eng)
    assert updates == ["adam_head"] * 3


def test_a_deferred_update_keeps_the_paired_program():
    eng = DeferrableEngine(0)
    updates, deferred = _steps(eng, defer_head_update=True)
    assert updates == ["adam_head"] * 3 and deferred == [False] * 3


def test_images_run_one_by_one_keep_the_paired_program():
    """Two images per step through separate backward programs: their gradients are added up in the arena before Adam #2."""
    eng = DeferrableEngine(0)
    eng.anchor_targets_launch = lambda gt, width, height, W, H, slot=0: dict(slot=slot)      # (the stand-in counts a step per image otherwise)
    eng.k = 0
    updates, deferred = _steps(eng, n_images=2)
    assert updates == ["adam_head"] * 3 and deferred == [False] * 6


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "rock-art-radnet_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng = DeferrableEngine(rank)
    out[rank] = _steps(eng, world_size=world, defer_head_update=False)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_keep_the_paired_program():
    """world_size 2 over gloo: the gradients are exchanged between the backward and Adam #2, so they must be in the arena."""
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for rank in range(world):
        updates, deferred = out[rank]
        assert updates == ["adam_head"] * 3 and deferred == [False] * 3
