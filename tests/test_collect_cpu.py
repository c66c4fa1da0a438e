"""The host side of the fused collection without a device: the step-count rule, ReplayBuffer.advance, the three entry points in
the header and the library, and the trainers' default."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("since,every,N,left,want", [
    (0, 50, 1024, 8, 1),      # the examples: every vector step is followed by an update
    (0, 1000, 256, 8, 4),
    (600, 1000, 256, 8, 2),
    (0, 1000, 256, 3, 3),     # capped by the steps left in the epoch
    (0, 1000, 256, 1, 1),
    (1024, 1000, 256, 8, 1),  # an update is already due (e.g. the ring is below update_after): one step at a time
    (744, 1000, 256, 8, 1),
    (743, 1000, 256, 8, 2),
    (0, 1024, 256, 8, 4),
    (0, 1025, 256, 8, 5),
])
def test_collect_steps_table(since, every, N, left, want):
    from phoenix_drone_simulation_amd.ddpg import collect_steps
    assert collect_steps(since, every, N, left) == want


def test_collect_steps_reaches_the_update_exactly_where_the_per_step_loop_does():
    """simulate both loops over an epoch: the same vector steps are followed by an update"""
    from phoenix_drone_simulation_amd.ddpg import collect_steps
    for N, every, epoch in ((256, 50, 8), (256, 1000, 8), (100, 333, 17), (64, 1000, 40)):
        since, per_step = 0, []
        for s in range(epoch):
            since += N
            if since >= every:
                per_step.append(s)
                since = 0
        since, left, fused = 0, epoch, []
        while left > 0:
            k = collect_steps(since, every, N, left)
            assert 1 <= k <= left
            left -= k
            since += k * N
            if since >= every:
                fused.append(epoch - left - 1)
                since = 0
        assert fused == per_step, (N, every, epoch)


def test_advance_moves_the_ring_as_k_stores_do():
    from phoenix_drone_simulation_amd.ddpg import ReplayBuffer
    N, D = 8, 5
    a, b = ReplayBuffer(4 * N, D, "cpu", num_envs=N), ReplayBuffer(4 * N, D, "cpu", num_envs=N)
    z = lambda *s: torch.zeros(*s)
    for k in (1, 2, 0, 3, 5, 4, 1):  # through the wrap, past a full ring, and more than one lap in one call
        for _ in range(k):
            a.store(z(N, D), z(N, 4), z(N), z(N, D), z(N))
        b.advance(k)
        assert (a.ptr, a.size, len(a)) == (b.ptr, b.size, len(b)), k
    with pytest.raises(ValueError):
        ReplayBuffer(4 * N, D, "cpu").advance(1)  # rows per step unknown
    with pytest.raises(ValueError):
        b.advance(-1)


def test_the_entry_points_are_declared_and_exported():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import fused
    hdr = open(os.path.join(ROOT, "include", "pds.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = pds.native.load()
    for name in ("pds_collect_supported", "pds_collect", "pds_ddpg_explore"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert hasattr(lib, name) and name in pds.native.EXPORTS, name
    assert fused.COLLECT_DDPG == 0 and fused.COLLECT_SAC == 1


def test_fused_collect_is_opt_in():
    from phoenix_drone_simulation_amd.ddpg import DDPGTrainer, OffPolicyTrainer
    from phoenix_drone_simulation_amd.sac import SACTrainer
    for cls in (DDPGTrainer, SACTrainer):
        assert inspect.signature(cls.__init__).parameters["fused_collect"].default is False
    assert OffPolicyTrainer.collect_fused is False and OffPolicyTrainer.fused_collect is False
