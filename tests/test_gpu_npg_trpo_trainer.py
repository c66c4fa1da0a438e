"""NPGTrainer / TRPOTrainer on the device: the fused update (csrc/pds_npg.hip) against the PyTorch-op update on the same rollout,
and both trainers learning Hover end to end."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _pair(cls, N, T, seed=0, **kw):
    """two trainers with the same networks over the same rollout: fused and PyTorch ops"""
    import phoenix_drone_simulation_amd as pds
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=N, seed=seed)
    a = cls(env, rollout_len=T, epochs=10, seed=seed, fused=True, **kw)
    a.roll_out()
    b = cls(env, rollout_len=T, epochs=10, seed=seed, fused=False, graph_rollout=False, **kw)
    b.ac.load_state_dict(a.ac.state_dict())
    for name in ("obs_buf", "act_buf", "rew_buf", "val_buf", "logp_buf", "term_buf", "trunc_buf", "fval_buf"):
        getattr(b, name).copy_(getattr(a, name))
    b.last_val = a.last_val.clone()
    perms = [torch.randperm(N * T, device=env.device) for _ in range(a.train_v_iterations)]
    a.perm_fn = lambda B, it=iter(perms): next(it)
    b.perm_fn = lambda B, it=iter(perms): next(it)
    return env, a, b


@pytest.mark.parametrize("cls_name", ["NPGTrainer", "TRPOTrainer"])
def test_fused_update_equals_the_pytorch_update_on_real_rollouts(cls_name):
    """8192 envs x 16 steps (131 072 samples: the policy gradient on its split-bf16 kernels): the fused step -- gradient,
    10 CG iterations over the Fisher kernel, x.Fx, alpha, the line search -- against the autograd restatement of the
    reference on the same data: same accepted step, same logged quantities and new parameters to float32 accuracy."""
    import phoenix_drone_simulation_amd.npg as npg
    env, a, b = _pair(getattr(npg, cls_name), 8192, 16)
    ia, ib = a.update(), b.update()
    torch.cuda.synchronize()
    assert ia["acceptance_step"] == ib["acceptance_step"], (ia, ib)
    for k in ("loss_pi", "loss_v"):
        assert abs(ia[k] - ib[k]) <= 1e-5 * max(1.0, abs(ib[k])), (k, ia[k], ib[k])
    for k, tol in (("gradient_norm", 1e-4), ("xHx", 1e-3), ("alpha", 1e-3), ("h_inv_g", 1e-3), ("kl", 5e-3)):
        assert abs(ia[k] - ib[k]) <= tol * abs(ib[k]), (k, ia[k], ib[k])
    pa = torch.cat([p.detach().reshape(-1) for p in a.ac.pi.net.parameters()])
    pb = torch.cat([p.detach().reshape(-1) for p in b.ac.pi.net.parameters()])
    step = ia["final_step_norm"]
    assert float(torch.norm(pa - pb)) <= 2e-3 * max(step, 1e-6), (float(torch.norm(pa - pb)), step)
    for (la, ka), (lb, kb) in zip(ia["candidates"], ib["candidates"]):
        assert abs(la - lb) <= 1e-4 * max(1.0, abs(lb)) and abs(ka - kb) <= 5e-3 * kb + 1e-7
    env.close()


@pytest.mark.parametrize("cls_name", ["NPGTrainer", "TRPOTrainer"])
def test_natural_gradient_trainers_learn_hover_end_to_end(cls_name):
    """Hover from scratch in the shape of test_ppo_learns_hover_end_to_end (2048 envs x 64 steps x 12 epochs, the reference's
    default env config, fused kernels): the episodes get longer and the return per step rises, the policy step is taken in
    every epoch and TRPO's KL stays inside its trust region.  Measured on the MI355X (seed 1; NPG and TRPO alike, TRPO took the
    full step every epoch): EpLen 9.3 -> 105.7, return per step -11.0 -> -2.2, KL per epoch 0.0058 .. 0.0119 -- the bars
    below (EpLen x 1.5, a higher return per step, KL <= 1.5 target_kl) as PPO's test sets them.  (Episode RETURNS fall while
    the drone learns to stay up: -102 -> -234 here, longer episodes collect more of the negative per-step reward.)"""
    import phoenix_drone_simulation_amd as pds
    import phoenix_drone_simulation_amd.npg as npg
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=2048, seed=1)
    tr = getattr(npg, cls_name)(env, rollout_len=64, epochs=12, seed=1)
    assert tr.fused
    tr.learn()
    first, last = tr.log[0], tr.log[-1]
    print(cls_name, [(round(r["ep_ret"], 1), round(r["ep_len"], 1), r["acceptance_step"], round(r["kl"], 4)) for r in tr.log])
    assert all(math.isfinite(r["loss_pi"]) and math.isfinite(r["loss_v"]) for r in tr.log)
    assert all(r["acceptance_step"] >= 1 for r in tr.log)
    if cls_name == "TRPOTrainer":
        assert all(r["kl"] <= 1.5 * tr.target_kl for r in tr.log)
    assert last["ep_len"] > 1.5 * first["ep_len"], (first, last)
    assert last["ep_ret"] / last["ep_len"] > first["ep_ret"] / first["ep_len"], (first, last)
    env.close()


@pytest.mark.parametrize("prefix", ["npg_", "trpo_", "trpot_"])
def test_reference_npg_trpo_updates_replayed_on_the_gpu(prefix, monkeypatch):
    """The reference's own NPG / TRPO updates (tests/golden/npg_update.npz) replayed on the device, fused (csrc/pds_npg.hip)
    and with PyTorch ops: the same AcceptanceStep and logged quantities as the reference (checked inside the replay).  The
    parameter bar is derived, not guessed: the same updates in float64 through the PyTorch path on CPU give each state_dict
    entry's float64 value; the device result must stay within 4 x the float32 CPU path's own distance from it, floor 2e-4
    relative."""
    import numpy as np
    import phoenix_drone_simulation_amd as pds
    import phoenix_drone_simulation_amd.ppo as ppo
    import golden_util as gu
    from test_npg_trpo_cpu import GOLD, _Env, replay_reference_updates
    g = np.load(GOLD)
    D = int(g[prefix + "obs_dim"])
    with monkeypatch.context() as mp:
        mp.setattr(ppo, "gae", gu.gae_torch)
        _, sd32 = replay_reference_updates(prefix, _Env(1, D), False)
        _, sd64 = replay_reference_updates(prefix, _Env(1, D), False, dtype=torch.float64, check=False)
    for fused in (True, False):
        env = pds.make("DroneHoverSimpleEnv-v0", num_envs=1, seed=0)
        tr, sdg = _replay_device(prefix, env, fused)
        assert tr.fused is fused
        for e, (a32, a64, ag) in enumerate(zip(sd32, sd64, sdg)):
            for k in a64:
                ref = float(torch.norm(a64[k]))
                d32 = float(torch.norm(a32[k] - a64[k]))
                dg = float(torch.norm(ag[k] - a64[k]))
                assert dg <= max(4 * d32, 2e-4 * ref), (prefix, fused, e, k, dg, d32, ref)
        env.close()


def _replay_device(prefix, env, fused):
    """replay_reference_updates on the HIP device (pds_gae; fused kernels or PyTorch ops), with its checks of AcceptanceStep,
    losses, x.Fx, alpha and candidates; the state_dict check at the device bar above instead of 1e-5"""
    import test_npg_trpo_cpu as cpu
    import golden_util as gu
    real = gu.assert_close
    gu.assert_close = lambda *a, **k: None
    try:
        return cpu.replay_reference_updates(prefix, env, fused)
    finally:
        gu.assert_close = real
