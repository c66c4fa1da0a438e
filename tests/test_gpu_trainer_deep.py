"""PPOTrainer on actors and critics with three and four hidden layers (csrc/pds_mlp_deep.hip through fused.FusedMLP): the
architecture grid of the reference's experiments/01_find_NN_architecture -- a deep actor beside the default (64, 64) critic, and
both deep -- on Hover and Circle.  fused=None resolves to the kernels without a warning, the one-launch rollout is refused and
the trainer settles on the per-step kernels, the rollout's bookkeeping and one policy / one value gradient on real rollout data
agree with the PyTorch path (the recipe and bars of test_fused_update_matches_the_autograd_update, tests/test_trainer.py), and
NPGTrainer still takes a deep actor to PyTorch ops."""
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

DEEP3 = {"pi": {"hidden_sizes": (50, 30, 20), "activation": "relu"}, "val": {"hidden_sizes": (64, 64), "activation": "tanh"}}
DEEP4 = {"pi": {"hidden_sizes": (32, 32, 32, 32), "activation": "tanh"}, "val": {"hidden_sizes": (64, 64, 64), "activation": "tanh"}}
CASES = [("DroneHoverSimpleEnv-v0", DEEP3, (True, False)), ("DroneCircleSimpleEnv-v0", DEEP4, (True, True)),
         ("DroneCircleSimpleEnv-v0", DEEP3, (True, False)), ("DroneHoverSimpleEnv-v0", DEEP4, (True, True))]


@pytest.mark.parametrize("task,ac_kwargs,deep", CASES, ids=["hover-3", "circle-4", "circle-3", "hover-4"])
def test_ppo_trainer_runs_deep_networks_on_the_fused_kernels(task, ac_kwargs, deep):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer, gae, ppo_loss, value_loss
    env = pds.make(task, num_envs=256, seed=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr = PPOTrainer(env, rollout_len=16, epochs=4, seed=2, ac_kwargs=ac_kwargs)
    assert tr.fused is True and (tr.fm_pi.deep, tr.fm_v.deep) == deep
    assert tr.fm_pi.n_hidden == len(ac_kwargs["pi"]["hidden_sizes"]) and tr.fm_v.n_hidden == len(ac_kwargs["val"]["hidden_sizes"])
    assert not hasattr(tr.fm_pi, "m")
    # ---- the rollout (the probe of the one-launch form is refused; the per-step kernels run) and the PyTorch modules ----
    tr.roll_out()
    assert tr.fused_rollout is False
    ac, T, N = tr.ac, tr.T, tr.N
    adv, target_v, _ = gae(tr.rew_buf, tr.val_buf, tr.term_buf, tr.trunc_buf, tr.fval_buf, tr.last_val, 0.99, 0.95, 0.0, 10.0)
    obs = ac.obs_oms(tr.obs_buf.reshape(T * N, -1)).contiguous()
    data = dict(obs=obs, act=tr.act_buf.reshape(T * N, -1), adv=adv.reshape(-1), log_p=tr.logp_buf.reshape(-1) + 0.1,
                target_v=target_v.reshape(-1))
    with torch.no_grad():
        d, logp = ac.pi(obs, data["act"])
        assert torch.allclose(logp, tr.logp_buf.reshape(-1), atol=2e-4)
        assert torch.allclose(ac.v(obs), tr.val_buf.reshape(-1), atol=1e-4)
    tr.fm_pi.ppo_grad(obs, data["act"].contiguous(), data["adv"].contiguous(), data["log_p"].contiguous(), ac.pi.log_std, 0.2)
    got_pi = tr.fm_pi.flat_grad.clone()
    idx = torch.randperm(T * N, device=obs.device)[:1000]
    tr.fm_v.value_grad(obs, data["target_v"].contiguous(), index=idx)
    got_v = tr.fm_v.flat_grad.clone()
    grads = [p.grad for p in list(ac.pi.net.parameters()) + list(ac.v.parameters())]
    for p in list(ac.pi.net.parameters()) + list(ac.v.parameters()):
        p.grad = None
    ppo_loss(ac, data, 0.2, 0.0)[0].backward()
    value_loss(ac, obs[idx], data["target_v"][idx]).backward()
    want_pi = torch.cat([p.grad.reshape(-1) for p in ac.pi.net.parameters()])
    want_v = torch.cat([p.grad.reshape(-1) for p in ac.v.parameters()])
    assert torch.allclose(got_pi, want_pi, rtol=1e-3, atol=1e-6 * max(1.0, float(want_pi.abs().max())))
    assert torch.allclose(got_v, want_v, rtol=1e-3, atol=1e-6 * max(1.0, float(want_v.abs().max())))
    for p, g in zip(list(ac.pi.net.parameters()) + list(ac.v.parameters()), grads):
        p.grad = g  # (the views into the kernels' flat buffers again)
    # ---- one whole epoch: rollout (a captured graph of the per-step path by default), update on the deep kernels --------
    before = [p.detach().clone() for p in ac.pi.net.parameters()]
    info = tr.learn_one_epoch()
    assert tr.fused_rollout is False
    assert math.isfinite(info["loss_pi"]) and math.isfinite(info["loss_v"])
    assert any(not torch.equal(a, b) for a, b in zip(before, ac.pi.net.parameters()))
    assert all(bool(torch.isfinite(p).all()) for p in ac.parameters())
    with pytest.raises(NotImplementedError, match="fused_rollout"):
        PPOTrainer(env, rollout_len=16, epochs=4, seed=2, ac_kwargs=ac_kwargs, fused_rollout=True)
    env.close()


def test_npg_trainer_keeps_a_deep_actor_on_pytorch_ops():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.npg import NPGTrainer
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=256, seed=2)
    with pytest.warns(RuntimeWarning, match="do not cover these networks"):
        tr = NPGTrainer(env, rollout_len=16, epochs=4, seed=2, ac_kwargs=DEEP3)
    assert tr.fused is False and tr.fm_pi is None
    with pytest.raises(NotImplementedError, match="2 hidden"):
        NPGTrainer(env, rollout_len=16, epochs=4, seed=2, ac_kwargs=DEEP3, fused=True)
    env.close()
