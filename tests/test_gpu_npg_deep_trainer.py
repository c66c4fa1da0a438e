"""NPGTrainer / TRPOTrainer with deep_fused=True on the device: an actor with three or four hidden layers takes the fused policy step
on the kernels of csrc/pds_npg_deep.hip -- against the PyTorch-op step on the same rollout (the recipe and bars of
tests/test_gpu_npg_trpo_trainer.py), at construction, over a short TRPO run, and with a two-hidden-layer actor, where the keyword
changes nothing."""
import math
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

ACTORS = [((50, 30, 20), "relu"), ((32, 32, 32, 32), "tanh")]  # the architecture search's two deep actors


def _kw(hidden, act):
    return {"pi": {"hidden_sizes": tuple(hidden), "activation": act}, "val": {"hidden_sizes": (64, 64), "activation": "tanh"}}


def _pair(cls, N, T, ac_kwargs, seed=0):
    """two trainers with the same networks over the same rollout: the deep fused step and PyTorch ops"""
    import phoenix_drone_simulation_amd as pds
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=N, seed=seed)
    a = cls(env, rollout_len=T, epochs=10, seed=seed, fused=True, deep_fused=True, ac_kwargs=ac_kwargs)
    a.roll_out()
    b = cls(env, rollout_len=T, epochs=10, seed=seed, fused=False, graph_rollout=False, ac_kwargs=ac_kwargs)
    b.ac.load_state_dict(a.ac.state_dict())
    for name in ("obs_buf", "act_buf", "rew_buf", "val_buf", "logp_buf", "term_buf", "trunc_buf", "fval_buf"):
        getattr(b, name).copy_(getattr(a, name))
    b.last_val = a.last_val.clone()
    perms = [torch.randperm(N * T, device=env.device) for _ in range(a.train_v_iterations)]
    a.perm_fn = lambda B, it=iter(perms): next(it)
    b.perm_fn = lambda B, it=iter(perms): next(it)
    return env, a, b


@pytest.mark.parametrize("hidden,act", ACTORS, ids=["50x30x20-relu", "32x32x32x32-tanh"])
@pytest.mark.parametrize("cls_name", ["NPGTrainer", "TRPOTrainer"])
def test_deep_fused_update_equals_the_pytorch_update_on_real_rollouts(cls_name, hidden, act):
    """1 024 envs x 16 steps: the fused step -- gradient, 10 CG iterations over the deep Fisher kernel, x.Fx, alpha, the line search
    -- against the autograd restatement of the reference on the same data: same accepted step, same logged quantities and new
    parameters to float32 accuracy"""
    import phoenix_drone_simulation_amd.npg as npg
    env, a, b = _pair(getattr(npg, cls_name), 1024, 16, _kw(hidden, act))
    assert a.fused is True and a.fm_pi.deep and a.fm_pi.npg_deep and b.fused is False
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


@pytest.mark.parametrize("hidden,act", ACTORS, ids=["50x30x20-relu", "32x32x32x32-tanh"])
@pytest.mark.parametrize("cls_name", ["NPGTrainer", "TRPOTrainer"])
def test_construction_with_the_keyword_is_fused_without_a_warning(cls_name, hidden, act):
    import phoenix_drone_simulation_amd as pds
    import phoenix_drone_simulation_amd.npg as npg
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=256, seed=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tr = getattr(npg, cls_name)(env, rollout_len=8, epochs=2, seed=0, deep_fused=True, ac_kwargs=_kw(hidden, act))  # fused=None
        tr2 = getattr(npg, cls_name)(env, rollout_len=8, epochs=2, seed=0, fused=True, deep_fused=True, ac_kwargs=_kw(hidden, act))
    for t in (tr, tr2):
        assert t.fused is True and t.fm_pi.deep and t.fm_pi.npg_deep and t.fm_pi.n_hidden == len(hidden) and not t.fm_v.deep
    env.close()


def test_a_short_deep_trpo_run_stays_inside_the_trust_region():
    """three epochs of 512 x 32 on the fused deep step: finite losses, moved parameters, and KL <= 1.5 target_kl in every epoch --
    which holds by construction of the line search (a candidate beyond it is not accepted), not as a measured figure"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.npg import TRPOTrainer
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=512, seed=1)
    tr = TRPOTrainer(env, rollout_len=32, epochs=3, seed=1, deep_fused=True, ac_kwargs=_kw((50, 30, 20), "relu"))
    assert tr.fused is True and tr.fm_pi.npg_deep
    before = torch.cat([p.detach().reshape(-1).clone() for p in tr.ac.pi.net.parameters()])
    tr.learn()
    assert len(tr.log) == 3
    assert all(math.isfinite(r["loss_pi"]) and math.isfinite(r["loss_v"]) for r in tr.log)
    assert all(r["kl"] <= 1.5 * tr.target_kl for r in tr.log)
    after = torch.cat([p.detach().reshape(-1) for p in tr.ac.pi.net.parameters()])
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)
    env.close()


@pytest.mark.parametrize("cls_name", ["NPGTrainer", "TRPOTrainer"])
def test_with_a_shallow_actor_the_keyword_changes_no_bit(cls_name):
    import phoenix_drone_simulation_amd as pds
    import phoenix_drone_simulation_amd.npg as npg
    outs = []
    for deep_fused in (False, True):
        env = pds.make("DroneHoverSimpleEnv-v0", num_envs=512, seed=3)
        tr = getattr(npg, cls_name)(env, rollout_len=16, epochs=2, seed=3, deep_fused=deep_fused)
        assert tr.fused is True and not tr.fm_pi.deep and not tr.fm_pi.npg_deep
        tr.roll_out()
        info = tr.update()
        torch.cuda.synchronize()
        outs.append((torch.cat([p.detach().reshape(-1).clone() for p in tr.ac.parameters()]), info["acceptance_step"]))
        env.close()
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
