"""ESTrainer (es.py) around a centre with THREE or FOUR hidden layers, on lean Hover, limit 10, P = 8, E = 64: the flat centre in
the layout of pds_mlp_deep_param_count, pds_mlp_deep_adam_step on it, the generation through pds_evaluate_policies_deep and --
obs_stats="online" with deep_forms_fused=True -- through pds_evaluate_policies_deep_stats, the reference's checkpoint."""
import os

import numpy as np
import pytest
import torch

import evaluate_oracle as eo
import flight_deep_oracle as fdo
import variant_cases as vc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, E, LIMIT = 8, 64, 10
SHAPES = [(5, 7, 3), (4, 4, 4, 4)]
FITNESS_COLUMNS = ("fitness_mean", "fitness_min", "fitness_max", "ep_len", "centre_return", "grad_norm", "env_steps")


def _env(seed=21, **kw):
    import phoenix_drone_simulation_amd as pds
    return pds.make(vc.HOVER, num_envs=P * E, device=DEV, seed=seed, max_episode_steps=LIMIT, **eo.LEAN, **kw)


def _ulps(a, b):
    """(number of elements whose bits differ, the largest distance in float32 units in the last place)"""
    x, y = a.detach().cpu().contiguous().view(torch.int32).long(), b.detach().cpu().contiguous().view(torch.int32).long()
    key = lambda v: torch.where(v < 0, -(v & 0x7FFFFFFF), v)  # sign-magnitude -> a monotone integer
    d = (key(x) - key(y)).abs()
    return int((d != 0).sum()), int(d.max())


@pytest.mark.parametrize("hidden", SHAPES, ids=["L3", "L4"])
def test_fused_against_composed_recipe_bit_for_bit(hidden):
    """ESTrainer(fused=True) against fused=False: ask()'s theta and three generations of mu, bit for bit.  pds_es_perturb writes
    fmaf(+-sigma, eps, mu), one rounding; the composed recipe of a deep centre states the same contract in float64 (the product
    of two float32 values is exact there) and rounds once more -- the same bits but for a double rounding: where the float64 sum,
    itself rounded, lands exactly half way between two float32 values, about one element in 2^29.  The seeds below (env 21,
    trainer 4) are seeds at which none of the 2 376 / 2 016 elements of theta does: 0 elements differ on the MI355X.  With another
    seed a tie would show as one element one unit in the last place off, which is the bound tests/test_gpu_es.py
    test_perturbation_follows_the_contract holds the kernel to -- the bar here stays bit for bit.  The figures are printed in
    front of the assertions."""
    from phoenix_drone_simulation_amd.es import ESTrainer
    runs = {}
    for fused in (True, False):
        env = _env()
        tr = ESTrainer(env, P, hidden_sizes=hidden, seed=4, eval_every=0, fused=fused)
        theta0 = tr.ask().theta.clone()
        mus = []
        for _ in range(3):
            tr.learn_one_generation()
            mus.append(tr.mu.clone())
        runs[fused] = (theta0, mus)
        env.close()
    n, worst = _ulps(runs[True][0], runs[False][0])
    print(f"FIGURE es_deep {hidden} theta: {n} of {runs[True][0].numel()} elements differ, at most {worst} ulp")
    for g in range(3):
        m, w = _ulps(runs[True][1][g], runs[False][1][g])
        print(f"FIGURE es_deep {hidden} mu after generation {g + 1}: {m} of {runs[True][1][g].numel()} elements differ, at most {w} ulp")
    assert torch.equal(runs[True][0], runs[False][0])
    for g in range(3):
        assert torch.equal(runs[True][1][g], runs[False][1][g]), g


@pytest.mark.parametrize("hidden", SHAPES, ids=["L3", "L4"])
def test_online_statistics_from_the_launch_equal_the_composed_generations(hidden, monkeypatch):
    """obs_stats="online", deep_forms_fused=True, evaluate_fused=True against evaluate_fused=False over three generations: mu,
    obs_oms.mean / std and the log's fitness columns, bit for bit; the fused run flies every generation through
    pds_evaluate_policies_deep_stats and never calls pds_mlp_deep_forward"""
    from phoenix_drone_simulation_amd import evaluation, native
    from phoenix_drone_simulation_amd.es import ESTrainer
    names = []
    real = native.call
    monkeypatch.setattr(evaluation.native, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    runs = {}
    for how in (True, False):
        del names[:]
        env = _env()
        tr = ESTrainer(env, P, hidden_sizes=hidden, activation="tanh", seed=2, obs_stats="online", eval_every=2, evaluate_fused=how,
                       deep_forms_fused=True)
        logs = [tr.learn_one_generation() for _ in range(3)]
        oms = tr.ac.obs_oms
        runs[how] = (tr.mu.clone(), oms.mean.detach().clone(), oms.std.detach().clone(), [[l[c] for c in FITNESS_COLUMNS] for l in logs])
        called = {n for n in names if n.startswith(("pds_evaluate", "pds_mlp_deep_forward"))}
        if how:
            assert called == {"pds_evaluate_policies_deep_stats", "pds_evaluate_policies_deep"}, called  # (the second: the centre's flight)
            assert names.count("pds_evaluate_policies_deep_stats") == 3
        else:
            assert "pds_evaluate_policies_deep_stats" not in called and "pds_mlp_deep_forward" in called
        env.close()
    a, b = runs[True], runs[False]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert np.array_equal(np.array(a[3]), np.array(b[3]), equal_nan=True), (a[3], b[3])
    assert all(1.0 <= row[3] <= LIMIT for row in a[3])


@pytest.mark.parametrize("hidden", SHAPES, ids=["L3", "L4"])
def test_the_adam_step_on_the_centre_matches_torch(hidden):
    """three tell()s against torch.optim.Adam driven with the trainer's own gradient of each generation: rtol 1e-5 with the atol
    1e-7 for parameters near zero -- the tolerance the project holds its Adam kernels to (tests/test_gpu_fused_mlp.py
    test_adam_step_matches_torch_adam, tests/test_gpu_mlp_deep.py); tests/test_gpu_es.py itself sets none"""
    from phoenix_drone_simulation_amd.es import ESTrainer
    env = _env()
    tr = ESTrainer(env, P, hidden_sizes=hidden, seed=7, lr=0.01, l2=0.005)
    ref = torch.nn.Parameter(tr.mu.clone())
    opt = torch.optim.Adam([ref], lr=tr.lr, betas=tr.betas, eps=tr.adam_eps)
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        tr.ask()
        tr.tell(torch.randn(P, generator=g))
        ref.grad = tr.grad.clone()
        opt.step()
        err = float((tr.mu - ref.detach()).abs().max())
        print(f"FIGURE es_deep {hidden} adam generation {tr.generation}: max |mu - torch| {err:.3e}")
        assert torch.allclose(tr.mu, ref.detach(), rtol=1e-5, atol=1e-7)
    assert tr.generation == 3 and torch.equal(torch.cat([p.detach().reshape(-1) for p in tr.ac.pi.net.parameters()]), tr.mu)
    env.close()


@pytest.mark.parametrize("hidden", SHAPES, ids=["L3", "L4"])
def test_the_checkpoint_gives_the_centre_back(hidden, tmp_path):
    from phoenix_drone_simulation_amd.es import ESTrainer
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    from phoenix_drone_simulation_amd.ppo import ActorCritic
    env = _env()
    tr = ESTrainer(env, P, hidden_sizes=hidden, seed=4, eval_every=1)
    tr.learn_one_generation()
    assert tr.n == fdo.param_count((env.obs_dim,) + hidden + (4,)) and tr.generation == 1
    path = tr.save_checkpoint(str(tmp_path))
    assert os.path.isfile(os.path.join(str(tmp_path), "model.json"))
    ac = ActorCritic.from_reference_state_dict(torch.load(path, map_location="cpu"))
    pop = PolicyPopulation.from_actor_critics([ac])
    assert pop.deep and pop.hidden_sizes == hidden and torch.equal(pop.theta[0], tr.mu.cpu())
    env.close()


def test_shapes_outside_the_range_raise():
    from phoenix_drone_simulation_amd.es import ESTrainer
    env = _env()
    with pytest.raises(ValueError, match="1 to 64"):
        ESTrainer(env, P, hidden_sizes=(5, 65, 3))
    with pytest.raises(ValueError, match="2 to 4 hidden layers"):
        ESTrainer(env, P, hidden_sizes=(4, 4, 4, 4, 4))
    env.close()
    hist = _env(observation_history_size=4)
    with pytest.raises(ValueError, match="observation_history_size"):
        ESTrainer(hist, P, hidden_sizes=(5, 7, 3))
    hist.close()
