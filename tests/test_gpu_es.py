"""GPU tests of the evolution strategy: pds_es_perturb / pds_es_gradient (csrc/pds_es.hip) against the noise contract of
DESIGN.md section 4 -- the noise for every comparison comes from pds_gaussian_sample on zeros, the entry point that
tests/test_gpu_sampler.py holds draw for draw against the float64 restatement of that contract (tests/sampler_oracle.py; the
same file checks the rows of pds_es_perturb against the restatement directly, without the detour through the sampler) -- and
ESTrainer (es.py) on a quadratic and end to end on Hover."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import phoenix_drone_simulation_amd as pds
from phoenix_drone_simulation_amd import es
from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
from phoenix_drone_simulation_amd.fused import gaussian_sample
from phoenix_drone_simulation_amd.ppo import ActorCritic

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED, GENERATION = 0x5EED0123456789, 3
SIGMA = float(np.float32(0.05))
NS = (1, 3, 8, 9, 170, 4504)          # one lane; a partial block; one / two blocks; unaligned rows (170 % 4 = 2); the Hover actor
PAIR_KEYS = ("1", "2", "c-1", "c", "c+1")
GUARD = 64                             # floats behind every output that the kernels must leave alone


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def chunk():
    """the chunk length of pds_es_gradient, read off pds_es_workspace_floats"""
    ws = pds.native.load().pds_es_workspace_floats
    c = 1
    while ws(1, c + 1) == 1:
        c += 1
    return c


def pairs_of(key):
    c = chunk()
    return {"1": 1, "2": 2, "c-1": c - 1, "c": c, "c+1": c + 1}[key]


def noise(n, pairs, seed=SEED, generation=GENERATION, pair_base=0):
    """eps [pairs, n] (float32, device) through pds_gaussian_sample on zeros: the reference of the contract"""
    Q = (n + 7) // 8
    out, logp = torch.empty(pairs * Q, 8, device=DEV), torch.empty(pairs * Q, device=DEV)
    gaussian_sample(torch.zeros(pairs * Q, 8, device=DEV), torch.zeros(8, device=DEV), out, logp, seed, generation,
                    id_base=pair_base * Q)
    return out.reshape(pairs, 8 * Q)[:, :n].contiguous()


@functools.lru_cache(maxsize=None)
def reference(n):
    """(mu [n], eps [c + 1, n]) as float64 numpy arrays of float32 values, computed once per n and left unchanged; fewer pairs
    are the leading rows (sample id = pair * Q + q)"""
    g = torch.Generator().manual_seed(100 + n)
    mu = torch.randn(n, generator=g)
    eps = noise(n, chunk() + 1).cpu()
    mu64, eps64 = mu.double().numpy(), eps.double().numpy()
    mu64.setflags(write=False); eps64.setflags(write=False)
    return mu64, eps64


def perturb(mu, n, pairs, sigma=SIGMA, seed=SEED, generation=GENERATION, pair_base=0):
    buf = torch.full((2 * pairs * n + GUARD,), 12345.0, device=DEV)
    rc = pds.native.load().pds_es_perturb(_ptr(mu), n, pairs, sigma, seed, generation, pair_base, _ptr(buf), _stream())
    assert rc == pds.native.OK
    assert bool((buf[2 * pairs * n:] == 12345.0).all()), "pds_es_perturb wrote behind theta"
    return buf[:2 * pairs * n].reshape(2 * pairs, n)


def gradient(w, mu, n, pairs, scale, l2, seed=SEED, generation=GENERATION, pair_base=0):
    lib = pds.native.load()
    nws = lib.pds_es_workspace_floats(n, pairs)
    ws = torch.full((nws + GUARD,), 12345.0, device=DEV)
    grad = torch.full((n + GUARD,), 12345.0, device=DEV)
    rc = lib.pds_es_gradient(_ptr(w), _ptr(mu), n, pairs, scale, l2, seed, generation, pair_base, _ptr(grad), _ptr(ws), _stream())
    assert rc == pds.native.OK
    assert bool((ws[nws:] == 12345.0).all()) and bool((grad[n:] == 12345.0).all()), "pds_es_gradient wrote out of bounds"
    return grad[:n]


@pytest.mark.parametrize("key", PAIR_KEYS)
@pytest.mark.parametrize("n", NS)
def test_perturbation_follows_the_contract(n, key):
    """Every element within one float32 unit in the last place of float32(float64(mu) +- float64(sigma) * float64(eps)): the
    float64 product of two float32 values is exact, so the only difference to fmaf is the double rounding.  Derived bound."""
    pairs = pairs_of(key)
    mu64, eps64 = reference(n)
    eps64 = eps64[:pairs]
    mu = torch.tensor(mu64, dtype=torch.float32, device=DEV)
    theta = perturb(mu, n, pairs)
    got = theta.cpu().numpy()
    want = np.empty((2 * pairs, n), dtype=np.float32)
    want[0::2] = (mu64 + float(SIGMA) * eps64).astype(np.float32)
    want[1::2] = (mu64 - float(SIGMA) * eps64).astype(np.float32)
    ok = (got == want) | (got == np.nextafter(want, np.float32(-np.inf))) | (got == np.nextafter(want, np.float32(np.inf)))
    print(f"n {n} pairs {pairs}: {int((got != want).sum())} of {got.size} elements one ulp off, {int((~ok).sum())} further off")
    assert ok.all()
    assert torch.equal(perturb(mu, n, pairs), theta)  # a second call: the same bits


@pytest.mark.parametrize("n", (9, 170, 4504))
def test_perturbation_slices_and_counters(n):
    mu = torch.tensor(reference(n)[0], dtype=torch.float32, device=DEV)
    whole = perturb(mu, n, 8)
    assert torch.equal(perturb(mu, n, 5, pair_base=3), whole[6:16])  # a slice of the pairs: bitwise the rows of the whole
    assert not torch.equal(perturb(mu, n, 8, generation=GENERATION + 1), whole)
    assert not torch.equal(perturb(mu, n, 8, seed=SEED + 1), whole)


@pytest.mark.parametrize("l2", (0.0, 0.005))
@pytest.mark.parametrize("key", PAIR_KEYS)
@pytest.mark.parametrize("n", NS)
def test_gradient_against_float64(n, key, l2):
    """|error_j| <= (pairs + 4) 2^-24 (|scale| sum_i |w_i eps_ij| + |l2 mu_j|): the a-priori bound of float32 summation, valid
    for any order of the sum.  Derived, not measured."""
    pairs = pairs_of(key)
    mu64, eps64 = reference(n)
    eps64 = eps64[:pairs]
    g = torch.Generator().manual_seed(7 * n + pairs)
    w = torch.randn(pairs, generator=g)
    scale, l2 = float(np.float32(-1.0 / (2 * pairs * SIGMA))), float(np.float32(l2))
    mu = torch.tensor(mu64, dtype=torch.float32, device=DEV)
    wd = w.to(DEV)
    got = gradient(wd, mu, n, pairs, scale, l2)
    w64 = w.double().numpy()
    want = scale * (w64 @ eps64) + l2 * mu64
    bound = (pairs + 4) * 2.0 ** -24 * (abs(scale) * (np.abs(w64)[:, None] * np.abs(eps64)).sum(axis=0) + np.abs(l2 * mu64))
    err = np.abs(got.cpu().double().numpy() - want)
    print(f"n {n} pairs {pairs} l2 {l2}: worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert torch.equal(gradient(wd, mu, n, pairs, scale, l2), got)  # two calls: equal bits
    if l2 == 0.0:  # d_mu = NULL skips the l2 term
        assert torch.equal(gradient(wd, None, n, pairs, scale, 0.005), got)


@pytest.mark.parametrize("n", (9, 4504))
def test_gradient_slice_of_the_pairs(n):
    """pair_base shifts the noise: the gradient of pairs 3 .. 7 alone equals the whole sum with the other weights zero, to the
    summation bound (the chunks fall differently, so not bitwise)."""
    _, eps64 = reference(n)
    w = torch.zeros(8)
    w[3:] = torch.tensor([0.5, -0.25, 1.0, 0.125, -1.0])
    got = gradient(w[3:].contiguous().to(DEV), None, n, 5, 1.0, 0.0, pair_base=3).cpu().double().numpy()
    want = w.double().numpy() @ eps64[:8]
    bound = 9 * 2.0 ** -24 * (np.abs(w.double().numpy())[:, None] * np.abs(eps64[:8])).sum(axis=0)
    assert (np.abs(got - want) <= bound).all()


# ---- the trainer -----------------------------------------------------------------------------------------------------------
LEAN = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0)


def param_count(d_in, h1, h2, d_out=4):
    return h1 * d_in + h1 + h2 * h1 + h2 + d_out * h2 + d_out


@pytest.mark.parametrize("fused", (True, False))
def test_trainer_converges_on_the_quadratic(fused):
    """ESTrainer.ask / tell on the quadratic of tests/test_es_cpu.py (P = 256, sigma = 0.05, lr = 0.02, l2 = 0, 60 generations,
    mu0 = 0, target ~ 0.5 N(0, 1)), the fitness computed in torch from theta -- no env is stepped; the bar is that test's 0.25.
    The env handle gives the shapes only: 256 x 64 envs, because the constructor refuses E = 512 / 256 = 2; no hidden sizes give
    n = 170 with this env's inputs, D -> 2 -> 12 -> 4 is the actor nearest to it (n = 174 at D = 42; rows 8-byte aligned)."""
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=256 * 64, device=DEV, seed=3, **LEAN)
    try:
        tr = es.ESTrainer(env, 256, hidden_sizes=(2, 12), sigma=0.05, lr=0.02, l2=0.0, seed=11, fused=fused)
        assert tr.n == param_count(env.obs_dim, 2, 12) and 160 <= tr.n <= 180
        g = torch.Generator().manual_seed(5)
        target = (0.5 * torch.randn(tr.n, generator=g)).to(DEV)
        tr.mu.zero_()
        d0 = float((tr.mu - target).norm())
        for _ in range(60):
            pop = tr.ask()
            assert pop.theta.data_ptr() == tr._theta.data_ptr() and pop.theta.is_cuda  # the tensor the kernel wrote: no host copy
            tr.tell(-((pop.theta - target) ** 2).sum(dim=1))
        ratio = float((tr.mu - target).norm()) / d0
        print(f"fused={fused}: |mu - target| ratio {ratio:.4f}")
        assert tr.generation == 60
        assert ratio < 0.25
    finally:
        env.close()


def _run(tmp=None):
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=8 * 64, device=DEV, seed=21, max_episode_steps=30, **LEAN)
    tr = es.ESTrainer(env, 8, seed=4, eval_every=1)
    mu0 = tr.mu.clone()
    logs = [tr.learn_one_generation() for _ in range(2)]
    return env, tr, mu0, logs


def test_trainer_end_to_end(tmp_path):
    env, tr, mu0, logs = _run()
    try:
        assert tr.n == param_count(env.obs_dim, 50, 50) and tr.generation == 2 and [l["generation"] for l in logs] == [1, 2]
        for l in logs:
            assert all(math.isfinite(v) for v in l.values()), l
            assert l["fitness_min"] <= l["fitness_mean"] <= l["fitness_max"]
            assert 1.0 <= l["ep_len"] <= 30.0 and l["env_steps"] >= 2 * 512 and l["grad_norm"] > 0.0
        assert not torch.equal(tr.mu, mu0)  # the centre moved
        # the actor's parameters ARE the flat centre
        flat = torch.cat([p.detach().reshape(-1) for p in tr.ac.pi.net.parameters()])
        assert torch.equal(flat, tr.mu)
        # same seeds, same bits
        env2, tr2, mu02, _ = _run()
        try:
            assert torch.equal(mu02, mu0) and torch.equal(tr2.mu, tr.mu)
        finally:
            env2.close()
        # the checkpoint is the reference's and gives the centre back bitwise
        path = tr.save_checkpoint(str(tmp_path))
        assert os.path.isfile(os.path.join(str(tmp_path), "model.json"))
        ac = ActorCritic.from_reference_state_dict(torch.load(path, map_location="cpu"))
        pop = PolicyPopulation.from_actor_critics([ac])
        assert torch.equal(pop.theta[0], tr.mu.cpu())
        tr.write_progress_csv(os.path.join(str(tmp_path), "progress.csv"))
        assert len(open(os.path.join(str(tmp_path), "progress.csv")).read().splitlines()) == 3
        # the env is usable after a reset()
        obs, _ = env.reset()
        obs, r, term, trunc, info = env.step(torch.zeros(512, 4, device=DEV))
        assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(r).all())
    finally:
        env.close()


def test_trainer_refusals_and_nonfinite_fitness():
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=512, device=DEV, seed=1, **LEAN)
    try:
        for population in (7, 6, 16):  # odd; 512 % 6 != 0; E = 32 is not a multiple of 64
            with pytest.raises(ValueError):
                es.ESTrainer(env, population)
        tr = es.ESTrainer(env, 8, hidden_sizes=(3, 8))
        tr.ask()
        with pytest.raises(FloatingPointError):
            tr.tell(torch.full((8,), float("nan")))
        assert tr.generation == 0
    finally:
        env.close()
