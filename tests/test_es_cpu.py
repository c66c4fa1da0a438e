"""Host-side tests of the evolution strategy (es.py, csrc/pds_es.hip): fitness shaping, the workspace size, every refusal of
the two entry points (all of them come before the first device call, so no GPU is needed), and the recipe of
ESTrainer.tell restated in numpy on a quadratic."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import phoenix_drone_simulation_amd as pds
from phoenix_drone_simulation_amd import es

EINVAL = pds.native.EINVAL
FAKE = C.c_void_p(4096)  # a non-NULL pointer for the arguments a refused call never touches


def test_centered_ranks_range_sum_ties_and_nan():
    g = torch.Generator().manual_seed(0)
    f = torch.randn(64, generator=g)
    u = es.centered_ranks(f)
    assert u.dtype == torch.float32 and u.shape == (64,)
    assert float(u.min()) == -0.5 and float(u.max()) == 0.5
    assert abs(float(u.double().sum())) < 1e-6  # even P: the ranks are symmetric about 0
    assert torch.equal(torch.argsort(u), torch.argsort(f))  # order preserving
    assert torch.equal(torch.sort(u).values, torch.arange(64, dtype=torch.float32) / 63 - 0.5)
    # ties are broken by index: the earlier of two equal values gets the lower rank
    u = es.centered_ranks(torch.tensor([1.0, 0.0, 1.0, 0.0]))
    assert torch.equal(u, torch.tensor([2.0, 0.0, 3.0, 1.0]) / 3 - 0.5)
    # NaN ranks below everything, -inf included (index order among the NaNs)
    u = es.centered_ranks(torch.tensor([0.5, float("nan"), -math.inf, 2.0, float("nan"), math.inf]))
    assert torch.equal(u, torch.tensor([3.0, 0.0, 2.0, 4.0, 1.0, 5.0]) / 5 - 0.5)
    assert torch.equal(es.centered_ranks(torch.tensor([3.0])), torch.zeros(1))


def test_pair_weights_shape_and_values():
    u = torch.tensor([0.5, -0.5, 0.1, 0.3, -0.2, -0.2])
    w = es.pair_weights(u)
    assert w.shape == (3,)
    assert torch.equal(w, torch.tensor([0.5, 0.1, -0.2]) - torch.tensor([-0.5, 0.3, -0.2]))
    w = es.pair_weights(es.centered_ranks(torch.arange(8.0)))
    assert torch.allclose(w, torch.full((4,), -1.0 / 7))


def test_workspace_floats():
    lib = pds.native.load()
    ws = lib.pds_es_workspace_floats
    for n in (1, 9, 4504):
        assert ws(n, 1) == n
        sizes = [ws(n, p) for p in range(1, 200)]
        steps = np.diff(sizes)
        assert set(steps.tolist()) <= {0, n}  # monotone, and a jump is exactly one [n] slab
        chunk = 1 + int(np.flatnonzero(steps)[0])  # pairs 1 .. chunk share the first slab
        assert chunk >= 2
        for p in range(1, 200):
            assert ws(n, p) == -(-p // chunk) * n
    assert ws(0, 1) == EINVAL and ws(1, 0) == EINVAL


def _perturb(mu=FAKE, n=8, pairs=2, sigma=0.1, seed=1, generation=0, pair_base=0, theta=FAKE):
    return pds.native.load().pds_es_perturb(mu, n, pairs, sigma, seed, generation, pair_base, theta, None)


def _gradient(w=FAKE, mu=FAKE, n=8, pairs=2, scale=-1.0, l2=0.0, seed=1, generation=0, pair_base=0, grad=FAKE, ws=FAKE):
    return pds.native.load().pds_es_gradient(w, mu, n, pairs, scale, l2, seed, generation, pair_base, grad, ws, None)


@pytest.mark.parametrize("kw", [dict(mu=None), dict(theta=None), dict(n=0), dict(n=-3), dict(pairs=0), dict(pairs=-1),
                                dict(sigma=0.0), dict(sigma=-0.1), dict(sigma=math.nan), dict(sigma=math.inf),
                                dict(pair_base=2 ** 56), dict(pair_base=2 ** 56 - 2),            # (base + 2) * 1 = 2^56
                                dict(n=17, pairs=1, pair_base=(2 ** 56 + 2) // 3 - 1),              # Q = 3: (base + 1) * 3 >= 2^56
                                dict(pair_base=2 ** 64 - 1), dict(n=2 ** 40, pairs=2 ** 40)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_perturb_refusals(kw):
    assert _perturb(**kw) == EINVAL


@pytest.mark.parametrize("kw", [dict(w=None), dict(grad=None), dict(ws=None), dict(n=0), dict(pairs=0), dict(pairs=-5),
                                dict(scale=math.nan), dict(scale=math.inf), dict(scale=-math.inf), dict(l2=math.nan),
                                dict(l2=math.inf), dict(pair_base=2 ** 56), dict(pair_base=2 ** 56 - 2),
                                dict(n=17, pairs=1, pair_base=(2 ** 56 + 2) // 3 - 1), dict(pair_base=2 ** 64 - 1),
                                dict(mu=None, n=0)],
                         ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_gradient_refusals(kw):
    assert _gradient(**kw) == EINVAL


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_recipe_converges_on_a_quadratic(seed):
    """ESTrainer.tell in numpy: centred ranks, pair weights, scale -1 / (2 H sigma), Adam with the expressions of adam_kernel
    (csrc/pds_train.hip), on fitness = -|theta - target|^2.  n = 170, P = 256, sigma = 0.05, lr = 0.02, l2 = 0, 60 generations,
    mu0 = 0, target ~ 0.5 N(0, 1): |mu - target| must fall below 0.25 of its initial value (over 64 seeds of numpy's normals
    the ratio was 0.049 - 0.118: a factor 2 over the worst seed)."""
    n, P, sigma, lr, b1, b2, eps = 170, 256, 0.05, 0.02, 0.9, 0.999, 1e-8
    H = P // 2
    rs = np.random.RandomState(seed)
    target = 0.5 * rs.standard_normal(n)
    mu, m, v = np.zeros(n), np.zeros(n), np.zeros(n)
    d0 = np.linalg.norm(mu - target)
    for g in range(60):
        noise = rs.standard_normal((H, n))
        theta = np.empty((P, n))
        theta[0::2], theta[1::2] = mu + sigma * noise, mu - sigma * noise
        fitness = -((theta - target) ** 2).sum(axis=1)
        w = es.pair_weights(es.centered_ranks(torch.from_numpy(fitness))).double().numpy()
        grad = (-1.0 / (2 * H * sigma)) * (w @ noise)
        step = g + 1
        m = b1 * m + (1 - b1) * grad
        v = b2 * v + (1 - b2) * grad * grad
        bc1, bc2s = 1 - b1 ** step, math.sqrt(1 - b2 ** step)
        mu = mu - (lr / bc1) * (m / (np.sqrt(v) / bc2s + eps))
    ratio = np.linalg.norm(mu - target) / d0
    print(f"seed {seed}: |mu - target| ratio {ratio:.4f}")
    assert ratio < 0.25
