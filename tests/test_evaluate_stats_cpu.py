"""The host side of the running observation statistics (no GPU): OnlineMeanStd.merge_moments against numpy, the weights of
Augmented Random Search, ObsSums on synthetic slabs, the tree order of the composed path, and the new symbol's declaration."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oms(d):
    from phoenix_drone_simulation_amd.ppo import OnlineMeanStd
    return OnlineMeanStd(shape=(d,))


def _moments(x):
    return x.shape[0], x.mean(axis=0), ((x - x.mean(axis=0)) ** 2).sum(axis=0)


def test_merge_moments_is_the_mean_and_variance_of_everything_seen():
    """three unequal batches, the first into an empty OnlineMeanStd: after every merge mean and std are numpy's float64 mean and
    (biased) std of the concatenation.  Bound: the merge runs in float64 (errors ~1e-15) and stores float32, a relative error of at
    most 2^-24 = 6e-8 per element: 1e-6 relative."""
    rs = np.random.RandomState(0)
    D = 7
    batches = [rs.standard_normal((n, D)) * rs.uniform(0.1, 30.0, D) + rs.uniform(-50.0, 50.0, D) for n in (5, 1000, 37)]
    oms = _oms(D)
    address = (oms.mean.data_ptr(), oms.std.data_ptr(), oms.count.data_ptr())
    for j in range(3):
        oms.merge_moments(*_moments(batches[j]))
        seen = np.concatenate(batches[:j + 1])
        assert float(oms.count) == seen.shape[0]
        np.testing.assert_allclose(oms.mean.double().numpy(), seen.mean(axis=0), rtol=1e-6, atol=0)
        np.testing.assert_allclose(oms.std.double().numpy(), seen.std(axis=0), rtol=1e-6, atol=0)
        assert (oms.mean.data_ptr(), oms.std.data_ptr(), oms.count.data_ptr()) == address  # in place
    before = (oms.mean.clone(), oms.std.clone(), oms.count.clone())
    oms.merge_moments(0, np.zeros(D), np.zeros(D))  # an empty batch changes nothing
    assert all(torch.equal(a, b) for a, b in zip(before, (oms.mean, oms.std, oms.count)))


def test_merge_moments_is_not_the_reference_s_update():
    """update(x) takes the batch variance around the NEW mean and adds the delta^2 term on top: after a second batch with another
    mean its std is larger than the std of everything seen, which merge_moments gives"""
    rs = np.random.RandomState(1)
    a, b = rs.standard_normal((64, 3)), rs.standard_normal((64, 3)) + 5.0
    ref, mine = _oms(3), _oms(3)
    for x in (a, b):
        ref.update(torch.from_numpy(x).float())
        mine.merge_moments(*_moments(x))
    both = np.concatenate([a, b])
    np.testing.assert_allclose(mine.std.double().numpy(), both.std(axis=0), rtol=1e-6)
    np.testing.assert_allclose(mine.mean.double().numpy(), ref.mean.double().numpy(), rtol=1e-5)
    assert bool((ref.std > mine.std * 1.05).all())


def test_ars_pair_weights():
    from phoenix_drone_simulation_amd.es import ars_pair_weights
    # pairs (r+, r-): (1, 3) (5, 2) (0, 0.5) (10, 9); max: 3, 5, 0.5, 10 -> the best two are pairs 3 and 1; their returns 10, 9, 5, 2:
    # mean 6.5, variance (12.25 + 6.25 + 2.25 + 20.25) / 4 = 10.25
    f = torch.tensor([1.0, 3.0, 5.0, 2.0, 0.0, 0.5, 10.0, 9.0])
    sigma = 10.25 ** 0.5
    w = ars_pair_weights(f, 2)
    assert w.dtype == torch.float32 and tuple(w.shape) == (4,)
    np.testing.assert_allclose(w.numpy(), [0.0, 3.0 / sigma, 0.0, 1.0 / sigma], rtol=1e-6)
    # top_b = all pairs: every difference over the std of all eight returns
    w = ars_pair_weights(f, 4)
    np.testing.assert_allclose(w.numpy(), np.array([-2.0, 3.0, -0.5, 1.0]) / f.numpy().std(), rtol=1e-6)
    # a pair with a non-finite return gets 0 and takes no place
    g = f.clone(); g[6] = float("nan")
    w = ars_pair_weights(g, 2)
    assert float(w[3]) == 0.0 and bool(torch.isfinite(w).all())
    sigma = np.array([5.0, 2.0, 1.0, 3.0]).std()
    np.testing.assert_allclose(w.numpy(), [-2.0 / sigma, 3.0 / sigma, 0.0, 0.0], rtol=1e-6)
    g = f.clone(); g[7] = float("inf")
    assert float(ars_pair_weights(g, 4)[3]) == 0.0
    # at most top_b pairs carry weight
    rs = torch.Generator().manual_seed(0)
    r = torch.randn(64, generator=rs)
    for b in (1, 5, 32):
        assert int((ars_pair_weights(r, b) != 0).sum()) <= b
    assert not bool(ars_pair_weights(torch.ones(8), 2).any())  # sigma_R = 0: every difference is 0
    for bad in (0, 5):
        with pytest.raises(ValueError):
            ars_pair_weights(f, bad)


def _synthetic(P, tiles_per, D, rs, shifts):
    """observations, their per-policy shift, and the slab a kernel without rounding would write: each policy's observations dealt
    over its tiles_per x 4 slab parts"""
    slab = np.zeros((P * tiles_per, 4, 2, 64))
    xs = []
    for p in range(P):
        parts = []
        for t in range(tiles_per):
            for w in range(4):
                x = rs.standard_normal((rs.randint(1, 40), D)) * 3.0 + 10.0
                d = x - shifts[p]
                slab[p * tiles_per + t, w, 0, :D] = d.sum(axis=0)
                slab[p * tiles_per + t, w, 1, :D] = (d * d).sum(axis=0)
                parts.append(x)
        xs.append(np.concatenate(parts))
    return xs, slab


@pytest.mark.parametrize("shared", [True, False])
def test_obs_sums_moments_and_pooled(shared):
    """float64 moments from synthetic slabs (stored as float32: 2^-24 relative per entry; the shifts are near the mean, so S2 is
    well conditioned and 1e-5 covers the cancellation in S2 - S1^2 / n with room)"""
    from phoenix_drone_simulation_amd.evaluation import ObsSums
    rs = np.random.RandomState(3)
    P, tiles_per, D = 3, 2, 5
    shifts = np.tile(rs.uniform(9.0, 11.0, D), (P, 1)) if shared else rs.uniform(8.0, 12.0, (P, D))
    shifts = shifts.astype(np.float32).astype(np.float64)
    xs, slab = _synthetic(P, tiles_per, D, rs, shifts)
    sums = ObsSums(torch.from_numpy(slab).float(), [x.shape[0] for x in xs], shifts)
    assert tuple(sums.sum_d.shape) == (P, D) and sums.sum_d.dtype == torch.float64
    n, mean, m2 = sums.moments()
    for p in range(P):
        assert float(n[p]) == xs[p].shape[0]
        np.testing.assert_allclose(mean[p].numpy(), xs[p].mean(axis=0), rtol=1e-6)
        np.testing.assert_allclose(m2[p].numpy(), ((xs[p] - xs[p].mean(axis=0)) ** 2).sum(axis=0), rtol=1e-5)
    everything = np.concatenate(xs)
    n, mean, m2 = sums.pooled()
    assert float(n) == everything.shape[0] and tuple(mean.shape) == (D,)
    np.testing.assert_allclose(mean.numpy(), everything.mean(axis=0), rtol=1e-6)
    np.testing.assert_allclose(m2.numpy(), ((everything - everything.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-5)


def test_obs_sums_without_observations():
    from phoenix_drone_simulation_amd.evaluation import ObsSums
    sums = ObsSums(torch.zeros(2, 4, 2, 64), [0, 0], np.ones((2, 3)))
    n, mean, m2 = sums.moments()
    assert not bool(n.any()) and bool((mean == 1).all()) and not bool(m2.any())
    with pytest.raises(ValueError):
        ObsSums(torch.zeros(3, 4, 2, 64), [0, 0], np.ones((2, 3)))


def test_the_tree_order_of_the_composed_path():
    """tree_reduce_rows == a float32 loop in the documented order: env j + env j + 8, then j + (j + 4), then + 2, then + 1, per
    quarter tile; on values whose float32 sum depends on the order"""
    from phoenix_drone_simulation_amd.evaluation import tree_reduce_rows
    g = torch.Generator().manual_seed(5)
    N, D = 192, 6
    acc = (torch.randn(N, D, generator=g) * torch.tensor(10.0).pow(torch.randint(-3, 6, (N, D), generator=g).float())).float()
    got = tree_reduce_rows(acc)
    assert tuple(got.shape) == (3, 4, D) and got.dtype == torch.float32
    a = acc.numpy()
    want = np.zeros((3, 4, D), dtype=np.float32)
    for t in range(3):
        for w in range(4):
            for k in range(D):
                v = [np.float32(a[64 * t + 16 * w + j, k]) for j in range(16)]
                for h in (8, 4, 2, 1):
                    v = [np.float32(v[j] + v[j + h]) for j in range(h)]
                want[t, w, k] = v[0]
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    with pytest.raises(ValueError):
        tree_reduce_rows(torch.zeros(100, 3))


def test_the_symbol_is_declared_where_the_library_exports_it():
    from phoenix_drone_simulation_amd import native
    hdr = open(os.path.join(ROOT, "include", "pds.h")).read()
    assert re.search(r"\bint\s+pds_evaluate_policies_stats\s*\(", hdr)
    assert "pds_evaluate_policies_stats" in native.EXPORTS
    lib = native.load()
    assert len(lib.pds_evaluate_policies_stats.argtypes) == len(lib.pds_evaluate_policies_metrics.argtypes) + 1 == 16
    assert lib.pds_evaluate_policies_stats(None, 1, 64, None, None, None, None, 0.0, 1, None, None, None, None, None, None, None) == native.EINVAL


def test_the_trainer_s_new_arguments_are_checked():
    """(no env needed: the checks come first)"""
    from phoenix_drone_simulation_amd.es import ESTrainer

    class Env:
        num_envs = 256
    with pytest.raises(ValueError, match="shaping"):
        ESTrainer(Env(), 4, shaping="nes")
    with pytest.raises(ValueError, match="top_b"):
        ESTrainer(Env(), 4, shaping="ars", top_b=3)
