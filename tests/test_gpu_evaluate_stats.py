"""The observation sums of the one-launch policy evaluation on the GPU (include/pds.h pds_evaluate_policies_stats, csrc/pds_evaluate.h
STATS; evaluation.evaluate_population(..., obs_stats=True), ObsSums; ESTrainer(obs_stats="online")): the kernel's slab is bit for bit
what the composed path sums with one torch op per difference, product and sum and adds in the kernel's tree order, the other
outputs do not move, the sums are the sums of the observations the policies acted on, and the trainer's running statistics follow
them."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_evaluate import CONFIGS, HOVER, TAKEOFF, _equal, _make, _population, _snapshot, _unchanged

pytestmark = pytest.mark.gpu
U = 2.0 ** -24  # unit roundoff of float32


def _both(config, P, E, limit=None, max_steps=None, seed=0):
    """-> (fused with stats and metrics, composed with stats and metrics, fused metrics without stats), each as evaluate_population
    returns it, on three envs of the same seed"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    pop = _population(config, P, seed=seed)
    envs = [_make(config, P * E, max_episode_steps=limit) for _ in range(3)]
    fused = evaluate_population(envs[0], pop, fused=True, metrics=True, obs_stats=True, max_steps=max_steps)
    composed = evaluate_population(envs[1], pop, fused=False, metrics=True, obs_stats=True, max_steps=max_steps)
    plain = evaluate_population(envs[2], pop, fused=True, metrics=True, max_steps=max_steps)
    for e in envs:
        e.close()
    return pop, fused, composed, plain


def _flat(out):
    """returns, lengths, costs, raw metrics (and the slab, where there is one) as a list of tensors"""
    xs = [out[0], out[1], out[2], out[3].raw]
    if len(out) == 5:
        xs.append(out[4].slab)
    return xs


@pytest.mark.parametrize("E", [64, 192])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_the_slab_is_the_composed_path_s_bit_for_bit(config, P, E):
    """slab, returns, lengths, costs and raw metrics of the stats launch == the composed path's, on the bits; the first four ==
    the metrics launch without stats; in cases that hold both endings (TakeOff: every episode is cut)"""
    limit = CONFIGS[config][3]
    pop, fused, composed, plain = _both(config, P, E)
    length, sums = fused[1], fused[4]
    early, cut = int((length < limit).sum()), int((length == limit).sum())
    D = pop.d_in
    print(f"{config} P={P} E={E}: {early} episodes ended before step {limit}, {cut} were cut there; "
          f"{float(sums.count.sum()):.0f} observations summed")
    assert tuple(sums.slab.shape) == (P * E // 64, 4, 2, 64) and sums.slab.dtype == torch.float32 and not sums.slab.is_cuda
    assert _equal(_flat(fused), _flat(composed)), [float((a - b).abs().max()) for a, b in zip(_flat(fused), _flat(composed))]
    assert _equal(_flat(fused)[:4], _flat(plain))
    assert torch.equal(sums.count, length.double().sum(dim=1)) and torch.equal(composed[4].count, sums.count)
    assert not bool(sums.slab[..., D:].any())  # features >= D are zero
    assert early + cut == P * E
    if CONFIGS[config][0] == TAKEOFF:
        assert early == 0 and cut == P * E
    else:
        assert early >= 1 and cut >= 1, (early, cut)


def test_two_teams_and_an_odd_tile_count():
    """257 policies x 64 episodes: above 256 tiles the launcher may put two teams in a block, and the last block is half filled"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    for config, limit in (("hover_lean", 40), ("hover_default", 40)):
        pop = _population(config, 257, seed=3)
        env_f, env_c = _make(config, 257 * 64, max_episode_steps=limit), _make(config, 257 * 64, max_episode_steps=limit)
        fused = evaluate_population(env_f, pop, fused=True, metrics=True, obs_stats=True)
        composed = evaluate_population(env_c, pop, fused=False, metrics=True, obs_stats=True)
        env_f.close(); env_c.close()
        early = int((fused[1] < limit).sum())
        print(f"{config} 257 x 64: {early} of {257 * 64} episodes ended before step {limit}")
        assert _equal(_flat(fused), _flat(composed))
        assert tuple(fused[4].slab.shape) == (257, 4, 2, 64)
        assert 1 <= early < 257 * 64


def _logged(config, P, E, limit=None, max_steps=None):
    """The composed path with its float64 log of (d [N, D], alive [N]) per step, and the fused path beside it"""
    from phoenix_drone_simulation_amd import evaluation
    pop = _population(config, P)
    env_f, env_c = _make(config, P * E, max_episode_steps=limit), _make(config, P * E, max_episode_steps=limit)
    fused = evaluation.evaluate_population(env_f, pop, fused=True, obs_stats=True, max_steps=max_steps)
    log = []
    evaluation._OBS_STATS_LOG = log
    try:
        composed = evaluation.evaluate_population(env_c, pop, fused=False, obs_stats=True, max_steps=max_steps)
    finally:
        evaluation._OBS_STATS_LOG = None
    env_f.close(); env_c.close()
    d = torch.stack([x for x, _ in log]).numpy()      # [T, N, D] float64
    on = torch.stack([a for _, a in log]).numpy()     # [T, N] bool
    return pop, fused, composed, d, on


def _check_against_float64(slab, d, on, D, T):
    """every slab entry within (T + 6) u sum |terms| of the float64 sum of its own terms: the (n - 1) u sum |x| bound of a
    recursive float32 sum of n terms, n - 1 <= T adds per lane + 4 tree levels, + the roundings of d and of d * d"""
    N = d.shape[1]
    worst = 0.0
    for which, terms in ((0, d), (1, d * d)):
        terms = np.where(on[:, :, None], terms, 0.0)
        per_env, per_env_abs = terms.sum(axis=0), np.abs(terms).sum(axis=0)  # [N, D]
        want = per_env.reshape(N // 64, 4, 16, D).sum(axis=2)
        room = (T + 6) * U * per_env_abs.reshape(N // 64, 4, 16, D).sum(axis=2)
        got = slab[:, :, which, :D].double().numpy()
        err = np.abs(got - want)
        assert np.all(err <= room), (which, float((err - room).max()))
        worst = max(worst, float((err / np.maximum(room, 1e-300)).max()))
    return worst


@pytest.mark.parametrize("config", ["hover_default", "hover_lean"])  # with and without standardisation
def test_the_sums_mean_what_they_say(config):
    P, E = 2, 64
    T = CONFIGS[config][3]
    pop, fused, composed, d, on = _logged(config, P, E)
    assert (pop.mean is not None) == (config == "hover_default")
    sums, length = fused[3], fused[1]
    assert _equal([sums.slab], [composed[3].slab])
    assert d.shape == (T, P * E, pop.d_in)
    assert np.array_equal(on.sum(axis=0), length.reshape(-1).numpy().astype(np.int64))  # alive in front of step s <=> s < length
    worst = _check_against_float64(sums.slab, d, on, pop.d_in, T)
    print(f"{config}: largest error / bound {worst:.4f}")
    assert torch.equal(sums.count, length.double().sum(dim=1))
    # ObsSums: float64 sums over tiles and waves; mean and M2 of the observations themselves
    shift = pop.mean.double().numpy() if pop.mean is not None else np.zeros((P, pop.d_in))
    n, mean, m2 = sums.moments()
    for p in range(P):
        rows = slice(p * E, (p + 1) * E)
        dd = d[:, rows][on[:, rows]]  # [count, D]
        assert float(n[p]) == dd.shape[0]
        cnt = dd.shape[0]
        # the float32 sums carry e1 <= (T + 6) u sum |d| and e2 <= (T + 6) u sum d^2 (above); the float64 steps behind them add
        # nothing of that size.  mean = shift + S1 / n: e1 / n.  M2 = S2 - S1^2 / n: e2 + (2 |S1| e1 + e1^2) / n.
        e1, e2 = (T + 6) * U * np.abs(dd).sum(axis=0), (T + 6) * U * (dd * dd).sum(axis=0)
        s1 = dd.sum(axis=0)
        tiny = 1e-12  # (the float64 operations of both sides)
        assert np.all(np.abs(sums.sum_d[p].numpy() - s1) <= e1 + tiny)
        x = dd + shift[p]
        assert np.all(np.abs(mean[p].numpy() - x.mean(axis=0)) <= e1 / cnt + tiny * (1 + np.abs(shift[p])))
        want_m2 = ((dd - dd.mean(axis=0)) ** 2).sum(axis=0)
        assert np.all(np.abs(m2[p].numpy() - want_m2) <= e2 + (2 * np.abs(s1) * e1 + e1 * e1) / cnt + tiny * (1 + want_m2))


def test_a_tile_that_stops_early_and_one_that_flies_to_the_end():
    """P = 1, E = 64: ONE tile.  Every episode ends at step 3 (the env's TimeLimit) of 40 steps flown: the tile stops, its network
    waves leave through the stop and store the sums of exactly the steps 0, 1, 2.  TakeOff never terminates: all T rows."""
    pop, fused, composed, d, on = _logged("hover_lean", 1, 64, limit=3, max_steps=40)
    sums = fused[3]
    assert torch.equal(fused[1], torch.full((1, 64), 3.0)) and float(sums.count[0]) == 3 * 64
    assert _equal([sums.slab], [composed[3].slab])
    assert d.shape[0] == 40 and on[:3].all() and not on[3:].any()
    _check_against_float64(sums.slab, d, on, pop.d_in, 3)
    assert bool((sums.slab[:, :, 1, :pop.d_in].sum(dim=(0, 1)) > 0).any())

    T = CONFIGS["takeoff"][3]
    pop, fused, composed, d, on = _logged("takeoff", 1, 64)
    sums = fused[3]
    assert torch.equal(fused[1], torch.full((1, 64), float(T))) and float(sums.count[0]) == T * 64
    assert _equal([sums.slab], [composed[3].slab])
    assert on.all() and d.shape[0] == T
    if np.isfinite(d).all():
        _check_against_float64(sums.slab, d, on, pop.d_in, T)


def test_metrics_false_drops_the_metrics_and_keeps_the_bits():
    from phoenix_drone_simulation_amd.evaluation import ObsSums, evaluate_population
    pop = _population("hover_default", 2)
    env_a, env_b = _make("hover_default", 128), _make("hover_default", 128)
    with_m = evaluate_population(env_a, pop, fused=True, metrics=True, obs_stats=True)
    without = evaluate_population(env_b, pop, fused=True, obs_stats=True)
    env_a.close(); env_b.close()
    assert len(without) == 4 and isinstance(without[3], ObsSums)
    assert _equal(list(with_m[:3]) + [with_m[4].slab], list(without[:3]) + [without[3].slab])


def test_abi_refusals_leave_the_handle_as_it_was():
    """PDS_EINVAL for a NULL or misaligned d_obs_sums, PDS_EUNSUPPORTED without auto_reset and for an env configuration without
    kernel; nothing moves"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    pop = _population("hover_default", 2)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(e, obs, sums="own", off=0):
        dpop = pop.to(e.device)
        out = [torch.zeros(128, device=e.device) for _ in range(3)]
        raw = torch.zeros(128, 8, device=e.device)
        slab = torch.zeros(2 * 4 * 2 * 64 + 4, device=e.device)
        rc = e.lib.pds_evaluate_policies_stats(e._handle, 2, 64, C.byref(dpop.mlp(0)), p(dpop.theta), p(dpop.mean), p(dpop.std),
                                               dpop.eps, 10, p(obs), p(out[0]), p(out[1]), p(out[2]), p(raw),
                                               None if sums is None else p(slab, off), e._stream())
        torch.cuda.synchronize()
        return rc, slab

    env = pds.make(HOVER, num_envs=128, seed=3)
    obs, _ = env.reset()
    snap = _snapshot(env)
    rc, _ = call(env, obs, sums=None)
    assert rc == native.EINVAL
    rc, slab = call(env, obs, off=4)
    assert rc == native.EINVAL and b"d_obs_sums" in env.lib.pds_last_error(env._handle) and not bool(slab.any())
    _unchanged(env, snap)
    env.step(torch.zeros(128, 4, device=env.device))  # still a reset handle
    obs, _ = env.reset()
    rc, slab = call(env, obs)  # and the call itself
    assert rc == native.OK and bool(slab.any())
    env.close()

    env = pds.make(HOVER, num_envs=128, seed=3, auto_reset=False)
    obs, _ = env.reset()
    snap = _snapshot(env)
    rc, _ = call(env, obs)
    assert rc == native.EUNSUPPORTED and b"auto_reset" in env.lib.pds_last_error(env._handle)
    _unchanged(env, snap)
    env.close()

    env = pds.make(HOVER, num_envs=128, seed=3, use_ground_effect=True)
    obs, _ = env.reset()
    snap = _snapshot(env)
    rc, _ = call(env, obs)
    assert rc == native.EUNSUPPORTED
    _unchanged(env, snap)
    env.close()


def _chan(count, mean, std, n_b, mean_b, m2_b):
    """float64 numpy: (count, mean, std) merged with a batch's (n_b, mean_b, M2_b)"""
    n = count + n_b
    delta = mean_b - mean
    m2 = count * std ** 2 + m2_b + delta ** 2 * (count * n_b / n)
    return n, mean + delta * n_b / n, np.sqrt(m2 / n)


def test_the_es_trainer_keeps_its_statistics_running():
    """ESTrainer(obs_stats="online"), 4 policies x 64 episodes, two generations, once with the stats kernel and once on the
    composed path.  After every generation obs_oms == the float64 Chan merge of the composed path's pooled moments into what it
    held before: both sides compute in float64 from the same float32 inputs, and the result is stored as float32 -- a relative
    error of at most 2^-24 = 6e-8 per element, so 1e-6 relative.  The [P, D] rows the kernel reads keep their address.  Both runs
    see the same returns and the same statistics: the same centre on the bits."""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.es import ESTrainer
    kw = dict(observation_noise=0, domain_randomization=0.0, motor_thrust_noise=0.0)
    runs = {}
    for how in (True, False):
        env = pds.make(HOVER, num_envs=4 * 64, seed=5, max_episode_steps=30, **kw)
        tr = ESTrainer(env, 4, seed=2, obs_stats="online", eval_every=0, evaluate_fused=how)
        oms = tr.ac.obs_oms
        assert float(oms.count) > 0  # started as "warmup" does
        address = (tr._mean_P.data_ptr(), tr._std_P.data_ptr(), oms.mean.data_ptr(), oms.std.data_ptr())
        seen, merge = [], tr.merge_obs_sums
        tr.merge_obs_sums = lambda s, seen=seen, merge=merge: (seen.append(s), merge(s))
        history = []
        for g in range(2):
            before = (float(oms.count), oms.mean.double().cpu().numpy(), oms.std.double().cpu().numpy())
            used = tr._mean_P.clone()
            tr.learn_one_generation()
            assert len(seen) == g + 1
            assert torch.equal(seen[g].shift.float(), used.cpu())  # generation g flew with what the generations before it saw
            history.append((before, seen[g], (float(oms.count), oms.mean.double().cpu().numpy(), oms.std.double().cpu().numpy())))
            assert (tr._mean_P.data_ptr(), tr._std_P.data_ptr(), oms.mean.data_ptr(), oms.std.data_ptr()) == address
            assert torch.equal(tr._mean_P, oms.mean.detach().expand(4, -1)) and torch.equal(tr._std_P, oms.std.detach().expand(4, -1))
            assert not torch.equal(tr._mean_P, used)
        runs[how] = (tr.mu.clone().cpu(), history)
        env.close()
    for g in range(2):
        before, sums_c, _ = runs[False][1][g]
        n_b, mean_b, m2_b = sums_c.pooled()
        n, mean, std = _chan(before[0], before[1], before[2], float(n_b), mean_b.numpy(), m2_b.numpy())
        for how in (True, False):
            after = runs[how][1][g][2]
            assert abs(after[0] - n) <= 1e-6 * n
            np.testing.assert_allclose(after[1], mean, rtol=1e-6, atol=0)
            np.testing.assert_allclose(after[2], std, rtol=1e-6, atol=0)
        assert _equal([runs[True][1][g][1].slab], [sums_c.slab])
    assert _equal([runs[True][0]], [runs[False][0]])
