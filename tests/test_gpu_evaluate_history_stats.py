"""The observation sums of observation-history policies on the GPU (pds_evaluate_policies_history_stats of
include/pds_history_stats.h, the stats form of evaluate_hist_kernel, csrc/pds_evaluate_hist.h; evaluation.evaluate_population(...,
history_fused=True, obs_stats=True, history_stats_fused=True)): the launch of tests/test_gpu_evaluate_history.py that also sums the
histories its actors read -- a slab [tiles, 4, 2, W], W = 64, 96, 128 or 192 -- bit for bit what the composed path sums with one torch
op per difference, product and sum and adds in the kernel's tree order; the sums are the sums of their own terms (the derived bound of
tests/test_gpu_evaluate_stats.py) and within the bars of tests/test_gpu_evaluate_forms_reference.py of the independent float64
reference (tests/flight_oracle.py); the refusals leave the env alone; the trainer's running statistics follow.

Throughout, unless a test says otherwise: P = 2, 256 envs (two tiles per policy), max_episode_steps = 30 and the seeded 0.1 randn
actors of test_gpu_evaluate_history._pop_for, which fall mid-flight: tiles stop at different steps and some rows reach the cut."""
import ctypes as C

import numpy as np
import pytest
import torch

import evaluate_oracle as eo
import flight_oracle as fo
from test_gpu_evaluate_forms_reference import BAR_UNITS, _agree, _fly, _margin
from test_gpu_evaluate_forms_variants import HISTORY_FLIGHTS, LIMIT, MAX_STEPS, E as SWEEP_E, _population as _variant_population
from test_gpu_evaluate_history import CIRCLE, HOVER, LEAN, TAKEOFF, _equal, _pop_for, _snapshot, _unchanged
from test_gpu_evaluate_stats import _check_against_float64

pytestmark = pytest.mark.gpu
P, N, STEPS = 2, 256, 30
NOT_BUILT = ()  # the slab widths README names as left to the composed path: none (no stats code object spills a VGPR at any width)

# name -> (env id, env kwargs, H, network inputs, input tiles HN): one case per slab width and padding shape
CASES = {
    "hover_h3": (HOVER, {}, 3, 51, 4),                                                   # padded
    "hover_h4": (HOVER, {}, 4, 68, 6),                                                   # padded
    "hover_h7": (HOVER, {}, 7, 119, 8),                                                  # odd width, padded
    "circle_lean_h8": (CIRCLE, LEAN, 8, 160, 12),                                        # padded
    "takeoff_h8": (TAKEOFF, {}, 8, 192, 12),                                             # full, no padding
    "hover_attrate_h4": (HOVER, dict(control_mode="AttitudeRate"), 4, 68, 6),            # the PID units
}
STATS_ON = dict(fused=True, history_fused=True, obs_stats=True, history_stats_fused=True)


def _make(case, n=N, seed=3, **extra):
    import phoenix_drone_simulation_amd as pds
    env_id, kw, H, d_in, _ = CASES[case]
    env = pds.make(env_id, num_envs=n, seed=seed, max_episode_steps=STEPS, observation_history_size=H, **dict(kw, **extra))
    assert env.obs_dim == d_in
    return env


def _pop(env, with_statistics, P=P):
    """_pop_for's actors; with_statistics: a mean and a std per policy that differ between the policies, std away from 0"""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    pop = _pop_for(env, P)
    if not with_statistics:
        return pop
    g = torch.Generator().manual_seed(40 + env.obs_dim)
    mean, std = 0.1 * torch.randn(P, env.obs_dim, generator=g), 0.5 + torch.rand(P, env.obs_dim, generator=g)
    assert not torch.equal(mean[0], mean[1]) and not torch.equal(std[0], std[1])
    return PolicyPopulation.from_flat(pop.theta, pop.d_in, pop.hidden_sizes, pop.activation, mean, std, 1e-5)


def _flat(out):
    return [out[0], out[1], out[2], out[3].raw, out[4].slab]


def _bits_differ(a, b):
    return [int((x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)).sum()) if x.shape == y.shape else (x.shape, y.shape)
            for x, y in zip(a, b)]


def _built(env):
    from phoenix_drone_simulation_amd.evaluation import fused_history_stats_evaluation_built
    return fused_history_stats_evaluation_built(env)


@pytest.mark.parametrize("with_statistics", [True, False], ids=["per_policy_mean_std", "no_statistics"])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_equals_composed_bit_for_bit(case, with_statistics):
    """return, length, cost, the raw metrics and the WHOLE slab of the stats launch == the composed path's, on the bits; the first
    four == the history kernel's metrics launch; the slab is slab_features(H half) wide and zero from column H half on"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population, slab_features
    _, _, H, d_in, hn = CASES[case]
    envs = [_make(case) for _ in range(3)]
    W = slab_features(d_in)
    assert W == 16 * hn
    if not _built(envs[0]):
        assert W in NOT_BUILT, (case, W)
        pytest.skip(f"the stats form is not built for {W} columns")
    pop = _pop(envs[0], with_statistics)
    fused = evaluate_population(envs[0], pop, metrics=True, **STATS_ON)
    composed = evaluate_population(envs[1], pop, fused=False, metrics=True, obs_stats=True)
    plain = evaluate_population(envs[2], pop, fused=True, history_fused=True, metrics=True)
    assert envs[0].sync_tick() == envs[1].sync_tick() == envs[2].sync_tick()
    for e in envs:
        e.close()
    length, sums = fused[1], fused[4]
    early, cut = int((length < STEPS).sum()), int((length == STEPS).sum())
    print(f"{case} statistics={with_statistics}: {early} episodes ended before step {STEPS}, {cut} were cut there; "
          f"{float(sums.count.sum()):.0f} histories summed")
    assert tuple(sums.slab.shape) == (N // 64, 4, 2, W) and sums.slab.dtype == torch.float32 and not sums.slab.is_cuda
    assert _equal(_flat(fused), _flat(composed)), (case, _bits_differ(_flat(fused), _flat(composed)))
    assert _equal(_flat(fused)[:4], [plain[0], plain[1], plain[2], plain[3].raw])
    assert not bool(sums.slab[..., d_in:].any())
    assert bool(sums.slab[:, :, 1, :d_in].any()) and torch.equal(sums.count, length.double().sum(dim=1))
    assert early + cut == N and float(length.min()) >= 1
    if CASES[case][0] == TAKEOFF:
        assert cut == N  # (no termination on this task)
    elif "control_mode" not in CASES[case][1]:  # (under AttitudeRate these actors stay up for the 30 steps: every episode is cut)
        assert early >= 1, (early, cut)  # episodes that end mid-flight: their rows stop adding while the tile flies on


def test_the_sweep_has_104_flights():
    assert len(HISTORY_FLIGHTS) == 104 and len({f[0] for f in HISTORY_FLIGHTS}) == 104


@pytest.mark.parametrize("fid,env_id,kw,H,width", HISTORY_FLIGHTS, ids=[f[0] for f in HISTORY_FLIGHTS])
def test_every_history_configuration_sums_what_the_composed_path_sums(fid, env_id, kw, H, width):
    """every code object of the stats form once: all 26 configurations at one H per input width class, P = 3, E = 64, metrics=True,
    the one-launch path equal to the composed path on the bits.  Skipped only at a width the support query answers 0 for -- and
    that only where README names the width"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import evaluate_population, slab_features
    P3 = 3
    make = lambda: pds.make(env_id, num_envs=P3 * SWEEP_E, seed=17, max_episode_steps=LIMIT, observation_history_size=H, **kw)
    env_f, env_c = make(), make()
    assert env_f.obs_dim <= width == slab_features(env_f.obs_dim)
    if not _built(env_f):
        env_f.close(); env_c.close()
        assert width in NOT_BUILT, (fid, width)
        pytest.skip(f"the stats form is not built for {width} columns")
    pop = _variant_population(env_f, P3, seed=H)
    fused = evaluate_population(env_f, pop, max_steps=MAX_STEPS, metrics=True, **STATS_ON)
    composed = evaluate_population(env_c, pop, fused=False, max_steps=MAX_STEPS, metrics=True, obs_stats=True)
    assert _equal(_flat(fused), _flat(composed)), (fid, _bits_differ(_flat(fused), _flat(composed)))
    assert tuple(fused[4].slab.shape) == (P3 * SWEEP_E // 64, 4, 2, width)
    length = fused[1]
    assert float(length.min()) >= 1 and float(length.max()) <= LIMIT and int((length == LIMIT).sum()) >= 1
    assert env_f.sync_tick() == env_c.sync_tick() == 1 + MAX_STEPS
    env_f.close(); env_c.close()


@pytest.mark.parametrize("with_statistics", [True, False], ids=["per_policy_mean_std", "no_statistics"])
@pytest.mark.parametrize("case", ["hover_h4", "circle_lean_h8", "takeoff_h8"])
def test_the_sums_are_the_sums_of_their_own_terms(case, with_statistics):
    """the composed path under evaluation._OBS_STATS_LOG: every entry of the FUSED slab within (T + 6) u sum |terms| of the float64
    sum of its own terms (tests/test_gpu_evaluate_stats.py _check_against_float64: the bound of a recursive float32 sum of at most
    T terms per lane, four tree levels, the roundings of d and d d); count == length.sum(1); M2 >= 0 wherever a policy has
    observations; and slot H - 2 of a history holds at step s what slot H - 1 held at step s - 1: without statistics d is the
    observation itself, so the logged terms of slot H - 2 over the steps 1 .. L - 1 are those of slot H - 1 over 0 .. L - 2, one by
    one, and so are their sums"""
    from phoenix_drone_simulation_amd import evaluation
    _, _, H, d_in, _ = CASES[case]
    env_f, env_c = _make(case), _make(case)
    if not _built(env_f):
        assert evaluation.slab_features(d_in) in NOT_BUILT
        pytest.skip("the stats form is not built for this width")
    pop = _pop(env_f, with_statistics)
    fused = evaluation.evaluate_population(env_f, pop, **STATS_ON)
    log = []
    evaluation._OBS_STATS_LOG = log
    try:
        composed = evaluation.evaluate_population(env_c, pop, fused=False, obs_stats=True)
    finally:
        evaluation._OBS_STATS_LOG = None
    env_f.close(); env_c.close()
    d = torch.stack([x for x, _ in log]).numpy()   # [T, N, D] float64
    on = torch.stack([a for _, a in log]).numpy()  # [T, N] bool
    sums, length = fused[3], fused[1]
    assert _equal([sums.slab], [composed[3].slab]) and d.shape == (STEPS, N, d_in)
    L = length.reshape(-1).numpy().astype(np.int64)
    assert np.array_equal(on.sum(axis=0), L)  # alive in front of step s <=> s < length
    worst = _check_against_float64(sums.slab, d, on, d_in, STEPS)
    print(f"{case} statistics={with_statistics}: largest error / bound {worst:.4f}")
    assert torch.equal(sums.count, length.double().sum(dim=1))
    n, mean, m2 = sums.moments()
    assert bool((n > 0).all()) and bool((m2 >= 0).all()) and bool(torch.isfinite(mean).all())
    assert bool((sums.pooled()[2] >= 0).all())
    if not with_statistics and H >= 2:
        half = d_in // H
        older, newest = d[:, :, (H - 2) * half:(H - 1) * half], d[:, :, (H - 1) * half:]
        later = on[1:]  # the steps 1 .. L - 1 of every env
        assert later.any()
        assert np.array_equal(older[1:][later], newest[:-1][later])
        s_older = np.where(later[:, :, None], older[1:], 0.0).sum(axis=0)
        s_newest = np.where(later[:, :, None], newest[:-1], 0.0).sum(axis=0)
        assert np.array_equal(s_older, s_newest) and np.abs(s_older).max() > 0


# ---- the independent float64 reference: tests/flight_oracle.py --------------------------------------------------------------------
_ORACLE = {
    "hover_default_h4": lambda: fo.history_case("hover_default_h4"),  # 68 inputs, a per-policy standardisation
    "circle_lean_h8": lambda: fo.HistoryCase("circle_lean_h8", eo.CIRCLE, dict(eo.LEAN), 8, (32, 48), "relu", 40, True, rows_seed=2, bias_lo=-1.4,
                                             bias_hi=1.4),  # 160 inputs
}
_oracle_case = eo._table(_ORACLE)


def check_history_stats(case, path, sums, length):
    """check_stats of tests/test_gpu_evaluate_forms_reference.py for a slab of slab_features(H half) columns (its own asks for 64):
    every 16-env part of the slab within BAR_UNITS = 4 units of the float64 sum of the reference's per-env sums over the same
    envs -- the reference's sums are obs_sums_of over the restacked history (flight_oracle.fly(..., history=H)), the unit
    flight_oracle.units_of's; parts with an env whose length disagrees are left out and counted; count = the sum of the lengths"""
    from phoenix_drone_simulation_amd.evaluation import slab_features
    f64, units = fo.flight(case, "f64"), fo.units_of(case)
    agree, _ = _agree(case, path, length)
    D, n = case.shape[0], case.N
    assert f64["history"] == case.history and f64["sum_d"].shape == (case.P, case.E, D)
    slab = sums.slab.numpy().astype(np.float64)
    assert slab.shape == (n // 64, 4, 2, slab_features(D)) and not slab[..., D:].any()
    whole = agree.reshape(-1, 16).all(axis=1)
    left_out = int((~whole).sum())
    assert left_out <= eo.length_cap(n)
    for j, name in ((0, "sum_d"), (1, "sum_d2")):
        want = fo.part_sums(f64[name].reshape(n, D))
        err = float(np.abs(slab[:, :, j, :D].reshape(n // 16, D) - want)[whole].max())
        _margin(case, path, f"history_stats.part_{name}", units["part_" + name], err, left_out)
    assert np.array_equal(sums.count.numpy(), length.numpy().astype(np.float64).sum(axis=1))


@pytest.mark.parametrize("name", list(_ORACLE))
def test_the_sums_against_the_float64_reference(name):
    """Hover at its defaults H = 4 (68 inputs, 96 columns) and lean Circle H = 8 (160 inputs, 192 columns), P = 8, E = 128: return,
    length and cost by the rule of tests/test_gpu_evaluate_reference.py check(), the slab by check_history_stats.  No bar is set
    from the device's output.  The MARGIN lines: profiles/evaluate_history_stats_parity_margins.txt keeps a run."""
    from test_gpu_evaluate_reference import check
    case = _oracle_case(name)
    out = _fly(case, True, history_fused=True, obs_stats=True, history_stats_fused=True)
    assert len(out) == 4
    check(case, out[:3], "fused_history.stats")
    check_history_stats(case, "fused_history", out[3], out[1])
    assert BAR_UNITS == 4.0


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def _abi_stats(env, pop, obs, history, T, slab, raw=None, out=None):
    """pds_evaluate_policies_history_stats through ctypes; slab: a tensor, an address or None -> (rc, ret, len, cost)"""
    n = env.num_envs
    out = out or [torch.zeros(n, device=env.device) for _ in range(3)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t)
    with torch.cuda.device(env.device):
        rc = env.lib.pds_evaluate_policies_history_stats(env._handle, history, pop.P, n // pop.P, C.byref(pop.mlp(0)), p(pop.theta),
                                                         p(pop.mean), p(pop.std), pop.eps, T, p(obs), p(out[0]), p(out[1]), p(out[2]),
                                                         p(raw), p(slab), env._stream())
    return rc, out[0], out[1], out[2]


def test_abi_refusals_leave_the_handle_as_it_was():
    """PDS_EINVAL for a NULL d_obs_sums and one misaligned by 4 bytes; PDS_EUNSUPPORTED for a ground-effect env and for TakeOff
    H = 9 (216 inputs), where the support query answers 0; nothing moves and nothing is written; a call that is not refused
    leaves an env that asks for a reset"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    T = 10
    for env, H in ((pds.make(HOVER, num_envs=128, seed=3, observation_history_size=4, use_ground_effect=True), 4),
                   (pds.make(TAKEOFF, num_envs=128, seed=3, observation_history_size=9), 9)):
        obs, _ = env.reset()
        pop = _pop_for(env).to(env.device)
        slab, raw = torch.zeros(2 * 4 * 2 * 192, device=env.device), torch.zeros(128, 8, device=env.device)
        snap = _snapshot(env)
        assert env.lib.pds_evaluate_history_stats_supported(env._handle, H) == 0 and not _built(env)
        assert _abi_stats(env, pop, obs, H, T, slab, raw)[0] == native.EUNSUPPORTED, H
        assert len(env.lib.pds_last_error(env._handle)) > 0
        _unchanged(env, snap)
        assert float(slab.abs().max()) == 0.0 and float(raw.abs().max()) == 0.0
        env.step(torch.zeros(128, 4, device=env.device))  # still a reset handle
        env.close()

    env = pds.make(HOVER, num_envs=128, seed=3, max_episode_steps=T, observation_history_size=4)
    if not _built(env):
        env.close()
        assert 96 in NOT_BUILT
        pytest.skip("the stats form is not built for 96 columns")
    assert env.lib.pds_evaluate_history_stats_supported(env._handle, 4) == 1 and env.lib.pds_evaluate_history_stats_supported(env._handle, 12) == 0
    obs, _ = env.reset()
    pop = _pop_for(env).to(env.device)
    slab, raw = torch.zeros(2 * 4 * 2 * 96 + 4, device=env.device), torch.zeros(128, 8, device=env.device)
    out = [torch.zeros(128, device=env.device) for _ in range(3)]
    snap = _snapshot(env)
    assert slab.data_ptr() % 16 == 0
    for name, arg in (("null", None), ("misaligned", slab.data_ptr() + 4)):
        assert _abi_stats(env, pop, obs, 4, T, arg, raw, out)[0] == native.EINVAL and b"d_obs_sums" in env.lib.pds_last_error(env._handle), name
        _unchanged(env, snap)
    assert _abi_stats(env, pop, obs, 3, T, slab, raw, out)[0] == native.EINVAL  # (a check of the sibling entry point: the actors read 4 halves)
    assert _abi_stats(env, pop, obs, 12, T, slab, raw, out)[0] == native.EUNSUPPORTED  # 12 x 17 = 204 inputs
    _unchanged(env, snap)
    for buf in (slab, raw, *out):
        assert float(buf.abs().max()) == 0.0  # nothing was written
    zero = torch.zeros(128, 4, device=env.device)
    env.step(zero)  # still a reset handle
    obs, _ = env.reset()
    assert _abi_stats(env, pop, obs, 4, T, slab, None, out)[0] == native.OK  # without metrics
    torch.cuda.synchronize()
    assert float(out[1].min()) >= 1 and float(raw.abs().max()) == 0.0
    assert float(slab[:2 * 4 * 2 * 96].abs().max()) > 0 and float(slab[2 * 4 * 2 * 96:].abs().max()) == 0.0  # nothing behind the end
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(zero)
    env.reset()
    env.step(zero)
    env.close()


def test_history_2_equals_the_standard_stats_launch():
    """pds_evaluate_policies_history_stats(history = 2) on Hover at its defaults == pds_evaluate_policies_stats: return, length,
    cost, metrics and the [tiles, 4, 2, 64] slab, on the bits, on envs of the same seed"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    envs = [pds.make(HOVER, num_envs=N, seed=6, max_episode_steps=STEPS) for _ in range(2)]
    assert envs[0].obs_dim == 34
    pop = _pop(envs[0], True)
    standard = evaluate_population(envs[0], pop, fused=True, metrics=True, obs_stats=True)
    obs, _ = envs[1].reset()
    dev = envs[1].device
    slab, raw = torch.zeros(N // 64, 4, 2, 64, device=dev), torch.zeros(N, 8, device=dev)
    rc, ret, length, cost = _abi_stats(envs[1], pop.to(dev), obs.contiguous(), 2, STEPS, slab, raw)
    assert rc == native.OK, envs[1].lib.pds_last_error(envs[1]._handle)
    mine = [x.cpu().reshape(P, N // P) for x in (ret, length, cost)] + [raw.cpu().reshape(P, N // P, 8), slab.cpu()]
    assert _equal(mine, _flat(standard)), _bits_differ(mine, _flat(standard))
    assert int((mine[1] < STEPS).sum()) >= 1 and bool(mine[4].any())
    assert envs[0].sync_tick() == envs[1].sync_tick()
    for e in envs:
        e.close()


def test_es_running_statistics_with_the_history_stats_launch():
    """ESTrainer(obs_stats="online", history_fused=True) on lean Hover with H = 4, 64 policies x 64 episodes, two generations: with
    history_stats_fused=True -- every generation one launch -- the running statistics (mean, std, count) and the centre are those
    of history_stats_fused=False, the composed path, on the bits"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import es
    seen = []
    for hsf in (True, False):
        env = pds.make(HOVER, num_envs=64 * 64, seed=21, max_episode_steps=STEPS, observation_history_size=4, **LEAN)
        if hsf and not _built(env):
            env.close()
            assert 96 in NOT_BUILT
            pytest.skip("the stats form is not built for 96 columns")
        tr = es.ESTrainer(env, 64, seed=4, eval_every=0, obs_stats="online", history_fused=True, history_stats_fused=hsf)
        mu0, count0 = tr.mu.clone(), float(tr.ac.obs_oms.count)
        for _ in range(2):
            tr.learn_one_generation()
        assert not torch.equal(tr.mu, mu0) and float(tr.ac.obs_oms.count) > count0
        zero = torch.zeros(64 * 64, 4, device=env.device)
        if hsf:  # the launch ran: the handle asks for a reset
            with pytest.raises(ValueError, match="before pds_reset"):
                env.step(zero)
        else:
            env.step(zero)
        oms = tr.ac.obs_oms
        seen.append([x.detach().cpu().clone().reshape(-1) for x in (tr.mu, oms.mean, oms.std, oms.count)])
        env.close()
    assert _equal(seen[0], seen[1]), _bits_differ(seen[0], seen[1])
