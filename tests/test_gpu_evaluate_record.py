"""The recorded flights of the one-launch policy evaluation on the GPU (include/pds.h pds_evaluate_policies_record,
csrc/pds_evaluate.h, the record; evaluation.evaluate_population(..., record=R) -> evaluation.Flights): bit for bit what the composed
path reads in front of every step, zero past every episode's end, without any effect on what the evaluation returns, x(0) the
reset state, hand-checkable on policies with zero weights, and enough to re-derive the flight metrics."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_evaluate import CONFIGS, TAKEOFF, HOVER, _equal, _make, _population, _snapshot, _unchanged

pytestmark = pytest.mark.gpu
SIX = ["hover_default", "hover_lean", "circle_attrate", "hover_latency", "hover_hold", "takeoff"]
SHAPES = [(1, 64, 64), (3, 192, 64), (2, 128, 128)]  # (P, E, R): one tile; the first of three tiles per policy; every tile


def _same_values(config, xs, ys):
    """on the bits; TakeOff (its explicit Euler step overflows under a random actor): on the values, NaNs in the same places"""
    if CONFIGS[config][0] == TAKEOFF:
        return all(x.shape == y.shape and torch.equal(torch.isnan(x), torch.isnan(y)) and
                   torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)) for x, y in zip(xs, ys))
    return _equal(xs, ys)


def _fields(out):
    """everything a call with metrics=True, record=R returns, as a flat list of tensors"""
    ret, length, cost, fm, fl = out
    return [ret, length, cost, fm.raw, fl.state, fl.action, fl.observation, fl.length]


@functools.lru_cache(maxsize=None)
def _both_paths(config, P, E, R):
    """one fused and one composed run of the case (two envs of the same seed and kwargs), shared by the tests below"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    pop = _population(config, P)
    env_f, env_c = _make(config, P * E), _make(config, P * E)
    limit = env_f._max_episode_steps
    fused = evaluate_population(env_f, pop, fused=True, metrics=True, record=R)
    composed = evaluate_population(env_c, pop, fused=False, metrics=True, record=R)
    ticks = (env_f.sync_tick(), env_c.sync_tick())
    env_f.close(); env_c.close()
    return fused, composed, limit, env_f.obs_dim, ticks


@pytest.mark.parametrize("P,E,R", SHAPES)
@pytest.mark.parametrize("config", SIX)
def test_fused_equals_composed_bit_for_bit(config, P, E, R):
    from phoenix_drone_simulation_amd.evaluation import FlightMetrics, Flights
    fused, composed, limit, D, ticks = _both_paths(config, P, E, R)
    assert len(fused) == len(composed) == 5 and isinstance(fused[3], FlightMetrics) and isinstance(fused[4], Flights)
    fl, length = fused[4], fused[1]
    assert tuple(fl.state.shape) == (P, R, limit, 12) and tuple(fl.action.shape) == (P, R, limit, 4)
    assert tuple(fl.observation.shape) == (P, R, limit, D) and tuple(fl.length.shape) == (P, R)
    for x in (fl.state, fl.action, fl.observation, fl.length):
        assert x.dtype == torch.float32 and not x.is_cuda
    assert torch.equal(fl.length, length[:, :R]) and fl.step_seconds == fused[3].step_seconds
    a, b = _fields(fused), _fields(composed)
    diff = [float((x - y).abs().nan_to_num().max()) for x, y in zip(a, b)]
    rec = length[:, :R]
    early, cut = int((rec < limit).sum()), int((rec == limit).sum())
    print(f"{config} P={P} E={E} R={R}: {early} recorded episodes ended early, {cut} were cut; max |fused - composed| of ret, len, "
          f"cost, metrics, state, action, observation, length: {diff}")
    assert _same_values(config, a, b), diff
    assert ticks[0] == ticks[1]
    assert early + cut == P * R
    if CONFIGS[config][0] == TAKEOFF:
        assert early == 0
    else:
        assert early >= 1 and cut >= 1, (early, cut)
        assert bool((fl.state[:, :, 0].abs().sum(-1) > 0).all())  # every recorded column was written


@pytest.mark.parametrize("P,E,R", SHAPES)
@pytest.mark.parametrize("config", SIX)
def test_rows_past_the_end_are_zero_and_rows_before_it_finite(config, P, E, R):
    fused, composed, limit, D, _ = _both_paths(config, P, E, R)
    for out in (fused, composed):
        fl = out[4]
        past = (torch.arange(limit).view(1, 1, limit) >= fl.length.unsqueeze(-1)).unsqueeze(-1)  # [P, R, T, 1]
        for x in (fl.state, fl.action, fl.observation):
            assert bool((x.view(torch.int32)[past.expand_as(x)] == 0).all())  # +0.0, bit for bit
            if CONFIGS[config][0] != TAKEOFF:
                assert bool(torch.isfinite(x).all())
        if CONFIGS[config][0] != TAKEOFF:  # a flown row is not a zero row: the observation holds the last action and the state a height
            flown = ~past.squeeze(-1)
            assert bool((fl.observation.abs().sum(-1)[flown] > 0).all()) and bool((fl.state.abs().sum(-1)[flown] > 0).all())


@pytest.mark.parametrize("config", ["hover_default", "circle_attrate", "takeoff"])
def test_recording_moves_nothing(config):
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E = 3, 64
    pop = _population(config, P)
    envs = [_make(config, P * E) for _ in range(3)]
    with_r = evaluate_population(envs[0], pop, fused=True, metrics=True, record=64)
    plain = evaluate_population(envs[1], pop, fused=True, metrics=True)
    no_obs = evaluate_population(envs[2], pop, fused=True, record=64, record_observations=False)
    assert len(plain) == 4 and len(with_r) == 5 and len(no_obs) == 4  # (metrics=False: the metrics the record form sums are dropped)
    assert _equal(list(with_r[:3]) + [with_r[3].raw], list(plain[:3]) + [plain[3].raw])
    assert _equal(no_obs[:3], plain[:3])
    assert envs[0].sync_tick() == envs[1].sync_tick() == envs[2].sync_tick()
    assert no_obs[3].observation is None
    assert _equal([no_obs[3].state, no_obs[3].action, no_obs[3].length], [with_r[4].state, with_r[4].action, with_r[4].length])
    for e in envs:
        e.close()


@pytest.mark.parametrize("fused", [True, False])
def test_x0_is_the_reset_state(fused):
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E = 2, 64
    pop = _population("hover_default", P)
    env, twin = _make("hover_default", P * E), _make("hover_default", P * E)
    ret, length, cost, fl = evaluate_population(env, pop, fused=fused, max_steps=1, record=64)
    obs0, _ = twin.reset()
    x0 = torch.cat([twin.get_state(f) for f in ("pos", "vel", "rpy", "omega")], dim=1).cpu()
    assert tuple(fl.state.shape) == (P, 64, 1, 12) and torch.equal(length, torch.ones(P, E))
    assert torch.equal(fl.state[:, :, 0].reshape(P * E, 12), x0) and float(x0.abs().max()) > 0
    assert torch.equal(fl.observation[:, :, 0].reshape(P * E, -1), obs0.cpu())
    assert torch.equal(fl.last_action0.reshape(P * E, 4), twin.get_state("last_action").cpu())
    env.close(); twin.close()


def test_hand_checkable_policies_with_zero_weights():
    """hover_lean, zero weights: the action is the output bias at every step -- 2.0 for policy 0, 0.5 for policy 1"""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    d_in, h1, h2, E = 42, 32, 48, 64
    n = h1 * d_in + h1 + h2 * h1 + h2 + 4 * h2 + 4
    theta = torch.zeros(2, n)
    theta[0, -4:], theta[1, -4:] = 2.0, 0.5
    pop = PolicyPopulation.from_flat(theta, d_in, (h1, h2), "tanh")
    for fused in (True, False):
        env = _make("hover_lean", 2 * E)
        T = env._max_episode_steps
        ret, length, cost, fl = evaluate_population(env, pop, fused=fused, record=64)
        flown = torch.arange(T).view(1, T) < length[:, :, None].reshape(2, E, 1)  # [2, E, T]
        assert float(length.min()) >= 1
        for p, b in ((0, 2.0), (1, 0.5)):
            assert bool((fl.action[p][flown[p]] == b).all()), (fused, p)
            assert bool((fl.action[p][~flown[p]] == 0).all()), (fused, p)
        env.close()


@pytest.mark.parametrize("config", ["hover_default", "circle_attrate"])
def test_the_record_explains_the_metrics(config):
    """Flights.metrics() -- the definitions in float64 over the recorded float32 states -- against the same launch's float32
    sums.  Counters and tilt_max: equal.  Sums: within (T + 4) 2^-24 relative, the bound of test_against_the_definitions_in_float64
    (tests/test_gpu_evaluate_metrics.py): T sequential float32 additions of non-negative terms plus the roundings inside one term,
    both sides reading the same float32 states."""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E = 2, 64
    pop = _population(config, P)
    env = _make(config, P * E)
    T = env._max_episode_steps
    ret, length, cost, fm, fl = evaluate_population(env, pop, fused=True, metrics=True, record=64)
    want, raw = fl.metrics(), fm.raw.numpy().astype(np.float64)
    rtol = (T + 4) * 2.0 ** -24
    worst = 0.0
    for p in range(P):
        for e in range(E):
            for j in (4, 5, 6, 7):
                assert raw[p, e, j] == want[p, e, j], (p, e, j, raw[p, e, j], want[p, e, j])
            for j in (0, 1, 2, 3):
                err = abs(raw[p, e, j] - want[p, e, j]) / want[p, e, j] if want[p, e, j] > 0 else abs(raw[p, e, j])
                worst = max(worst, err)
                assert err <= rtol, (p, e, j, raw[p, e, j], want[p, e, j], err, rtol)
    print(f"{config}: worst relative error of the four sums {worst:.3e} (bound {rtol:.3e}), lengths {int(length.min())}..{int(length.max())}")
    assert float(length.min()) < T
    env.close()


def test_more_tiles_than_cus_and_an_odd_tile_count():
    """257 x 64: above 256 tiles (two teams per block where the record form fits), an odd tile count, a half-filled last block"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    for config, limit in (("hover_lean", 40), ("hover_default", 40)):
        pop = _population(config, 257, seed=3)
        env_f, env_c = _make(config, 257 * 64, max_episode_steps=limit), _make(config, 257 * 64, max_episode_steps=limit)
        fused = evaluate_population(env_f, pop, fused=True, metrics=True, record=64)
        composed = evaluate_population(env_c, pop, fused=False, metrics=True, record=64)
        early = int((fused[1] < limit).sum())
        print(f"{config} 257 x 64: {early} of {257 * 64} episodes ended before step {limit}")
        assert _equal(_fields(fused), _fields(composed))
        assert 1 <= early < 257 * 64
        env_f.close(); env_c.close()


def test_abi_refusals_leave_the_handle_as_it_was():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    pop = _population("hover_default", 2)
    p = lambda t: C.c_void_p(t.data_ptr())
    T = 30

    def call(e, obs, out, raw, rec, flight_ptr, obs_rec, T=T):
        dpop = pop.to(e.device)
        call.keep = dpop
        return e.lib.pds_evaluate_policies_record(e._handle, 2, 64, C.byref(dpop.mlp(0)), p(dpop.theta), p(dpop.mean), p(dpop.std),
                                                  pop.eps, T, p(obs), p(out[0]), p(out[1]), p(out[2]), p(raw) if raw is not None else None,
                                                  rec, flight_ptr, p(obs_rec) if obs_rec is not None else None, e._stream())

    def buffers(dev):
        return ([torch.zeros(128, device=dev) for _ in range(3)], torch.zeros(128 * 8, device=dev),
                torch.zeros(T * 4 * 128 * 4 + 4, device=dev), torch.zeros(T * 128 * 34, device=dev))

    env = pds.make(HOVER, num_envs=128, seed=3, auto_reset=False)
    obs, _ = env.reset()
    out, raw, flight, obs_rec = buffers(env.device)
    snap = _snapshot(env)
    assert call(env, obs, out, raw, 64, p(flight), obs_rec) == native.EUNSUPPORTED and b"auto_reset" in env.lib.pds_last_error(env._handle)
    _unchanged(env, snap)
    assert float(flight.abs().max()) == 0.0 and float(obs_rec.abs().max()) == 0.0
    env.close()

    env = pds.make(HOVER, num_envs=128, seed=3, max_episode_steps=T)
    obs, _ = env.reset()
    out, raw, flight, obs_rec = buffers(env.device)
    snap = _snapshot(env)
    assert flight.data_ptr() % 16 == 0
    refused = [call(env, obs, out, raw, 64, None, obs_rec),                               # NULL d_flight
               call(env, obs, out, raw, 64, C.c_void_p(flight.data_ptr() + 4), obs_rec),  # misaligned d_flight
               call(env, obs, out, raw, 0, p(flight), obs_rec),
               call(env, obs, out, raw, 96, p(flight), obs_rec),
               call(env, obs, out, raw, 64 + 64, p(flight), obs_rec)]                     # E + 64
    for rc in refused:
        assert rc == native.EINVAL and len(env.lib.pds_last_error(env._handle)) > 0
        _unchanged(env, snap)
    for buf in (flight, obs_rec, raw, *out):
        assert float(buf.abs().max()) == 0.0  # nothing was written
    env.step(torch.zeros(128, 4, device=env.device))  # still a reset handle
    obs, _ = env.reset()
    assert call(env, obs, out, None, 64, p(flight), None) == native.OK  # the accepted call, without metrics and observations
    torch.cuda.synchronize()
    assert float(out[1].min()) >= 1 and float(raw.abs().max()) == 0.0 and float(obs_rec.abs().max()) == 0.0
    rows = flight[:T * 4 * 128 * 4].reshape(T, 4, 128, 4)
    assert float(rows[0, 0, :, 2].min()) > 0 and float(flight[T * 4 * 128 * 4:].abs().max()) == 0.0  # z(0) of every env; nothing behind the end
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(torch.zeros(128, 4, device=env.device))
    env.reset()
    env.step(torch.zeros(128, 4, device=env.device))  # the env steps on after a reset()
    env.close()

