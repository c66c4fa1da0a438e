"""The flight-quality metrics of the one-launch policy evaluation on the GPU (include/pds.h pds_evaluate_policies_metrics,
csrc/pds_evaluate.h, the flight metrics; evaluation.evaluate_population(..., metrics=True)): bit for bit what the composed path sums with
separate torch ops, equal in arithmetic to evaluation.metrics_from_arrays in float64 (held to an independent reference in
tests/test_gpu_evaluate_forms_reference.py), hand-checkable on policies
with zero weights, and without any effect on return, length and cost."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_evaluate import CONFIGS, TAKEOFF, HOVER, _equal, _make, _population, _snapshot, _unchanged

pytestmark = pytest.mark.gpu
EM = dict(roll_sq=0, pitch_sq=1, rate_sq=2, action_rate_sq=3, tilt_max=4, saturated_steps=5, roll_rate_crossings=6,
          pitch_rate_crossings=7)


def _same(config, a, b):
    """all four outputs: on the bits; TakeOff (its explicit Euler step overflows under a random actor): on the values, with the
    NaNs in the same places"""
    xs, ys = list(a[:3]) + [a[3].raw], list(b[:3]) + [b[3].raw]
    if CONFIGS[config][0] == TAKEOFF:
        return all(x.shape == y.shape and torch.equal(torch.isnan(x), torch.isnan(y)) and
                   torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)) for x, y in zip(xs, ys))
    return _equal(xs, ys)


@pytest.mark.parametrize("P,E", [(1, 64), (3, 192)])
@pytest.mark.parametrize("config", ["hover_default", "hover_lean", "circle_attrate", "hover_latency", "hover_hold", "takeoff"])
def test_fused_equals_composed_bit_for_bit(config, P, E):
    from phoenix_drone_simulation_amd.evaluation import FlightMetrics, evaluate_population
    pop = _population(config, P)
    env_f, env_c = _make(config, P * E), _make(config, P * E)
    limit = env_f._max_episode_steps
    fused = evaluate_population(env_f, pop, fused=True, metrics=True)
    composed = evaluate_population(env_c, pop, fused=False, metrics=True)
    assert len(fused) == 4 and isinstance(fused[3], FlightMetrics)
    fm, length = fused[3], fused[1]
    assert tuple(fm.raw.shape) == (P, E, 8) and fm.raw.dtype == torch.float32 and not fm.raw.is_cuda
    assert torch.equal(fm.length, length) and fm.step_seconds == pytest.approx(env_f.cfg.time_step * env_f.cfg.aggregate_phy_steps)
    early, cut = int((length < limit).sum()), int((length == limit).sum())
    diff = [float((x - y).abs().nan_to_num().max()) for x, y in zip(list(fused[:3]) + [fm.raw], list(composed[:3]) + [composed[3].raw])]
    print(f"{config} P={P} E={E}: {early} early, {cut} cut; max |fused - composed| of ret, len, cost, metrics: {diff}; "
          f"table {({k: [round(float(x), 4) for x in v] for k, v in fm.table().items()})}")
    assert _same(config, fused, composed), diff
    assert early + cut == P * E
    if CONFIGS[config][0] == TAKEOFF:
        assert early == 0
    else:
        assert early >= 1 and cut >= 1, (early, cut)
        # the counters are bounded by the episode: saturated steps <= L, crossings <= L - 1
        assert bool((fm.saturated_steps <= length).all()) and bool((fm.roll_rate_crossings <= length - 1).all())
        assert bool((fm.raw[..., :5] >= 0).all())
    env_f.close(); env_c.close()


@pytest.mark.parametrize("config", ["hover_default", "circle_attrate", "takeoff"])
def test_metrics_do_not_move_return_length_and_cost(config):
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E = 3, 64
    pop = _population(config, P)
    env_m, env_p = _make(config, P * E), _make(config, P * E)
    with_m = evaluate_population(env_m, pop, fused=True, metrics=True)
    plain = evaluate_population(env_p, pop, fused=True)
    assert len(plain) == 3 and _equal(with_m[:3], plain)
    assert env_m.sync_tick() == env_p.sync_tick()
    env_m.close(); env_p.close()


def test_more_tiles_than_cus_and_an_odd_tile_count():
    """257 x 64: above 256 tiles (two teams per block where the metrics form fits), an odd tile count, a half-filled last block"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    for config, limit in (("hover_lean", 40), ("hover_default", 40)):
        pop = _population(config, 257, seed=3)
        env_f, env_c = _make(config, 257 * 64, max_episode_steps=limit), _make(config, 257 * 64, max_episode_steps=limit)
        fused = evaluate_population(env_f, pop, fused=True, metrics=True)
        composed = evaluate_population(env_c, pop, fused=False, metrics=True)
        early = int((fused[1] < limit).sum())
        print(f"{config} 257 x 64: {early} of {257 * 64} episodes ended before step {limit}")
        assert _same(config, fused, composed)
        assert 1 <= early < 257 * 64
        env_f.close(); env_c.close()


def test_one_step_counts_the_reset_state_only():
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E = 2, 64
    pop = _population("hover_default", P)
    env, twin = _make("hover_default", P * E), _make("hover_default", P * E)
    ret, length, cost, fm = evaluate_population(env, pop, fused=True, metrics=True, max_steps=1)
    twin.reset()
    rpy, omega = twin.get_state("rpy").cpu(), twin.get_state("omega").cpu()
    assert torch.equal(length, torch.ones(P, E))
    assert torch.equal(fm.roll_rate_crossings, torch.zeros(P, E)) and torch.equal(fm.pitch_rate_crossings, torch.zeros(P, E))
    assert torch.equal(fm.roll_sq.reshape(-1), rpy[:, 0] * rpy[:, 0]) and float(fm.roll_sq.max()) > 0
    assert torch.equal(fm.pitch_sq.reshape(-1), rpy[:, 1] * rpy[:, 1])
    assert torch.equal(fm.rate_sq.reshape(-1), (omega[:, 0] * omega[:, 0] + omega[:, 1] * omega[:, 1]) + omega[:, 2] * omega[:, 2])
    assert torch.equal(fm.tilt_max.reshape(-1), torch.maximum(rpy[:, 0].abs(), rpy[:, 1].abs()))
    env.close(); twin.close()


def test_hand_checkable_policies_with_zero_weights():
    """hover_lean, zero weights: the action is the output bias at every step.  b3 = 2: every step saturates, and the action
    changes once, from the reset's action to 2.  b3 = 0.5: no step saturates."""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    d_in, h1, h2, E = 42, 32, 48, 64
    n = h1 * d_in + h1 + h2 * h1 + h2 + 4 * h2 + 4
    theta = torch.zeros(2, n)
    theta[0, -4:], theta[1, -4:] = 2.0, 0.5
    pop = PolicyPopulation.from_flat(theta, d_in, (h1, h2), "tanh")
    for fused in (True, False):
        env, twin = _make("hover_lean", 2 * E), _make("hover_lean", 2 * E)
        ret, length, cost, fm = evaluate_population(env, pop, fused=fused, metrics=True)
        twin.reset()
        u0 = twin.get_state("last_action").cpu()
        assert torch.equal(fm.saturated_steps[0], length[0]) and float(length.min()) >= 1
        assert torch.equal(fm.saturated_steps[1], torch.zeros(E))
        for p, b in ((0, 2.0), (1, 0.5)):
            d = torch.full((E, 4), b) - u0[p * E:(p + 1) * E]
            dd = d * d
            assert torch.equal(fm.action_rate_sq[p], ((dd[:, 0] + dd[:, 1]) + dd[:, 2]) + dd[:, 3]), (fused, p)
        env.close(); twin.close()


class _Recorder:
    """records what the composed path reads in front of every step and the actions it hands over"""

    def __init__(self, env):
        self.env, self.fields, self.actions = env, {"rpy": [], "omega": [], "last_action": []}, []
        self._get, self._step = env.get_state, env.step
        env.get_state, env.step = self.get_state, self.step

    def get_state(self, name):
        v = self._get(name)
        if name in self.fields:
            self.fields[name].append(v.cpu().numpy().copy())
        return v

    def step(self, act):
        self.actions.append(act.cpu().numpy().copy())
        return self._step(act)


@pytest.mark.parametrize("config", ["hover_default", "circle_attrate"])
def test_against_the_definitions_in_float64(config):
    """every env's first episode, as the composed path saw it, through metrics_from_arrays.  Counters and tilt_max: equal.  Sums:
    within (T + 4) 2^-24 relative -- T sequential float32 additions of non-negative terms plus the roundings inside one term,
    both sides reading the same float32 states.  This checks the ARITHMETIC of the sums only: the states, `u` and the "state
    before step s" convention are the composed path's own (env.get_state), and metrics_from_arrays is the project's.  The
    independent check -- the true state and last_action read off the float64 CPU oracle, the definitions restated from
    include/pds.h -- is tests/test_gpu_evaluate_forms_reference.py (tests/flight_oracle.py)."""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population, metrics_from_arrays
    P, E = 2, 64
    pop = _population(config, P)
    env = _make(config, P * E)
    T = env._max_episode_steps
    rec = _Recorder(env)
    ret, length, cost, fm = evaluate_population(env, pop, fused=False, metrics=True)
    assert len(rec.actions) == T and all(len(v) == T for v in rec.fields.values())
    rpy, omega, last = (np.stack(rec.fields[k]) for k in ("rpy", "omega", "last_action"))  # [T, N, width]
    acts = np.stack(rec.actions)
    raw, L = fm.raw.reshape(P * E, 8).numpy().astype(np.float64), length.reshape(-1).numpy().astype(int)
    rtol = (T + 4) * 2.0 ** -24
    worst = 0.0
    for n in range(P * E):
        want = metrics_from_arrays(rpy[:L[n], n], omega[:L[n], n], acts[:L[n], n], last[0, n])
        for j in (4, 5, 6, 7):
            assert raw[n, j] == want[j], (n, j, raw[n, j], want[j])
        for j in (0, 1, 2, 3):
            err = abs(raw[n, j] - want[j]) / want[j] if want[j] > 0 else abs(raw[n, j])
            worst = max(worst, err)
            assert err <= rtol, (n, j, raw[n, j], want[j], err, rtol)
    print(f"{config}: worst relative error of the four sums {worst:.3e} (bound {rtol:.3e}), lengths {L.min()}..{L.max()}")
    assert L.min() < T  # the case holds episodes that froze before the limit
    env.close()


def test_abi_refusals_leave_the_handle_as_it_was():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    pop = _population("hover_default", 2)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(e, obs, out, metrics_ptr, T=10):
        dpop = pop.to(e.device)
        call.keep = dpop
        return e.lib.pds_evaluate_policies_metrics(e._handle, 2, 64, C.byref(dpop.mlp(0)), p(dpop.theta), p(dpop.mean), p(dpop.std),
                                                   pop.eps, T, p(obs), p(out[0]), p(out[1]), p(out[2]), metrics_ptr, e._stream())

    env = pds.make(HOVER, num_envs=128, seed=3, auto_reset=False)
    obs, _ = env.reset()
    out = [torch.zeros(128, device=env.device) for _ in range(3)]
    raw = torch.zeros(128 * 8 + 4, device=env.device)
    snap = _snapshot(env)
    assert call(env, obs, out, p(raw)) == native.EUNSUPPORTED and b"auto_reset" in env.lib.pds_last_error(env._handle)
    _unchanged(env, snap)
    env.close()

    env = pds.make(HOVER, num_envs=128, seed=3, max_episode_steps=30)
    obs, _ = env.reset()
    snap = _snapshot(env)
    assert raw.data_ptr() % 16 == 0
    assert call(env, obs, out, None) == native.EINVAL and len(env.lib.pds_last_error(env._handle)) > 0
    _unchanged(env, snap)
    assert call(env, obs, out, C.c_void_p(raw.data_ptr() + 4)) == native.EINVAL and b"aligned" in env.lib.pds_last_error(env._handle)
    _unchanged(env, snap)
    assert call(env, obs, out, p(raw), T=0) == native.EINVAL
    _unchanged(env, snap)
    assert float(raw.abs().max()) == 0.0  # nothing was written
    env.step(torch.zeros(128, 4, device=env.device))  # still a reset handle
    obs, _ = env.reset()
    assert call(env, obs, out, p(raw), T=30) == native.OK  # the accepted call: "not reset" afterwards, like the plain entry
    torch.cuda.synchronize()
    assert float(out[1].min()) >= 1 and float(raw[:128 * 8].reshape(128, 8)[:, 2].min()) > 0
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(torch.zeros(128, 4, device=env.device))
    env.reset()
    env.step(torch.zeros(128, 4, device=env.device))  # the env steps on after a reset()
    env.close()


def test_log_dir_writes_metrics_csv(tmp_path):
    from phoenix_drone_simulation_amd.evaluation import METRIC_NAMES, evaluate_population
    pop = _population("hover_default", 2)
    env = _make("hover_default", 2 * 64, seed=2, max_episode_steps=30)
    ret, length, cost, fm = evaluate_population(env, pop, fused=True, log_dir=str(tmp_path), metrics=True)
    for p in range(2):
        lines = open(tmp_path / str(p) / "metrics.csv").read().split()
        assert lines[0] == ",".join(METRIC_NAMES) + ",length" and len(lines) == 65
        rows = np.array([[float(x) for x in l.split(",")] for l in lines[1:]])
        assert np.array_equal(rows[:, :8], fm.raw[p].numpy().astype(np.float64)) and np.array_equal(rows[:, 8], length[p].numpy())
        assert (tmp_path / str(p) / "returns.csv").exists()
    env.close()


def _trainer(**kw):
    from phoenix_drone_simulation_amd.es import ESTrainer
    env = _make("hover_default", 4 * 64, seed=6, max_episode_steps=30)
    return ESTrainer(env, 4, seed=5, eval_every=0, **kw)


def test_es_fitness_none_is_the_trainer_as_it_was():
    a, b = _trainer(), _trainer(fitness=None)
    for _ in range(2):
        ia, ib = a.learn_one_generation(), b.learn_one_generation()
        assert ia["fitness_mean"] == ib["fitness_mean"]
    assert a.generation == 2 and torch.equal(a.mu, b.mu)
    a.env.close(); b.env.close()


def test_es_penalised_return_reaches_tell(monkeypatch):
    from phoenix_drone_simulation_amd import es
    seen = {}
    real = es.evaluate_population

    def spy(*args, **kw):
        seen["kw"], seen["out"] = kw, real(*args, **kw)
        return seen["out"]

    monkeypatch.setattr(es, "evaluate_population", spy)
    t = _trainer(fitness=es.penalised_return({"action_rate_sq": 1.0}))
    tell = t.tell
    monkeypatch.setattr(t, "tell", lambda f: (seen.__setitem__("fitness", f.clone()), tell(f))[1])
    t.learn_one_generation()
    assert seen["kw"].get("metrics") is True
    ret, length, cost, fm = seen["out"]
    want = (ret - 1.0 * fm.action_rate_sq).mean(dim=1)
    assert tuple(seen["fitness"].shape) == (4,) and torch.equal(seen["fitness"], want)
    assert not torch.equal(want, ret.mean(dim=1))  # the penalty is there
    assert t.generation == 1
    t.env.close()
