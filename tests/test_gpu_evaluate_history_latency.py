"""The one-launch evaluation of observation-history policies on the latency ring (include/pds_history_latency_evaluate.h; the
V::LAT forms of evaluate_hist_kernel, csrc/pds_evaluate_hist.h; evaluation.evaluate_population(..., history_fused=True,
history_latency_fused=True)): bit for bit the composed path -- per step pds_mlp_forward + pds_step + pds_history_advance_latency, what
such an env ran before -- in the metrics, the record and the stats form over all 24 configurations x 4 input widths; the rule shows
in the record; the float64 reference flight of tests/flight_latency_oracle.py at the 4-unit bar of
tests/test_gpu_evaluate_forms_reference.py; the refusals leave the handle alone; the ES trainer follows.

The sweep: P = 2, E = 64 (one tile per policy), max_steps = 12 with an episode limit of 5 .. 9 -- the TimeLimit ends first episodes
inside the launch, envs fly on into a second episode, policy 0 crashes within a few steps and its tile stops early -- on rings of
1, 2 and 3 rows with 1 and 2 sub-steps."""
import ctypes as C

import numpy as np
import pytest
import torch

import flight_latency_oracle as flo
import variant_cases as vc
from test_gpu_evaluate_history import _equal, _pop_for
from test_gpu_evaluate_variants import _population

pytestmark = pytest.mark.gpu
HOVER, CIRCLE, TAKEOFF = vc.HOVER, vc.CIRCLE, vc.TAKEOFF
MAX_STEPS, E = 12, 64
ON = dict(fused=True, history_fused=True, history_latency_fused=True)
# (latency in seconds -> ring rows B at the env's 0.01 s time step, aggregate_phy_steps): the rule fires at every j, at the even j,
# at j = 2, 3, 5, 6 (B = 3, agg = 2: some but not all j <= H), every third j, and twice per step's worth of rows
RINGS = ((0.015, 1), (0.025, 1), (0.035, 2), (0.035, 1), (0.025, 2))


def _half(env_id, kw):
    return {HOVER: 17 if kw.get("observation_noise", 1) > 0 else 21, CIRCLE: 20}[env_id]


def _configurations():
    """{Hover, Circle} x {PWM, AttitudeRate, Attitude} x {with, without motor dynamics} x {noise off, reference default}: 24"""
    out = []
    for (task, env_id) in vc.TASKS[:2]:
        for ctrl in vc.CTRL:
            for motor in (False, True):
                for full in (False, True):
                    f = (motor, full, full, full, False, ctrl, False, False)
                    out.append((vc._name(task, *f) + "-ring", env_id, vc.kwargs_of(*f)))
    return out


CONFIGURATIONS = _configurations()
FLIGHTS = [(f"{name}-h{H}-w{width}", env_id, dict(kw, latency=RINGS[(i + k) % 5][0], aggregate_phy_steps=RINGS[(i + k) % 5][1]), H, width, 5 + (i + k) % 5)
           for i, (name, env_id, kw) in enumerate(CONFIGURATIONS) for k, (H, width) in enumerate(vc.history_sizes(_half(env_id, kw)))]


def _make(env_id, kw, H, n, limit, seed=17, **extra):
    import phoenix_drone_simulation_amd as pds
    return pds.make(env_id, num_envs=n, seed=seed, max_episode_steps=limit, observation_history_size=H, use_latency=True, history_latency=True,
                    **dict(kw, **extra))


def _snapshot(env):
    """the tick, the state fields, the ring where the handle has one, the history the env keeps and its step counts"""
    fields = ("pos", "vel", "rpy", "omega", "last_action", "step_count") + (("action_buffer", "action_idx") if env.latency_steps >= 1 else ())
    snap = {f: env.get_state(f).clone() for f in fields}
    snap["_hist"] = env._hist.clone()
    if env.history_latency:
        snap["_hist_steps"] = env._hist_steps.clone()
    return snap, env.tick


def _unchanged(env, snap):
    before, tick = snap
    assert env.tick == tick and env.sync_tick() == tick
    for f, v in before.items():
        assert torch.equal(getattr(env, f) if f.startswith("_") else env.get_state(f), v), f


def _bits_differ(a, b):
    return [int((x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)).sum()) if x.shape == y.shape else (x.shape, y.shape)
            for x, y in zip(a, b)]


def _record_tensors(out):
    ret, length, cost, fm, fl = out
    return [ret, length, cost, fm.raw, fl.state, fl.action, fl.observation, fl.length, fl.last_action0]


def _stats_tensors(out):
    ret, length, cost, fm, sums = out
    return [ret, length, cost, fm.raw, sums.slab, sums.count.float()]


def _metrics_tensors(out):
    return [out[0], out[1], out[2], out[3].raw]


def _three_forms(make, pop, max_steps, R):
    """the metrics, the record and the stats flight, each on a fresh pair of envs: the launch against the composed path -> the
    fused results"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    got = {}
    for form, kw, tensors in (("metrics", dict(metrics=True), _metrics_tensors), ("record", dict(metrics=True, record=R), _record_tensors),
                              ("stats", dict(metrics=True, obs_stats=True, history_stats_fused=True), _stats_tensors)):
        env_f, env_c = make(), make()
        fused = evaluate_population(env_f, pop, max_steps=max_steps, **ON, **kw)
        composed = evaluate_population(env_c, pop, fused=False, max_steps=max_steps, **{k: v for k, v in kw.items() if k != "history_stats_fused"})
        assert _equal(tensors(fused), tensors(composed)), (form, _bits_differ(tensors(fused), tensors(composed)))
        assert env_f.sync_tick() == env_c.sync_tick() == 1 + max_steps
        with pytest.raises(ValueError, match="before pds_reset"):  # the launch ran: the env asks for a reset
            env_f.step(torch.zeros(env_f.num_envs, 4, device=env_f.device))
        env_f.close(); env_c.close()
        got[form] = fused
    assert _equal(_metrics_tensors(got["metrics"]), _metrics_tensors(got["record"])) and _equal(_metrics_tensors(got["metrics"]), _metrics_tensors(got["stats"]))
    return got


def test_the_sweep_has_96_flights_on_every_ring():
    assert len(CONFIGURATIONS) == 24 and len(FLIGHTS) == 96 and len({f[0] for f in FLIGHTS}) == 96
    assert {(f[2]["latency"], f[2]["aggregate_phy_steps"]) for f in FLIGHTS} == set(RINGS) and {f[5] for f in FLIGHTS} == {5, 6, 7, 8, 9}
    assert {f[4] for f in FLIGHTS} == {64, 96, 128, 192}


@pytest.mark.parametrize("fid,env_id,kw,H,width,limit", FLIGHTS, ids=[f[0] for f in FLIGHTS])
def test_every_configuration_and_width_equals_the_composed_path_in_every_form(fid, env_id, kw, H, width, limit):
    """every code object of the three forms once: returns, lengths, costs, the eight metrics, the record (state, action,
    observation [P, R, T, H half], last_action0) and the stats slab, on the bits"""
    from phoenix_drone_simulation_amd.evaluation import (fused_history_evaluation_built, fused_history_latency_evaluation_built,
                                                         fused_history_latency_stats_evaluation_built, slab_features)
    make = lambda: _make(env_id, kw, H, 2 * E, limit)  # noqa: E731
    env = make()
    assert env.obs_dim <= width == slab_features(env.obs_dim) and env.latency_steps >= 1
    assert fused_history_latency_evaluation_built(env) and fused_history_latency_stats_evaluation_built(env)
    assert not fused_history_evaluation_built(env) and env.lib.pds_evaluate_history_supported(env._handle, H) == 0  # (as before)
    pop = _population(env, 2, seed=H)
    env.close()
    got = _three_forms(make, pop, MAX_STEPS, E)
    length, fl, sums = got["metrics"][1], got["record"][4], got["stats"][4]
    assert float(length.min()) >= 1 and float(length.max()) <= limit
    assert tuple(fl.observation.shape) == (2, E, MAX_STEPS, env.obs_dim) and tuple(sums.slab.shape) == (2, 4, 2, width)
    assert int((length == limit).sum()) >= 1  # the TimeLimit ended first episodes inside the launch
    if env_id == HOVER and kw.get("control_mode", "PWM") == "PWM" and not kw.get("use_motor_dynamics"):
        assert float(length[0].max()) < limit, length[0]  # policy 0 crashes: its tile stops before its neighbour


@pytest.mark.parametrize("env_id,kw,H,ring", [(HOVER, {}, 4, RINGS[2]), (CIRCLE, vc.kwargs_of(True, False, False, False, False, "AttitudeRate", False, False), 8, RINGS[0]),
                                              (HOVER, vc.kwargs_of(False, False, False, False, False, "Attitude", False, False), 1, RINGS[1])],
                         ids=["hover_full_h4_b3_agg2", "circle_lean_attrate_motor_h8_b1", "hover_lean_attitude_h1_b2"])
def test_a_tile_that_does_not_record(env_id, kw, H, ring):
    """P = 1, E = 128 with R = 64: the second tile of the policy flies and sums, and records nothing; H = 1 among the cases"""
    kw = dict(kw, latency=ring[0], aggregate_phy_steps=ring[1])
    make = lambda: _make(env_id, kw, H, 128, 7)  # noqa: E731
    env = make()
    pop = _population(env, 1, seed=3)
    env.close()
    got = _three_forms(make, pop, MAX_STEPS, 64)
    assert tuple(got["record"][4].state.shape) == (1, 64, MAX_STEPS, 12) and tuple(got["record"][1].shape) == (1, 128)


def test_random_actors_at_the_default_limit_terminate_at_different_steps():
    """Hover at its defaults, H = 4, ring of 2 rows, max_episode_steps at its default of 500 and max_steps = 40: the 0.1 randn actors
    fall mid-flight, envs terminate at steps of their own, none is cut"""
    make = lambda: _make(HOVER, dict(latency=0.025), 4, 2 * E, 500)  # noqa: E731
    env = make()
    pop = _pop_for(env)
    env.close()
    got = _three_forms(make, pop, 40, E)
    length = got["metrics"][1]
    assert len(torch.unique(length)) >= 4 and float(length.min()) < 40, torch.unique(length)


def test_above_256_tiles():
    """257 policies x 64 episodes: 257 blocks, a policy per tile, lean Hover H = 3 on a ring of 3 rows with 2 sub-steps"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    kw = dict(vc.kwargs_of(False, False, False, False, False, "PWM", False, False), latency=0.035, aggregate_phy_steps=2)
    env_f, env_c = (_make(HOVER, kw, 3, 257 * E, 6) for _ in range(2))
    pop = _population(env_f, 257, seed=5)
    fused = evaluate_population(env_f, pop, max_steps=8, metrics=True, **ON)
    composed = evaluate_population(env_c, pop, fused=False, max_steps=8, metrics=True)
    env_f.close(); env_c.close()
    assert _equal(_metrics_tensors(fused), _metrics_tensors(composed)), _bits_differ(_metrics_tensors(fused), _metrics_tensors(composed))
    assert tuple(fused[0].shape) == (257, E) and float(fused[1][256].min()) >= 1


def test_the_rule_shows_in_the_record():
    """the composed path with the rule switched off (the env advances its histories with pds_history_advance, as an env without
    history_latency would) records other observations than the launch, first in the action columns the rule rewrites
    -- a kernel that dropped the rule could not pass the sweep.  Lean Hover, H = 4, ring of 3 rows with 2 sub-steps."""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    kw = dict(vc.kwargs_of(False, False, False, False, False, "PWM", False, False), latency=0.035, aggregate_phy_steps=2)
    H, limit = 4, 9
    env_f, env_c, env_off = (_make(HOVER, kw, H, 2 * E, limit) for _ in range(3))
    pop = _population(env_f, 2, seed=H)
    env_off.history_latency = False  # (the per-step history launch without the rule)
    kwargs = dict(max_steps=MAX_STEPS, metrics=True, record=E)
    fused = evaluate_population(env_f, pop, **ON, **kwargs)
    composed = evaluate_population(env_c, pop, fused=False, **kwargs)
    off = evaluate_population(env_off, pop, fused=False, **kwargs)
    for e in (env_f, env_c, env_off):
        e.close()
    assert _equal(_record_tensors(fused), _record_tensors(composed))
    a, b = fused[4].observation[1], off[4].observation[1]  # policy 1 (policy 0 crashes within a few steps)
    half = a.shape[-1] // H
    both = min(int(fused[1][1].min()), int(off[1][1].min()))  # steps every env of the policy recorded on both paths
    assert both >= 3
    differ = (a != b)[:, :both].reshape(E, both, H, half)
    assert not bool(differ[:, 0].any()) and not bool(differ[:, 1].any())  # j = 1 does not fire on this ring; o(0) is the reset's
    # behind step j = 2 the slots 0 .. H - 2 show a(1): o(2) differs there, in action columns alone (from o(3) on the flights part:
    # the actors read other histories)
    assert bool(differ[:, 2, :H - 1, half - 4:].any()) and not bool(differ[:, 2, :, :half - 4].any()) and not bool(differ[:, 2, H - 1].any())
    act = fused[4].action
    assert torch.equal(a.reshape(E, MAX_STEPS, H, half)[:, 2, 0, half - 4:], act[1, :, 1])  # the RAW action
    assert float(act.abs().max()) > 1.0


# ---- the float64 reference flight: tests/flight_latency_oracle.py ------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "composed"])
@pytest.mark.parametrize("name", flo.CASES)
def test_against_the_float64_reference_flight(name, path):
    """return, length and cost by the rule of tests/test_gpu_evaluate_reference.py check(); the metrics, the record and the slab by
    check_metrics / check_record / check_history_stats: 4 units, a unit being the float32 reference's own distance from the
    float64 one per quantity group.  No env is left out (tests/test_history_latency_evaluate_cpu.py: the flights agree on every
    length).  The MARGIN lines: profiles/evaluate_history_latency_parity_margins.txt keeps a run."""
    from test_gpu_evaluate_forms_reference import BAR_UNITS, _fly, check_metrics, check_record
    from test_gpu_evaluate_history_stats import check_history_stats
    from test_gpu_evaluate_reference import check
    case = flo.case(name)
    flo.units_of(case)  # (both flights into the case's memo, where flight_oracle's checks look them up)
    fused = path == "fused"
    on = dict(history_fused=True, history_latency_fused=True) if fused else {}
    tag = f"{path}_history_latency"
    R = case.E
    out = _fly(case, fused, metrics=True, record=R, **on)
    check(case, out[:3], f"{tag}.record")
    check_metrics(case, tag, "record", out[3], out[1])
    check_record(case, tag, out[4], R, True)
    out = _fly(case, fused, metrics=True, obs_stats=True, **(dict(on, history_stats_fused=True) if fused else {}))
    check(case, out[:3], f"{tag}.stats")
    check_metrics(case, tag, "stats", out[3], out[1])
    check_history_stats(case, tag, out[4], out[1])
    assert BAR_UNITS == 4.0


# ---- refusals and predicates --------------------------------------------------------------------------------------------------------
def _abi(env, name, pop, obs, H, T, *trail):
    n = env.num_envs
    out = [torch.zeros(n, device=env.device) for _ in range(3)]
    p = lambda t: None if t is None else (C.c_void_p(t.data_ptr()) if isinstance(t, torch.Tensor) else t)  # noqa: E731
    with torch.cuda.device(env.device):
        rc = getattr(env.lib, name)(env._handle, H, pop.P, n // pop.P, C.byref(pop.mlp(0)), p(pop.theta), p(pop.mean), p(pop.std), pop.eps, T,
                                    p(obs), p(out[0]), p(out[1]), p(out[2]), *[p(t) for t in trail], env._stream())
    return rc, out


REFUSED = {
    "takeoff": (TAKEOFF, dict(use_latency=True, history_latency=True)),
    "kalman_hold": (HOVER, dict(use_latency=True, history_latency=True, observation_frequency=50)),
    "ground_effect": (HOVER, dict(use_latency=True, history_latency=True, use_ground_effect=True)),
    "partial_noise": (HOVER, dict(use_latency=True, history_latency=True, motor_thrust_noise=0)),
    "no_ring": (HOVER, dict()),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refusals_leave_the_handle_untouched(case):
    """TakeOff on the ring, the Kalman hold, the ground effect, partial noise, a handle without the ring: the two questions answer
    0, the three calls PDS_EUNSUPPORTED with nothing moved and nothing written, fused=True raises with the env untouched, "auto"
    flies (the composed path on the ring; the non-latency launch without it) -- and the old predicates answer as before"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.evaluation import (evaluate_population, fused_history_evaluation_built,
                                                         fused_history_latency_evaluation_built, fused_history_latency_stats_evaluation_built)
    env_id, kw = REFUSED[case]
    H, n, T = 4, 128, 6
    env = pds.make(env_id, num_envs=n, seed=3, max_episode_steps=5, observation_history_size=H, **kw)
    obs, _ = env.reset()
    pop = _pop_for(env).to(env.device)
    assert env.lib.pds_evaluate_history_latency_supported(env._handle, H) == 0 and env.lib.pds_evaluate_history_latency_stats_supported(env._handle, H) == 0
    assert not fused_history_latency_evaluation_built(env) and not fused_history_latency_stats_evaluation_built(env)
    assert fused_history_evaluation_built(env) == (case == "no_ring") == (env.lib.pds_evaluate_history_supported(env._handle, H) == 1)
    snap = _snapshot(env)
    raw, slab = torch.zeros(n, 8, device=env.device), torch.zeros(2 * 4 * 2 * 192, device=env.device)
    flight, obs_rec = torch.zeros(T, 4, n, 4, device=env.device), torch.zeros(T, n, env.obs_dim, device=env.device)
    for name, trail in (("pds_evaluate_policies_history_latency", (raw,)),
                        ("pds_evaluate_policies_history_latency_record", (raw, C.c_int64(64), flight, obs_rec)),
                        ("pds_evaluate_policies_history_latency_stats", (raw, slab))):
        rc, out = _abi(env, name, pop, obs.contiguous(), H, T, *trail)
        assert rc == native.EUNSUPPORTED and len(env.lib.pds_last_error(env._handle)) > 0, name
        _unchanged(env, snap)
        for buf in (raw, slab, flight, obs_rec, *out):
            assert float(buf.abs().max()) == 0.0, name
    if case != "no_ring":
        with pytest.raises(NotImplementedError):
            evaluate_population(env, pop, max_steps=T, **ON)
        _unchanged(env, snap)
    out = evaluate_population(env, pop, fused="auto", history_fused=True, history_latency_fused=True, max_steps=T)
    assert float(out[1].min()) >= 1
    if case == "no_ring":  # the non-latency launch flew: the env asks for a reset
        with pytest.raises(ValueError, match="before pds_reset"):
            env.step(torch.zeros(n, 4, device=env.device))
    else:
        env.step(torch.zeros(n, 4, device=env.device))  # the composed path leaves an env that steps
    env.close()


def test_more_than_192_inputs_and_a_frozen_env():
    """H = 12 on Hover (204 inputs): the questions answer 0.  set_latency one step into an episode freezes views: the predicates
    answer False until the next full reset, fused=True raises, "auto" runs the composed path"""
    from phoenix_drone_simulation_amd.evaluation import (evaluate_population, fused_history_latency_evaluation_built,
                                                         fused_history_latency_stats_evaluation_built)
    env = _make(HOVER, dict(latency=0.025), 4, 128, 6)
    assert env.lib.pds_evaluate_history_latency_supported(env._handle, 4) == 1 and env.lib.pds_evaluate_history_latency_supported(env._handle, 12) == 0
    assert env.lib.pds_evaluate_history_latency_stats_supported(env._handle, 11) == 1 and env.lib.pds_evaluate_history_latency_supported(env._handle, 0) == 0
    env.reset()
    assert fused_history_latency_evaluation_built(env) and fused_history_latency_stats_evaluation_built(env)
    env.step(torch.zeros(128, 4, device=env.device))
    env.set_latency(0.035)
    assert env._hist_frozen and not fused_history_latency_evaluation_built(env) and not fused_history_latency_stats_evaluation_built(env)
    assert env.lib.pds_evaluate_history_latency_supported(env._handle, 4) == 1  # (the handle itself is on the ring: the env knows better)
    pop = _pop_for(env)
    with pytest.raises(NotImplementedError):
        evaluate_population(env, pop, max_steps=6, **ON)
    out = evaluate_population(env, pop, fused="auto", history_fused=True, history_latency_fused=True, max_steps=6)
    assert float(out[1].min()) >= 1
    env.step(torch.zeros(128, 4, device=env.device))  # the composed path
    env.reset()
    assert fused_history_latency_evaluation_built(env)  # a full reset: the views start again
    env.close()


def test_without_the_keyword_the_env_flies_as_before():
    """history_fused=True alone on a ring env: fused=True raises with the env untouched, "auto" runs the composed path"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    env = _make(HOVER, dict(latency=0.025), 4, 128, 6)
    env.reset()
    pop = _pop_for(env)
    snap = _snapshot(env)
    with pytest.raises(NotImplementedError):
        evaluate_population(env, pop, fused=True, history_fused=True, max_steps=6)
    _unchanged(env, snap)
    evaluate_population(env, pop, fused="auto", history_fused=True, max_steps=6)
    env.step(torch.zeros(128, 4, device=env.device))
    env.close()


# ---- the trainer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("online", [False, True], ids=["frozen_statistics", "online_statistics"])
def test_es_generations_with_the_latency_launch(online):
    """ESTrainer(history_fused=True, history_latency_fused=True) on Circle under AttitudeRate, H = 4, on the ring, 8 policies x 64
    episodes: two generations leave the centre bit for bit where the composed evaluation leaves it; with obs_stats="online" and
    history_stats_fused=True the running statistics as well"""
    from phoenix_drone_simulation_amd import es
    seen = []
    for fused in (True, False):
        env = _make(CIRCLE, dict(control_mode="AttitudeRate", latency=0.025), 4, 8 * 64, 30, seed=21)
        tr = es.ESTrainer(env, 8, seed=4, eval_every=0, obs_stats="online" if online else "warmup", history_fused=fused,
                          history_stats_fused=fused and online, history_latency_fused=fused)
        mu0 = tr.mu.clone()
        for _ in range(2):
            tr.learn_one_generation()
        assert not torch.equal(tr.mu, mu0)
        zero = torch.zeros(8 * 64, 4, device=env.device)
        if fused:  # the launch ran: the handle asks for a reset
            with pytest.raises(ValueError, match="before pds_reset"):
                env.step(zero)
        else:
            env.step(zero)
        oms = tr.ac.obs_oms
        seen.append([x.detach().cpu().clone().reshape(-1) for x in (tr.mu, oms.mean, oms.std, oms.count)])
        env.close()
    assert _equal(seen[0], seen[1]), _bits_differ(seen[0], seen[1])
