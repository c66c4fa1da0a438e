"""The population evaluation of observation-history policies on the GPU (include/pds.h pds_evaluate_policies_history,
csrc/pds_evaluate_hist.h; evaluation.evaluate_population(..., history_fused=True)): P policies x E episodes in one launch, bit for
bit what the composed path -- per step one pds_mlp_forward per policy + pds_step + pds_history_advance + the accumulator updates
of evaluation.evaluate -- gives.  Every equality is on the bits; the oracle is evaluate_population(fused=False)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
HOVER, CIRCLE, TAKEOFF = "DroneHoverSimpleEnv-v0", "DroneCircleSimpleEnv-v0", "DroneTakeOffSimpleEnv-v0"
LEAN = dict(observation_noise=0, domain_randomization=0.0, motor_thrust_noise=0.0)

# name -> (env id, env kwargs, H, network inputs, hidden sizes, activation, per-policy mean / std, max_episode_steps).
# The smallest shapes that reach each path of the kernel: an odd half with scalar moves (Hover: 17 with observation noise, 21
# without), H x half no multiple of 4 (b), no shift at all (c), b128 moves (Circle 20, TakeOff 24), the PID modes (d, e), every
# input width the kernels are instantiated for (4, 6, 8, 12 tiles) with the 96 and 192 boundaries (g, h).
# max_episode_steps is set so that a case holds BOTH endings -- episodes that end before the limit and episodes the limit cuts --
# from one run of the composed path over 200 steps with the P = 1 population of this file, 128 episodes.  Medians of its episode
# lengths [shortest .. longest]: a 16 [3 .. 61], b 15 [4 .. 41], c 10 [3 .. 24], d 11 [7 .. 23], e 15 [12 .. 200: a quarter of the
# episodes flies on to the end], i 34 [22 .. 45]; the three policies of a P = 3 population have medians within 5 steps of these.  The
# limit is that median.  TakeOff has no termination (envs/takeoff.py): every episode is cut by the limit, 40 as in
# tests/test_gpu_evaluate.py -- far longer flights of random actors overflow there, and a NaN return carries whatever sign its last
# operation left, in pds_evaluate_policies as here.
CASES = {
    "a_hover_h4": (HOVER, {}, 4, 68, (32, 48), "relu", True, 16),
    "b_hover_h3": (HOVER, {}, 3, 51, (64, 64), "tanh", False, 15),
    "c_hover_lean_h1": (HOVER, LEAN, 1, 21, (32, 48), "tanh", True, 10),
    "d_circle_attrate_h3": (CIRCLE, dict(control_mode="AttitudeRate", aggregate_phy_steps=4), 3, 60, (64, 64), "relu", False, 11),
    "e_hover_lean_attitude_motor_h6": (HOVER, dict(control_mode="Attitude", use_motor_dynamics=True, **LEAN), 6, 126, (64, 64), "tanh", True, 15),
    "f_takeoff_h2": (TAKEOFF, {}, 2, 48, (32, 48), "tanh", False, 40),
    "g_takeoff_h4": (TAKEOFF, {}, 4, 96, (64, 64), "relu", True, 40),
    "h_takeoff_h8": (TAKEOFF, {}, 8, 192, (32, 48), "tanh", False, 40),
    "i_circle_lean_motor_h8": (CIRCLE, dict(use_motor_dynamics=True, **LEAN), 8, 160, (32, 48), "relu", True, 34),
}


def _population(case, P, seed=0):
    """P seeded random actors for `case` (torch's nn.Linear initialisation) whose output biases are spread from "falls at once"
    to "climbs"; where the case says so, a per-policy random mean / std, std bounded away from 0"""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    _, _, _, d_in, (h1, h2), act, stats, _ = CASES[case]
    g = torch.Generator().manual_seed(2000 + seed)
    n = h1 * d_in + h1 + h2 * h1 + h2 + 4 * h2 + 4
    theta = torch.empty(P, n)
    for p in range(P):
        k = 0
        for fan_in, count in ((d_in, h1 * d_in), (d_in, h1), (h1, h2 * h1), (h1, h2), (h2, 4 * h2), (h2, 4)):
            theta[p, k:k + count] = (torch.rand(count, generator=g) * 2 - 1) / fan_in ** 0.5
            k += count
        theta[p, -4:] += -0.6 + 1.2 * p / max(P - 1, 1) if P > 1 else -0.3
    mean = std = None
    if stats:
        mean = 0.1 * torch.randn(P, d_in, generator=g)
        std = 0.5 + torch.rand(P, d_in, generator=g)
    return PolicyPopulation.from_flat(theta, d_in, (h1, h2), act, mean, std, 1e-5)


def _make(case, n, seed=11, max_episode_steps=None, **extra):
    import phoenix_drone_simulation_amd as pds
    env_id, kwargs, H, d_in, _, _, _, limit = CASES[case]
    kw = dict(kwargs)
    kw.update(extra)
    env = pds.make(env_id, num_envs=n, seed=seed, max_episode_steps=max_episode_steps or limit, observation_history_size=H, **kw)
    assert env.obs_dim == d_in
    return env


def _abi_call(env, pop, obs, history, T, metrics=True, P=None, E=None, shape=None, mean="pop", std="pop", out=None, raw=None, params="pop"):
    """pds_evaluate_policies_history through ctypes -> (rc, ret, len, cost, raw), the tensors on the device"""
    n = env.num_envs
    P = pop.P if P is None else P
    E = n // pop.P if E is None else E
    out = out or [torch.zeros(n, device=env.device) for _ in range(3)]
    if raw is None and metrics:
        raw = torch.zeros(n, 8, device=env.device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t)
    mean = pop.mean if isinstance(mean, str) else mean
    std = pop.std if isinstance(std, str) else std
    params = pop.theta if isinstance(params, str) else params
    with torch.cuda.device(env.device):
        rc = env.lib.pds_evaluate_policies_history(env._handle, history, P, E, C.byref(shape or pop.mlp(0)), p(params), p(mean), p(std),
                                                   pop.eps, T, p(obs), p(out[0]), p(out[1]), p(out[2]), p(raw), env._stream())
    return rc, out[0], out[1], out[2], raw


def _fused(env, pop, metrics=False, max_steps=None):
    """the one-launch path -> evaluate_population's tuple with the raw metrics [P, E, 8] in place of the FlightMetrics.  At H = 2
    the keyword of evaluate_population changes nothing (the env flies pds_evaluate_policies), so the history kernel is called
    through the ABI there."""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    from phoenix_drone_simulation_amd import native
    if env.observation_history_size != 2:
        out = evaluate_population(env, pop, fused=True, history_fused=True, metrics=metrics, max_steps=max_steps)
        return out[:3] + ((out[3].raw,) if metrics else ())
    P, E = pop.P, env.num_envs // pop.P
    obs, _ = env.reset()
    rc, ret, length, cost, raw = _abi_call(env, pop.to(env.device), obs, 2, max_steps or env._max_episode_steps, metrics=metrics)
    assert rc == native.OK, env.lib.pds_last_error(env._handle)
    out = tuple(x.cpu().reshape(P, E) for x in (ret, length, cost))
    return out + ((raw.cpu().reshape(P, E, 8),) if metrics else ())


def _composed(env, pop, metrics=False, max_steps=None):
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    out = evaluate_population(env, pop, fused=False, metrics=metrics, max_steps=max_steps)
    return out[:3] + ((out[3].raw,) if metrics else ())


def _equal(a, b):
    """torch.equal on the BITS (a NaN return -- TakeOff's explicit Euler step can overflow under a random actor -- equals itself)"""
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("E", [64, 128])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_equals_composed_bit_for_bit(case, P, E):
    """returns, lengths, costs -- and at E = 128 the [P, E, 8] raw metrics, from the same launch; at E = 64 the launch runs without
    a metrics array -- of the one-launch path and of the composed path are equal on the bits, in cases that hold both endings"""
    metrics = E == 128
    pop = _population(case, P)
    env_f, env_c = _make(case, P * E), _make(case, P * E)
    limit = env_f._max_episode_steps
    fused = _fused(env_f, pop, metrics)
    composed = _composed(env_c, pop, metrics)
    length = fused[1]
    early, cut = int((length < limit).sum()), int((length == limit).sum())
    print(f"{case} P={P} E={E}: {early} episodes ended before step {limit}, {cut} were cut there; mean return {float(fused[0].mean()):.3f}")
    for x in fused[:3]:
        assert tuple(x.shape) == (P, E) and x.dtype == torch.float32 and not x.is_cuda
    assert _equal(fused, composed), [float((a - b).abs().max()) for a, b in zip(fused, composed)]
    assert early + cut == P * E and float(length.min()) >= 1
    if CASES[case][0] == TAKEOFF:
        assert early == 0 and cut == P * E  # (no termination on this task)
    else:
        assert early >= 1 and cut >= 1, (early, cut)
    assert env_f.sync_tick() == env_c.sync_tick()
    env_f.close(); env_c.close()


@pytest.mark.parametrize("case", ["a_hover_h4", "c_hover_lean_h1"])
def test_many_tiles_with_a_policy_each(case):
    """257 policies x 64 episodes: many blocks, every tile its own policy"""
    limit = 40
    pop = _population(case, 257, seed=3)
    env_f, env_c = _make(case, 257 * 64, max_episode_steps=limit), _make(case, 257 * 64, max_episode_steps=limit)
    fused, composed = _fused(env_f, pop), _composed(env_c, pop)
    early = int((fused[1] < limit).sum())
    print(f"{case} 257 x 64: {early} of {257 * 64} episodes ended before step {limit}")
    assert _equal(fused, composed)
    assert 1 <= early < 257 * 64
    env_f.close(); env_c.close()


@pytest.mark.parametrize("case", ["a_hover_h4", "d_circle_attrate_h3"])
def test_a_policy_s_rows_do_not_depend_on_the_population(case):
    """rows of policy p in a population run == a P = 1 run of that policy in an env with the same seed and env_id_base = p E"""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    P, E = 5, 128
    pop = _population(case, P, seed=7)
    env = _make(case, P * E, seed=21)
    whole = _fused(env, pop, True)
    env.close()
    for p in (0, 2, 4):
        one = PolicyPopulation.from_flat(pop.theta[p:p + 1], pop.d_in, pop.hidden_sizes, pop.activation,
                                         None if pop.mean is None else pop.mean[p:p + 1],
                                         None if pop.std is None else pop.std[p:p + 1], pop.eps)
        env1 = _make(case, E, seed=21, env_id_base=p * E)
        alone = _fused(env1, one, True)
        env1.close()
        assert _equal([x[p:p + 1] for x in whole], alone), (case, p)


def test_history_2_equals_the_standard_evaluation():
    """pds_evaluate_policies_history(history = 2) on Hover at its defaults == pds_evaluate_policies (return, length, cost) and ==
    pds_evaluate_policies_metrics (the metrics), on envs of the same seed"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    P, E, limit = 3, 128, 60
    g = torch.Generator().manual_seed(5)
    d_in, h = 34, 50
    n = h * d_in + h + h * h + h + 4 * h + 4
    theta = 0.1 * torch.randn(P, n, generator=g)
    theta[:, -4:] += torch.tensor([-0.6, 0.0, 0.6]).unsqueeze(1)
    pop = PolicyPopulation.from_flat(theta, d_in, (h, h), "relu", 0.1 * torch.randn(P, d_in, generator=g), 0.5 + torch.rand(P, d_in, generator=g))
    envs = [pds.make(HOVER, num_envs=P * E, seed=6, max_episode_steps=limit) for _ in range(3)]
    plain = evaluate_population(envs[0], pop, fused=True)
    with_metrics = evaluate_population(envs[1], pop, fused=True, metrics=True)
    obs, _ = envs[2].reset()
    rc, ret, length, cost, raw = _abi_call(envs[2], pop.to(envs[2].device), obs, 2, limit)
    assert rc == native.OK, envs[2].lib.pds_last_error(envs[2]._handle)
    mine = tuple(x.cpu().reshape(P, E) for x in (ret, length, cost))
    assert _equal(mine, plain) and _equal(mine, with_metrics[:3])
    assert _equal([raw.cpu().reshape(P, E, 8)], [with_metrics[3].raw])
    assert int((mine[1] < limit).sum()) >= 1 and int((mine[1] == limit).sum()) >= 1
    assert envs[2].sync_tick() == envs[0].sync_tick()
    for e in envs:
        e.close()


def _snapshot(env):
    sd = env.state_dict()  # every get_state field + the tick (+ the history the env keeps)
    return {f: v.clone() for f, v in sd.items() if f != "tick"}, sd["tick"]


def _unchanged(env, snap):
    before, tick = snap
    assert env.tick == tick and env.sync_tick() == tick
    for f, v in before.items():
        now = env._hist if f == "observation_history" else env.get_state(f)
        assert torch.equal(now, v), f


def _pop_for(env, P=2):
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    torch.manual_seed(0)
    d_in = env.obs_dim
    n = 50 * d_in + 50 + 50 * 50 + 50 + 4 * 50 + 4
    return PolicyPopulation.from_flat(0.1 * torch.randn(P, n), d_in, (50, 50), "relu")


@pytest.mark.parametrize("case", ["ground_effect_h4", "takeoff_h9", "obs_stats"])
def test_refusals_leave_the_env_as_it_was_and_auto_runs_composed(case):
    """history_fused=True with fused=True raises where the launch is not built -- an env configuration outside the history
    rollout's (here the ground effect), more than 192 inputs (TakeOff H = 9: 216), obs_stats=True -- and leaves the env untouched;
    fused="auto" runs the composed path there and leaves an env that steps (at 216 inputs the composed path stops at its own
    limit, pds_mlp_forward's 192 inputs, as it does without the keyword)"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import evaluate_population, fused_history_evaluation_built
    if case == "takeoff_h9":
        env = pds.make(TAKEOFF, num_envs=128, seed=3, max_episode_steps=30, observation_history_size=9)
        assert env.obs_dim == 216
    else:
        # (obs_stats: H = 3, 51 inputs -- the composed path's slab of observation sums holds 64 features)
        env = pds.make(HOVER, num_envs=128, seed=3, max_episode_steps=30, observation_history_size=4 if case == "ground_effect_h4" else 3,
                       use_ground_effect=case == "ground_effect_h4")
    extra = dict(obs_stats=True) if case == "obs_stats" else {}
    assert fused_history_evaluation_built(env) == (case == "obs_stats")
    env.reset()
    pop = _pop_for(env)
    snap = _snapshot(env)
    with pytest.raises(NotImplementedError):
        evaluate_population(env, pop, fused=True, history_fused=True, **extra)
    _unchanged(env, snap)
    if case == "takeoff_h9":  # the composed path has a limit of its own: pds_mlp_forward reads at most 192 inputs, with or without the keyword
        with pytest.raises(RuntimeError, match="pds_mlp_forward"):
            evaluate_population(env, pop, fused="auto", history_fused=True)
    else:
        out = evaluate_population(env, pop, fused="auto", history_fused=True, **extra)  # the composed path
        for x in out[:3]:
            assert tuple(x.shape) == (2, 64)
        assert float(out[1].min()) >= 1 and float(out[1].max()) <= 30
    env.step(torch.zeros(128, 4, device=env.device))  # the composed path leaves an env that steps
    env.close()


def test_the_latency_ring_has_no_history_env_and_no_history_kernel():
    """use_latency with observation_history_size != 2 is refused by the env's constructor, so evaluate_population never sees such
    an env; the ABI answers PDS_EUNSUPPORTED for a latency handle, whichever history it is asked for"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    with pytest.raises(NotImplementedError):
        pds.make(HOVER, num_envs=128, seed=3, observation_history_size=4, use_latency=True)
    env = pds.make(HOVER, num_envs=128, seed=3, use_latency=True)
    obs, _ = env.reset()
    snap = _snapshot(env)
    pop = _pop_for(env).to(env.device)
    assert env.lib.pds_evaluate_history_supported(env._handle, 2) == 0 and env.lib.pds_evaluate_history_supported(env._handle, 4) == 0
    assert _abi_call(env, pop, obs, 2, 10)[0] == native.EUNSUPPORTED
    _unchanged(env, snap)
    env.step(torch.zeros(128, 4, device=env.device))
    env.close()


def test_abi_refusals_leave_the_handle_as_it_was():
    """PDS_EUNSUPPORTED for a handle without auto_reset; PDS_EINVAL for the argument errors; nothing moves"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.evaluation import fused_history_evaluation_built
    env = pds.make(HOVER, num_envs=128, seed=3, auto_reset=False, observation_history_size=4)
    obs, _ = env.reset()
    pop = _pop_for(env).to(env.device)
    snap = _snapshot(env)
    assert not fused_history_evaluation_built(env)
    assert _abi_call(env, pop, obs, 4, 10)[0] == native.EUNSUPPORTED and b"auto_reset" in env.lib.pds_last_error(env._handle)
    _unchanged(env, snap)
    env.close()

    env = pds.make(HOVER, num_envs=128, seed=3, observation_history_size=4)
    assert fused_history_evaluation_built(env) and env.lib.pds_evaluate_history_supported(env._handle, 12) == 0
    obs = torch.zeros(128, env.obs_dim, device=env.device)
    assert _abi_call(env, pop, obs, 4, 10)[0] == native.EINVAL and b"before pds_reset" in env.lib.pds_last_error(env._handle)  # never reset
    obs, _ = env.reset()
    snap = _snapshot(env)
    ones = torch.ones(2, env.obs_dim, device=env.device)
    wide = pop.mlp(0); wide.h1 = 65
    raw = torch.zeros(128 * 8 + 4, device=env.device)
    calls = dict(d_in=lambda: _abi_call(env, pop, obs, 3, 10),  # the actors read 4 halves, the call says 3
                 h1=lambda: _abi_call(env, pop, obs, 4, 10, shape=wide),
                 p_x_e=lambda: _abi_call(env, pop, obs, 4, 10, P=3),
                 e32=lambda: _abi_call(env, pop, obs, 4, 10, P=4, E=32),
                 steps=lambda: _abi_call(env, pop, obs, 4, 0),
                 null=lambda: _abi_call(env, pop, obs, 4, 10, params=None),
                 mean_alone=lambda: _abi_call(env, pop, obs, 4, 10, mean=ones, std=None),
                 metrics_align=lambda: _abi_call(env, pop, obs, 4, 10, raw=raw.data_ptr() + 4),
                 history0=lambda: _abi_call(env, pop, obs, 0, 10))
    for name, call in calls.items():
        assert call()[0] == native.EINVAL and len(env.lib.pds_last_error(env._handle)) > 0, name
    assert _abi_call(env, pop, obs, 12, 10)[0] == native.EUNSUPPORTED  # 12 x 17 = 204 inputs
    _unchanged(env, snap)
    env.step(torch.zeros(128, 4, device=env.device))  # still a reset handle
    env.close()


def test_the_handle_afterwards():
    """not reset: step and step_k raise until reset(); the tick moved by reset + max_steps, whichever step the tiles stopped at; a
    fresh env of the same seed reproduces the bits; after reset() the env's history and a per-step flight are what an env that was
    never evaluated gives at the same tick.  A lean env (case e, H = 6): with the reference's noise the OU thrust state, the gyro
    bias and its low-pass carry over a reset by design, so there a reset behind tiles that stopped at steps of their own is not a
    function of the tick alone -- under pds_evaluate_policies as here."""
    case = "e_hover_lean_attitude_motor_h6"
    pop = _population(case, 2)
    limit, n = 30, 2 * 128
    env = _make(case, n, seed=9, max_episode_steps=limit)
    tick0 = env.tick
    first = _fused(env, pop, True)
    assert int((first[1] < limit).sum()) >= 1  # (episodes that ended early)
    assert env.tick == tick0 + 1 + limit and env.sync_tick() == env.tick
    zero = torch.zeros(n, 4, device=env.device)
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(zero)
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step_k(zero.unsqueeze(0))
    env2 = _make(case, n, seed=9, max_episode_steps=limit)
    assert _equal(_fused(env2, pop, True), first)
    env2.close()
    # a never-evaluated env at the same tick: the same reset, the same flight
    env3 = _make(case, n, seed=9, max_episode_steps=limit)
    env3.load_state_dict({"tick": env.tick})
    o1, _ = env.reset()
    o3, _ = env3.reset()
    assert torch.equal(o1, o3) and tuple(o1.shape) == (n, 126)
    g = torch.Generator().manual_seed(4)
    for k in range(6):
        a = (0.3 * torch.rand(n, 4, generator=g) - 0.25).to(env.device)
        out1, out3 = env.step(a), env3.step(a)
        for x, y in zip(out1[:4], out3[:4]):
            assert torch.equal(x, y), k
    env.close(); env3.close()


def test_es_generation_with_the_history_launch():
    """one generation of ESTrainer(history_fused=True) on lean Hover with H = 4 gives the centre of history_fused=False on the bits"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import es
    centres = []
    for hf in (True, False):
        env = pds.make(HOVER, num_envs=8 * 64, seed=21, max_episode_steps=30, observation_history_size=4, **LEAN)
        tr = es.ESTrainer(env, 8, seed=4, eval_every=10, history_fused=hf)
        mu0 = tr.mu.clone()
        tr.learn_one_generation()
        assert not torch.equal(tr.mu, mu0)
        zero = torch.zeros(512, 4, device=env.device)
        if hf:  # the launch ran: the handle asks for a reset
            with pytest.raises(ValueError, match="before pds_reset"):
                env.step(zero)
        else:
            env.step(zero)
        centres.append(tr.mu.detach().cpu().clone())
        env.close()
    assert torch.equal(centres[0].view(torch.int32), centres[1].view(torch.int32))
