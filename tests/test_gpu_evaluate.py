"""The population evaluation on the GPU (include/pds.h pds_evaluate_policies, csrc/pds_evaluate.h;
phoenix_drone_simulation_amd.evaluation.evaluate_population): P policies x E episodes in one launch, bit for bit what the
composed path -- per step one pds_mlp_forward per policy + pds_step + the accumulator updates of evaluation.evaluate -- gives."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOVER, CIRCLE, TAKEOFF = "DroneHoverSimpleEnv-v0", "DroneCircleSimpleEnv-v0", "DroneTakeOffSimpleEnv-v0"

# name -> (env id, env kwargs, bundled policies flown there (tests/golden), max_episode_steps of the bitwise cases).
# max_episode_steps is set so that a case holds BOTH endings -- episodes that end before the limit (the accumulators freeze, the
# tile may stop early) and episodes the limit cuts.  TakeOff has no termination (envs/takeoff.py: `done` is never set; csrc/pds_step.h),
# so every one of its episodes is cut by the limit and the case asserts exactly that.
# Where the limits come from: the episode lengths of these populations at the full 500 steps (medians: hip_policy_early 130 on
# Hover, with the latency ring 131, hip_policy_hover_hold 100; the random actors on lean Hover 14; hip_policy_circle_default at
# exp-07's PWM setting 32, where the bundled reference policy flies on; hip_policy_circle_attrate_late falls in ~20 % of its
# episodes) -- a limit near the median of the policy a P = 1 case flies puts both endings into every case.
CONFIGS = {
    "hover_default": (HOVER, {}, ("hip_policy_early", "hip_policy_late"), 140),
    "hover_lean": (HOVER, dict(observation_noise=0, domain_randomization=0.0, motor_thrust_noise=0.0), (), 14),
    "circle_pwm_exp07": (CIRCLE, dict(aggregate_phy_steps=2, use_motor_dynamics=True),
                         ("hip_policy_circle_default", "policy_PWM_seed_00000_model", "hip_policy_circle_attrate_late"), 32),
    "circle_attrate": (CIRCLE, dict(control_mode="AttitudeRate", aggregate_phy_steps=4),
                       ("hip_policy_circle_attrate_late", "hip_policy_circle_default", "policy_PWM_seed_00000_model"), 300),
    "hover_latency": (HOVER, dict(use_latency=True, latency=0.02),
                      ("hip_policy_early", "hip_policy_late", "hip_policy_hover_latency_motor"), 140),
    "takeoff": (TAKEOFF, {}, (), 40),
    "hover_hold": (HOVER, dict(observation_frequency=50), ("hip_policy_hover_hold", "hip_policy_early", "hip_policy_late"), 110),
}
OBS_DIM = {HOVER: 34, CIRCLE: 40, TAKEOFF: 48}


def _bundled(name):
    """(flat parameter row, mean, std) of a bundled policy, through the constructor its format has"""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    from phoenix_drone_simulation_amd.policy_io import load_network_json
    from phoenix_drone_simulation_amd.ppo import ActorCritic
    if name.endswith("_model"):
        pop = PolicyPopulation.from_json_policies([load_network_json(os.path.join(GOLD, name + ".json"))])
    else:
        sd = np.load(os.path.join(GOLD, name + ".npz"))
        pop = PolicyPopulation.from_actor_critics([ActorCritic.from_reference_state_dict({k: sd[k] for k in sd.files})])
    assert (pop.hidden_sizes, pop.activation, pop.eps) == ((50, 50), "relu", 1e-5)
    return pop.theta[0], pop.mean[0], pop.std[0]


def _population(config, P, seed=0):
    """P policies for `config`: its bundled policies in turn -- the first round as they are, every further round with a seeded
    perturbation of the weights (5 % of each weight's size), so that the rows differ.  Where no bundled policy has the env's
    observation width (Hover without observation noise: 42 inputs; TakeOff: 48): seeded random actors (torch's nn.Linear
    initialisation, tanh, 32 and 48 hidden units, no standardisation) whose output biases are spread, so that some fall at once."""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    env_id, kwargs, names, _ = CONFIGS[config]
    g = torch.Generator().manual_seed(1000 + seed)
    if names:
        base = [_bundled(n) for n in names]
        rows, means, stds = [], [], []
        for p in range(P):
            th, m, s = base[p % len(base)]
            if p >= len(base):
                th = th * (1.0 + 0.05 * torch.randn(th.shape, generator=g))
            rows.append(th); means.append(m); stds.append(s)
        return PolicyPopulation.from_flat(torch.stack(rows), base[0][1].numel(), (50, 50), "relu", torch.stack(means), torch.stack(stds), 1e-5)
    d_in = 42 if env_id == HOVER else OBS_DIM[env_id]
    h1, h2 = 32, 48
    n = h1 * d_in + h1 + h2 * h1 + h2 + 4 * h2 + 4
    theta = torch.empty(P, n)
    for p in range(P):
        k = 0
        for fan_in, count in ((d_in, h1 * d_in), (d_in, h1), (h1, h2 * h1), (h1, h2), (h2, 4 * h2), (h2, 4)):
            theta[p, k:k + count] = (torch.rand(count, generator=g) * 2 - 1) / fan_in ** 0.5
            k += count
        theta[p, -4:] += -0.6 + 1.2 * p / max(P - 1, 1) if P > 1 else -0.3  # output biases: from "falls at once" to "climbs"
    return PolicyPopulation.from_flat(theta, d_in, (h1, h2), "tanh")


def _make(config, n, seed=11, max_episode_steps=None, **extra):
    import phoenix_drone_simulation_amd as pds
    env_id, kwargs, _, limit = CONFIGS[config]
    kw = dict(kwargs)
    kw.update(extra)
    return pds.make(env_id, num_envs=n, seed=seed, max_episode_steps=max_episode_steps or limit, **kw)


def _equal(a, b):
    """torch.equal on the BITS (a NaN return -- TakeOff's explicit Euler step can overflow under a random actor -- equals itself)"""
    return all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("E", [64, 192])
@pytest.mark.parametrize("P", [1, 3, 8])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_fused_equals_composed_bit_for_bit(config, P, E):
    """returns, lengths and costs of the one-launch path and of the composed path are torch.equal (two envs of the same seed and
    kwargs), in cases that hold both endings"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    pop = _population(config, P)
    env_f, env_c = _make(config, P * E), _make(config, P * E)
    limit = env_f._max_episode_steps
    fused = evaluate_population(env_f, pop, fused=True)
    composed = evaluate_population(env_c, pop, fused=False)
    length = fused[1]
    early, cut = int((length < limit).sum()), int((length == limit).sum())
    print(f"{config} P={P} E={E}: {early} episodes ended before step {limit}, {cut} were cut there; "
          f"mean return {float(fused[0].mean()):.3f}, cost {float(fused[2].mean()):.3f}")
    for x in fused:
        assert tuple(x.shape) == (P, E) and x.dtype == torch.float32 and not x.is_cuda
    assert _equal(fused, composed), [float((a - b).abs().max()) for a, b in zip(fused, composed)]
    assert early + cut == P * E and float(length.min()) >= 1
    if CONFIGS[config][0] == TAKEOFF:
        assert early == 0 and cut == P * E  # (no termination on this task: see CONFIGS; its other ending has a test of its own below)
    else:
        assert early >= 1 and cut >= 1, (early, cut)
    env_f.close(); env_c.close()


def test_more_tiles_than_cus_and_an_odd_tile_count():
    """P = 257 policies x 64 episodes: above 256 tiles the launcher may put two teams in a block, and the last block is half
    filled"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    for config, limit in (("hover_lean", 40), ("hover_default", 40)):
        pop = _population(config, 257, seed=3)
        env_f, env_c = _make(config, 257 * 64, max_episode_steps=limit), _make(config, 257 * 64, max_episode_steps=limit)
        fused = evaluate_population(env_f, pop, fused=True)
        composed = evaluate_population(env_c, pop, fused=False)
        early = int((fused[1] < limit).sum())
        print(f"{config} 257 x 64: {early} of {257 * 64} episodes ended before step {limit}")
        assert _equal(fused, composed)
        assert 1 <= early < 257 * 64
        env_f.close(); env_c.close()


@pytest.mark.parametrize("config", ["hover_default", "circle_pwm_exp07", "hover_lean"])
def test_a_policy_s_result_does_not_depend_on_the_population(config):
    """rows of policy p in a population run == a P = 1 run of that policy in an env with the same seed and env_id_base = p E"""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    P, E = 5, 128
    pop = _population(config, P, seed=7)
    env = _make(config, P * E, seed=21)
    whole = evaluate_population(env, pop, fused=True)
    env.close()
    for p in (0, 2, 4):
        one = PolicyPopulation.from_flat(pop.theta[p:p + 1], pop.d_in, pop.hidden_sizes, pop.activation,
                                         None if pop.mean is None else pop.mean[p:p + 1],
                                         None if pop.std is None else pop.std[p:p + 1], pop.eps)
        env1 = _make(config, E, seed=21, env_id_base=p * E)
        alone = evaluate_population(env1, one, fused=True)
        env1.close()
        assert _equal([x[p:p + 1] for x in whole], alone), (config, p)


@pytest.mark.parametrize("name", ["early", "late", "circle_attrate"])
def test_population_evaluation_against_the_reference_s_own_episodes(name):
    """evaluate_population under the criteria test_hip_trained_policies_fly_the_same_in_the_reference_envs (tests/test_gpu_noise.py)
    applies to evaluation.evaluate: the bundled policy in the env settings tests/golden/policy_eval_stats.json carries, 8 192
    episodes as one population of 8 x 1 024 (eight copies of the policy) -- Welch p > 0.01 on length and return, a std ratio in
    (0.8, 1.25), the terminated share within 4 standard errors + 1e-3."""
    from scipy import stats
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    ref = json.load(open(os.path.join(GOLD, "policy_eval_stats.json")))[name]
    th, m, s = _bundled("hip_policy_circle_attrate_late" if name == "circle_attrate" else f"hip_policy_{name}")
    pop = PolicyPopulation.from_flat(th.expand(8, -1), m.numel(), (50, 50), "relu", m.expand(8, -1), s.expand(8, -1), 1e-5)
    env = pds.make(ref.get("env_id", HOVER), num_envs=8192, seed=5, **ref.get("env_kwargs", {}))
    ret, length, _ = evaluate_population(env, pop, fused=True)
    ret, length = ret.reshape(-1).numpy().astype(np.float64), length.reshape(-1).numpy().astype(np.float64)
    rl, rr = np.array(ref["ep_len"], dtype=np.float64), np.array(ref["ep_ret"], dtype=np.float64)
    for mine, theirs, what in ((length, rl, "episode length"), (ret, rr, "episode return")):
        t, p = stats.ttest_ind(mine, theirs, equal_var=False)
        print(f"{name} {what}: {mine.mean():.3f} +- {mine.std() / np.sqrt(len(mine)):.3f} vs {theirs.mean():.3f} +- "
              f"{theirs.std() / np.sqrt(len(theirs)):.3f}, Welch p {p:.4f}, std ratio {mine.std() / max(theirs.std(), 1e-9):.4f}")
        assert p > 0.01, (name, what, mine.mean(), theirs.mean(), t, p)
        assert 0.8 < mine.std() / max(theirs.std(), 1e-9) < 1.25, (name, what, mine.std(), theirs.std())
    term_ref = float(np.mean(ref["terminated"]))
    term_mine = float((length < env._max_episode_steps).mean())
    se = np.sqrt(max(term_ref * (1 - term_ref), 1e-4) / len(rl))
    print(f"{name} terminated share: {term_mine:.4f} vs {term_ref:.4f} (4 se + 1e-3 = {4 * se + 1e-3:.4f})")
    assert abs(term_mine - term_ref) < 4 * se + 1e-3, (name, term_mine, term_ref)
    env.close()


def _snapshot(env):
    sd = env.state_dict()  # every get_state field + the tick
    return {f: v.clone() for f, v in sd.items() if f not in ("tick", "observation_history")}, sd["tick"]


def _unchanged(env, snap):
    before, tick = snap
    assert env.tick == tick and env.sync_tick() == tick
    for f, v in before.items():
        assert torch.equal(env.get_state(f), v), f


@pytest.mark.parametrize("case", ["ground_effect", "history4"])
def test_refusals_leave_the_env_as_it_was_and_auto_falls_back(case):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    kw = dict(use_ground_effect=True) if case == "ground_effect" else dict(observation_history_size=4)
    env = pds.make(HOVER, num_envs=128, seed=3, max_episode_steps=30, **kw)
    env.reset()
    torch.manual_seed(0)
    d_in = env.obs_dim
    n = 50 * d_in + 50 + 50 * 50 + 50 + 4 * 50 + 4
    pop = PolicyPopulation.from_flat(0.1 * torch.randn(2, n), d_in, (50, 50), "relu")
    snap = _snapshot(env)
    with pytest.raises(NotImplementedError):
        evaluate_population(env, pop, fused=True)
    _unchanged(env, snap)
    out = evaluate_population(env, pop, fused="auto")  # the composed path
    for x in out:
        assert tuple(x.shape) == (2, 64) and bool(torch.isfinite(x).all())
    assert float(out[1].min()) >= 1 and float(out[1].max()) <= 30
    env.step(torch.zeros(128, 4, device=env.device))  # the composed path leaves an env that steps
    env.close()


def test_abi_refusals_leave_the_handle_as_it_was():
    """PDS_EUNSUPPORTED for a handle without auto_reset; PDS_EINVAL for the argument errors; nothing moves"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.evaluation import fused_evaluation_built
    env = pds.make(HOVER, num_envs=128, seed=3, auto_reset=False)
    obs, _ = env.reset()
    pop = _population("hover_default", 2).to(env.device)
    out = [torch.zeros(128, device=env.device) for _ in range(3)]
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(e, P=2, E=64, shape=None, params=pop.theta, mean=pop.mean, std=pop.std, T=10, o=None):
        shape = shape or pop.mlp(0)
        return e.lib.pds_evaluate_policies(e._handle, P, E, C.byref(shape), p(params), p(mean) if mean is not None else None,
                                           p(std) if std is not None else None, pop.eps, T, p(o if o is not None else obs),
                                           p(out[0]), p(out[1]), p(out[2]), e._stream())

    snap = _snapshot(env)
    assert not fused_evaluation_built(env)
    assert call(env) == native.EUNSUPPORTED and b"auto_reset" in env.lib.pds_last_error(env._handle)
    _unchanged(env, snap)
    env.close()

    env = pds.make(HOVER, num_envs=128, seed=3)
    assert fused_evaluation_built(env)
    assert call(env) == native.EINVAL and b"before pds_reset" in env.lib.pds_last_error(env._handle)  # never reset
    obs, _ = env.reset()
    snap = _snapshot(env)
    bad = pop.mlp(0); bad.d_in = 40
    wide = pop.mlp(0); wide.h1 = 65
    out5 = pop.mlp(0); out5.d_out = 5
    for rc in (call(env, P=3), call(env, P=4, E=32), call(env, P=1, E=128, T=0), call(env, shape=bad), call(env, shape=wide),
               call(env, shape=out5), call(env, std=None), call(env, T=0)):
        assert rc == native.EINVAL and len(env.lib.pds_last_error(env._handle)) > 0
    assert env.lib.pds_evaluate_policies(env._handle, 2, 64, C.byref(pop.mlp(0)), None, None, None, 0.0, 10, p(obs), p(out[0]),
                                         p(out[1]), p(out[2]), env._stream()) == native.EINVAL  # a NULL pointer
    _unchanged(env, snap)
    env.step(torch.zeros(128, 4, device=env.device))  # still a reset handle
    env.close()

    env = pds.make(HOVER, num_envs=128, seed=3, use_ground_effect=True)  # an env configuration outside rollout_supported
    obs, _ = env.reset()
    snap = _snapshot(env)
    assert call(env) == native.EUNSUPPORTED
    _unchanged(env, snap)
    env.close()


def test_the_handle_afterwards():
    """not reset: step raises until reset(); the tick moved by max_steps, so a second evaluation flies other episodes; a fresh env
    of the same seed reproduces the first call's bits"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    pop = _population("hover_default", 2)
    env = _make("hover_default", 2 * 128, seed=9)
    tick0 = env.tick
    first = evaluate_population(env, pop, fused=True)
    assert env.tick == tick0 + 1 + env._max_episode_steps and env.sync_tick() == env.tick  # reset + max_steps, early stop or not
    zero = torch.zeros(256, 4, device=env.device)
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(zero)
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step_k(zero.unsqueeze(0))
    env.reset()
    env.step(zero)
    second = evaluate_population(env, pop, fused=True)
    assert not torch.equal(first[0], second[0])
    env.close()
    env2 = _make("hover_default", 2 * 128, seed=9)
    assert _equal(evaluate_population(env2, pop, fused=True), first)
    env2.close()


def test_takeoff_episodes_freeze_and_the_tile_stops_before_the_last_step():
    """TakeOff never terminates, so the bitwise TakeOff cases above hold only episodes that the limit cuts at the last step.  Here
    the env's TimeLimit (25) is shorter than the steps flown (max_steps = 40): every episode is truncated at step 25, the
    accumulators freeze there, the tile stops, and the composed path flies the 15 steps on into the next episodes -- same bits."""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E = 3, 192
    pop = _population("takeoff", P)
    env_f, env_c = _make("takeoff", P * E, max_episode_steps=25), _make("takeoff", P * E, max_episode_steps=25)
    fused = evaluate_population(env_f, pop, fused=True, max_steps=40)
    composed = evaluate_population(env_c, pop, fused=False, max_steps=40)
    assert _equal(fused, composed)
    assert torch.equal(fused[1], torch.full((P, E), 25.0))
    assert env_f.sync_tick() == env_c.sync_tick()  # the clock moved by max_steps in the tiles that stopped at 25, too
    env_f.close(); env_c.close()


def test_state_fields_and_state_dict_after_an_evaluation_whose_tiles_stopped_at_different_steps():
    """Between launches the library reads ONE parity of the state ring for all envs (which slot is last_action, which
    prev_action): tiles that stopped after an odd and after an even number of steps must leave the same one.  Fused evaluation
    with mixed stop steps, reset, three steps with distinct actions: last_action / prev_action are the actions fed in, in every
    tile; and a fresh env continues from the state_dict bit for bit."""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E, limit = 16, 64, 40
    pop = _population("hover_lean", P, seed=5)
    env = _make("hover_lean", P * E, seed=13, max_episode_steps=limit)
    _, length, _ = evaluate_population(env, pop, fused=True)
    stop = length.max(dim=1).values.int().tolist()  # E = 64: one tile per policy; it ran until its last first episode ended
    print("steps each tile ran:", stop)
    assert {k & 1 for k in stop} == {0, 1}, stop  # the case holds tiles of both parities
    env.reset()
    n, dev = P * E, env.device
    g = torch.Generator().manual_seed(4)
    acts = [(0.3 * torch.rand(n, 4, generator=g) - 0.25).to(dev) for _ in range(3)]  # distinct, inside the action bounds
    fresh = torch.ones(n, dtype=torch.bool, device=dev)
    for a in acts:
        _, _, term, trunc, _ = env.step(a)
        fresh &= ~(term | trunc)  # (an env that finished was reset in place: its action history starts again)
    assert int(fresh.sum()) > n // 2
    for t in range(P):  # per tile, so that a failure names it
        rows = fresh[t * E:(t + 1) * E]
        assert torch.equal(env.get_state("last_action")[t * E:(t + 1) * E][rows], acts[2][t * E:(t + 1) * E][rows]), (t, stop[t])
        assert torch.equal(env.get_state("prev_action")[t * E:(t + 1) * E][rows], acts[1][t * E:(t + 1) * E][rows]), (t, stop[t])
    sd = env.state_dict()
    env2 = _make("hover_lean", n, seed=13, max_episode_steps=limit)
    env2.reset()
    env2.load_state_dict(sd)
    for f in ("last_action", "prev_action"):
        assert torch.equal(env2.get_state(f), sd[f]), f
    for k in range(6):
        a = (0.3 * torch.rand(n, 4, generator=g) - 0.25).to(dev)
        out1, out2 = env.step(a), env2.step(a)
        for x, y in zip(out1[:4], out2[:4]):
            assert torch.equal(x, y), k
        assert torch.equal(out1[4]["cost"], out2[4]["cost"])
    env.close(); env2.close()


def test_only_a_reset_of_every_env_lifts_the_state_an_evaluation_leaves():
    """the envs outside a mask would keep what the evaluation left (tiles stopped at steps of their own): a masked reset is
    refused, an edit of a state field does not make the env steppable, reset() does"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    pop = _population("hover_default", 2)
    env = _make("hover_default", 2 * 64, seed=4)
    evaluate_population(env, pop, fused=True)
    tick = env.tick
    mask = torch.zeros(128, dtype=torch.uint8, device=env.device)
    mask[:64] = 1
    with pytest.raises(ValueError, match="after pds_evaluate_policies"):
        env.reset(mask=mask)
    assert env.tick == tick and env.sync_tick() == tick
    env.set_state("pos", env.get_state("pos"))
    zero = torch.zeros(128, 4, device=env.device)
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(zero)
    env.reset()
    env.step(zero)
    env.reset(mask=mask)
    env.step(zero)
    env.close()


def test_the_caller_s_population_stays_where_it_is():
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    pop = _population("hover_default", 2)
    env = _make("hover_default", 2 * 64, seed=4, max_episode_steps=20)
    a = evaluate_population(env, pop, fused=1)  # (a truthy non-bool is True: the kernel)
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(torch.zeros(128, 4, device=env.device))
    assert not pop.theta.is_cuda and not pop.mean.is_cuda and not pop.std.is_cuda
    env.close()
    env = _make("hover_default", 2 * 64, seed=4, max_episode_steps=20)
    assert _equal(a, evaluate_population(env, pop, fused=False))
    env.close()


def test_log_dir_writes_one_directory_per_policy(tmp_path):
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    pop = _population("hover_default", 2)
    env = _make("hover_default", 2 * 64, seed=2)
    ret, _, cost = evaluate_population(env, pop, fused=True, log_dir=str(tmp_path))
    for p in range(2):
        r = [float(x) for x in open(tmp_path / str(p) / "returns.csv").read().split()]
        c = [float(x) for x in open(tmp_path / str(p) / "costs.csv").read().split()]
        assert np.allclose(r, ret[p].numpy()) and np.allclose(c, cost[p].numpy()) and len(r) == 64
    env.close()
