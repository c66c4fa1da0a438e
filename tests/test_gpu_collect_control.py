"""pds_collect_control (include/pds_collect_control.h, csrc/pds_collect.h): the one-launch off-policy collection under the PID
control modes (AttitudeRate, Attitude) and with the latency ring, bit for bit against the per-step composition of
tests/test_gpu_collect.py -- pds_mlp_forward + pds_ddpg_explore / pds_sac_sample + pds_step + the ring writes.  Compared: oa, obs2,
rew, done, the final obs, ep_ret / ep_len, the tile statistics and afterwards every state field pds_get_state reads (PDS_F_PID,
PDS_F_ACTION_BUFFER and PDS_F_ACTION_IDX among them: test_gpu_collect._assert_bitwise walks env.state_dict()).

Shapes: N = 200 (three whole tiles and one of 8 rows), max_episode_steps = 5, launches of 3 and then 12 steps against ONE composed
run of 15 -- the TimeLimit of the envs that never terminate falls on steps 2 and 7 of the second launch and on its last one, the
PID state and the delayed-action ring are reset inside the launch and carried from one launch into the next; the replay ring has
16 blocks and is entered at block 6, so it wraps inside the second launch.  latency 0.02 s = 2 and 0.05 s = 5 physics steps: the
delayed-action ring (one write per physics step) wraps inside 12 steps and, at K = 1, does not."""
import math

import numpy as np
import pytest
import torch

import test_gpu_collect as tg
import variant_cases as vc

pytestmark = pytest.mark.gpu
DEV = tg.DEV
DDPG, SAC = tg.DDPG, tg.SAC
MODES = pytest.mark.parametrize("mode", [DDPG, SAC], ids=["ddpg", "sac"])
LEAN = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0)
LIMIT = 5
N = 200
LOG_STD4 = [math.log(0.1), math.log(0.3), math.log(0.5), math.log(0.7)]
PAIRS = [("PWM", True), ("AttitudeRate", False), ("AttitudeRate", True), ("Attitude", False), ("Attitude", True)]  # (control mode, latency ring)


def control_family(task, motor, dr, tn, on, ge, ctrl, lat, hold):
    """"control" where pds_collect_control flies what pds_collect does not, written out from include/pds_collect_control.h and
    NOT read from the library: Hover and Circle, a PID control mode and / or the latency ring, no Kalman hold, no ground effect,
    noise all off or the reference's default, with and without motor dynamics"""
    if task == "takeoff" or hold or ge or (ctrl == "PWM" and not lat):
        return None
    if not ((dr and tn and on) or not (dr or tn or on)):
        return None
    return "control"


def _table():
    """[(id, env id, kwargs without the latency value)]: {Hover, Circle} x {with, without motor dynamics} x {lean, full} x PAIRS"""
    out = []
    for (task, env_id) in vc.TASKS[:2]:
        for motor in (False, True):
            for full in (False, True):
                for ctrl, lat in PAIRS:
                    f = (task, motor, full, full, full, False, ctrl, lat, False)
                    assert control_family(*f) == "control" and vc.collect_family(*f) is None and vc.family(*f) in ("pid", "latency")
                    out.append((vc._name(*f), env_id, vc.kwargs_of(*f[1:])))
    return out


TABLE = _table()
assert len(TABLE) == 40 and len({t[0] for t in TABLE}) == 40


def _kw(kw, latency):
    return dict(kw, latency=latency) if kw.get("use_latency") else dict(kw)


def _make(env_id, kw, n=N, limit=LIMIT, seed=11):
    import phoenix_drone_simulation_amd as pds
    return pds.make(env_id, num_envs=n, device=DEV, seed=seed, max_episode_steps=limit, **kw)


def _launch(env, fm, mode, K, buf, first_call, state, log_std, control=True):
    """one pds_collect_control (control=False: pds_collect) on the state's three tensors in place -> the statistics slab"""
    from phoenix_drone_simulation_amd.fused import collect_control_supported, collect_tiles, fused_collect
    assert collect_control_supported(env, fm, mode)
    obs, ep_ret, ep_len = state
    slab = torch.full((collect_tiles(env), 8), float("nan"), device=DEV)
    fused_collect(env, fm, mode, K, tg.ACT_LIMIT, log_std if mode == DDPG else None, tg.SEED, first_call, buf.oa, buf.obs2, buf.rew,
                  buf.done, buf.ptr, obs, ep_ret, ep_len, slab, control=control)
    buf.advance(K)
    return slab


def _fresh_state(env):
    n = env.num_envs
    return (env.reset()[0].clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV))


def _pair(env_id, kw, mode, launches, n=N, limit=LIMIT, blocks=None, ptr_block=0, fill=None, keep=False):
    """the launches (state carried over) against ONE composed run of sum(launches) steps, everything on its bits
    -> (slabs, composed per-step data[, the two envs and their (obs, ep_ret, ep_len)])"""
    K = sum(launches)
    env_f, env_c = _make(env_id, kw, n, limit), _make(env_id, kw, n, limit)
    D = env_f.obs_dim
    fm = tg._actor(D, mode)
    ls = torch.tensor(LOG_STD4, dtype=torch.float32, device=DEV)
    buf_f, buf_c = tg._ring(n, D, blocks or K, fill), tg._ring(n, D, blocks or K, fill)
    buf_f.ptr = buf_c.ptr = ptr_block * n
    out_c = tg._composed(env_c, fm, mode, K, buf_c, log_std=ls)
    state = _fresh_state(env_f)
    slabs, call = [], 1
    for k in launches:
        slabs.append(_launch(env_f, fm, mode, k, buf_f, call, state, ls))
        call += k
    tg._assert_bitwise(env_f, env_c, buf_f, buf_c, state, out_c[:3], (env_id, kw, mode, n, launches))
    if keep:
        return slabs, out_c[3], (env_f, env_c, state, out_c[:3], buf_f)
    env_f.close(); env_c.close()
    return slabs, out_c[3]


def _exact_statistics(slab, steps, n):
    """count, length sum, min and max exactly, return min / max exactly, return sum and sum of squares at rtol 1e-5 (a fixed-order
    float32 sum of at most a few hundred terms of like sign: tests/test_gpu_collect.py), per tile, against the composed steps"""
    slab = slab.double().cpu()
    for t in range((n + 63) // 64):
        rows = slice(64 * t, 64 * (t + 1))
        lens = torch.cat([ln[rows][dn[rows]].double().cpu() for dn, _, _, _, ln in steps])
        rets = torch.cat([ret[rows][dn[rows]].double().cpu() for dn, _, _, ret, _ in steps])
        got = slab[t]
        assert got[0] == lens.numel() >= 1
        assert got[5] == lens.sum() and got[6] == lens.min() and got[7] == lens.max()
        assert got[3] == rets.min() and got[4] == rets.max()
        assert abs(got[1] - rets.sum()) <= 1e-5 * abs(rets.sum())
        assert abs(got[2] - (rets * rets).sum()) <= 1e-5 * (rets * rets).sum()


# ---- every built variant, both modes -------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("vid,env_id,kw", TABLE, ids=[t[0] for t in TABLE])
def test_every_control_variant_fused_equals_composed(vid, env_id, kw, mode):
    """the whole table (module docstring).  DDPG flies the ring variants at latency 0.02 s, SAC at 0.05 s."""
    latency = 0.02 if mode == DDPG else 0.05
    fill = -7.5
    slabs, steps = _pair(env_id, _kw(kw, latency), mode, (3, 12), blocks=16, ptr_block=6, fill=fill)
    n_term, n_trunc = tg._counts(steps)
    assert n_trunc >= 1 and int(steps[14][2].sum()) >= 1  # the TimeLimit cuts episodes, also on the last step of the launch
    _exact_statistics(slabs[1], steps[3:], N)


@MODES
@pytest.mark.parametrize("K", [1, 12])
@pytest.mark.parametrize("latency,rows", [(0.02, 2), (0.05, 5)], ids=["lat2", "lat5"])
@pytest.mark.parametrize("env_id,kw", [(vc.HOVER, dict(control_mode="AttitudeRate", use_latency=True)),
                                       (vc.CIRCLE, dict(LEAN, use_latency=True, use_motor_dynamics=True))],
                         ids=["hover-attituderate-full-lat", "circle-pwm-lean-motor-lat"])
def test_one_launch_from_a_fresh_reset(env_id, kw, latency, rows, K, mode):
    """K = 1 and K = 12 from a fresh reset: the delayed-action ring of `rows` rows takes one write per physics step
    (aggregate_phy_steps = 1 per env step), so it wraps inside the 12 steps and does not at K = 1; the index it stops at is
    compared with the state"""
    env = _make(env_id, _kw(kw, latency), 64)
    assert env.latency_steps == rows and env.aggregate_phy_steps == 1
    assert (K > rows) == (K == 12)
    env.close()
    _pair(env_id, _kw(kw, latency), mode, (K,), blocks=2 if K == 1 else 4, ptr_block=1 if K == 1 else 3)


@pytest.mark.parametrize("env_id,kw", [(vc.HOVER, dict(LEAN, control_mode="AttitudeRate")),
                                       (vc.HOVER, dict(LEAN, use_latency=True, latency=0.02)),
                                       (vc.HOVER, dict(use_latency=True, latency=0.02)),
                                       (vc.CIRCLE, dict(control_mode="Attitude", use_latency=True, latency=0.05))],
                         ids=["hover-attituderate-lean", "hover-pwm-lean-lat", "hover-pwm-full-lat", "circle-attitude-full-lat"])
def test_257_tiles_take_the_two_team_form_where_it_fits(env_id, kw):
    """N = 257 x 64, the tile count of tests/test_gpu_collect_variants.py: above 256 tiles two teams per block where the two-team
    code object needs no more scratch than the one-team one (the two lean cases; the two default-noise ring cases spill there and
    stay on one team per block), the last block half filled.  A limit of 12: K = 2 from a fresh reset, terminations only."""
    _pair(env_id, kw, SAC, (2,), n=257 * 64, limit=12)


# ---- continuity ----------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("env_id,kw", [(vc.HOVER, dict(control_mode="Attitude", use_latency=True, latency=0.05)),
                                       (vc.CIRCLE, dict(LEAN, control_mode="AttitudeRate", use_motor_dynamics=True))],
                         ids=["hover-attitude-full-lat", "circle-attituderate-lean-motor"])
def test_two_launches_of_6_are_one_of_12_and_a_step_goes_on(env_id, kw, mode):
    """K = 6 twice against K = 12 once (and both against the composed run), then ONE pds_step with the same action on the env
    the launches left and on the env the per-step loop left: observation, reward, flags, final_obs and every state field on
    their bits"""
    _, _, (env_a, env_c, state_a, out_c, buf_a) = _pair(env_id, kw, mode, (6, 6), keep=True)
    _, _, (env_b, env_c2, state_b, _, buf_b) = _pair(env_id, kw, mode, (12,), keep=True)
    for name in ("oa", "obs2", "rew", "done"):
        assert tg._same(getattr(buf_a, name), getattr(buf_b, name)), name
    for x, y in zip(state_a, state_b):
        assert tg._same(x, y)
    g = torch.Generator(device=DEV).manual_seed(9)
    a = torch.rand(N, 4, device=DEV, generator=g) * 2 - 1
    outs = []
    for env in (env_a, env_b, env_c):
        o, r, te, tr, info = env.step(a)
        fin = torch.where((te | tr).unsqueeze(-1), info["final_obs"], torch.zeros_like(o))  # (rows of finished envs only: the others are not written)
        outs.append((o.clone(), r.clone(), te.clone(), tr.clone(), fin, env.state_dict()))
    for other in outs[:2]:
        for x, y in zip(other[:5], outs[2][:5]):
            assert tg._same(x, y)
        for f, v in outs[2][5].items():
            assert (other[5][f] == v) if f == "tick" else tg._same(other[5][f], v), f
    for env in (env_a, env_b, env_c, env_c2):
        env.close()


# ---- the entry point -----------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("case", ["hover_default", "circle_motor", "takeoff"])
def test_on_a_plain_pwm_handle_it_gives_the_bits_of_pds_collect(case, mode):
    from phoenix_drone_simulation_amd.fused import collect_control_supported, collect_supported
    env_id, kw = tg.CASES[case]
    envs = [_make(env_id, kw, 128, limit=3) for _ in range(2)]
    fm = tg._actor(envs[0].obs_dim, mode)
    assert collect_supported(envs[0], fm, mode) and collect_control_supported(envs[0], fm, mode)
    ls = torch.tensor(LOG_STD4, dtype=torch.float32, device=DEV)
    bufs = [tg._ring(128, envs[0].obs_dim, 4) for _ in range(2)]
    states = [_fresh_state(e) for e in envs]
    slabs = [_launch(e, fm, mode, 4, b, 1, s, ls, control=c) for e, b, s, c in zip(envs, bufs, states, (True, False))]
    tg._assert_bitwise(envs[0], envs[1], bufs[0], bufs[1], states[0], states[1], case)
    assert tg._same(slabs[0], slabs[1])
    for e in envs:
        e.close()


def _control_call(env, fm, mode):
    """tests/test_gpu_collect.py _call through pds_collect_control: valid arguments, every buffer keeps its sentinel where the
    call is refused"""
    from phoenix_drone_simulation_amd import fused
    plain = fused.fused_collect
    fused.fused_collect = lambda *a, **k: plain(*a, control=True, **k)
    try:
        tg._call(env, fm, mode)
    finally:
        fused.fused_collect = plain


REFUSED = [
    ("hold", vc.HOVER, dict(observation_frequency=50)),
    ("hold_attitude_rate", vc.HOVER, dict(observation_frequency=50, control_mode="AttitudeRate")),
    ("ground_effect", vc.HOVER, dict(use_ground_effect=True)),
    ("ground_effect_attitude", vc.CIRCLE, dict(use_ground_effect=True, control_mode="Attitude")),
    ("history4", vc.HOVER, dict(observation_history_size=4, control_mode="AttitudeRate")),
    ("dr_only_latency", vc.HOVER, dict(motor_thrust_noise=0, observation_noise=-1, use_latency=True)),
    ("takeoff_latency", vc.TAKEOFF, dict(use_latency=True)),
    ("takeoff_motor_dynamics", vc.TAKEOFF, dict(use_motor_dynamics=True)),
    ("no_auto_reset", vc.CIRCLE, dict(control_mode="AttitudeRate", auto_reset=False)),
]


@pytest.mark.parametrize("name,env_id,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_what_is_not_built_is_refused_with_the_handle_unchanged(name, env_id, kw):
    from phoenix_drone_simulation_amd.fused import collect_control_supported
    n = 128
    env = _make(env_id, kw, n, limit=12)
    env.reset()
    env.step(torch.zeros(n, 4, device=DEV))
    snap = tg._snapshot(env)
    for mode in (DDPG, SAC):
        fm = tg._actor(env.obs_dim, mode)
        assert not collect_control_supported(env, fm, mode)
        with pytest.raises(NotImplementedError):
            _control_call(env, fm, mode)
        tg._unchanged(env, snap)
    env.step(torch.zeros(n, 4, device=DEV))
    assert env.tick == snap[1] + 1
    env.close()


def test_takeoff_under_a_pid_mode_is_no_handle_at_all():
    """TakeOff + PID never reaches the entry point: the constructor refuses it (envs/takeoff.py:225 fixes control_mode PWM)"""
    with pytest.raises(TypeError):
        _make(vc.TAKEOFF, dict(control_mode="AttitudeRate"), 64)


@pytest.mark.parametrize("task,env_id", vc.TASKS)
def test_the_library_agrees_with_the_rule_on_every_configuration(task, env_id):
    """collect_control_supported == (collect_family or control_family) and the actor's d_out is the mode's, for every accepted
    combination of this task; collect_supported keeps answering collect_family alone"""
    from phoenix_drone_simulation_amd.fused import collect_control_supported, collect_supported
    actors, wrong, yes = {}, [], 0
    for vid, eid, kw, _ in vc.VARIANTS:
        if eid != env_id:
            continue
        env = _make(eid, kw, 64, limit=12)
        flags = vc.flags_of(eid, kw)
        old = vc.collect_family(*flags) is not None
        rule = old or control_family(*flags) is not None
        for mode in (DDPG, SAC):
            if (env.obs_dim, mode) not in actors:
                actors[env.obs_dim, mode] = tg._actor(env.obs_dim, mode)
        for mode in (DDPG, SAC):
            for actor_mode in (DDPG, SAC):
                fm = actors[env.obs_dim, actor_mode]
                if collect_control_supported(env, fm, mode) != (rule and mode == actor_mode) or collect_supported(env, fm, mode) != (old and mode == actor_mode):
                    wrong.append((vid, mode, actor_mode))
        env.close()
        yes += rule
    assert yes == {"hover": 4 + 20, "circle": 4 + 20, "takeoff": 2}[task]
    assert not wrong, wrong


# ---- the trainers --------------------------------------------------------------------------------------------------------------
NETS = {"pi": {"hidden_sizes": (32, 32)}, "q": {"hidden_sizes": (32, 32)}}
CONTROL_ENV = dict(control_mode="AttitudeRate", use_latency=True, latency=0.02)


def _ring_equal(a, b):
    for name in ("oa", "obs2", "rew", "done"):
        x, y = getattr(a.buffer, name), getattr(b.buffer, name)
        assert tg._same(x, y), (name, int((tg._bits(x) != tg._bits(y)).sum()))
    assert (a.buffer.ptr, a.buffer.size) == (b.buffer.ptr, b.buffer.size)


def test_a_sac_run_with_control_fused_is_bitwise_the_per_step_run():
    """Circle AttitudeRate + latency, 256 envs, 4 epochs of 60 vector steps, update_every 1000 (K = 4 between updates, cut at the
    end of an epoch): the ring, every parameter of ac and ac_targ, the observation and the episode counts of every epoch on
    their bits; without the keyword the same trainer reports collect_fused False"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.sac import SACTrainer
    n, trs = 256, []
    for kw in (dict(fused_collect=True, control_fused=True), dict(fused_collect=False), dict(fused_collect=True)):
        env = pds.make(vc.CIRCLE, num_envs=n, device=DEV, seed=21, max_episode_steps=6, **CONTROL_ENV)
        trs.append(SACTrainer(env, ac_kwargs=NETS, seed=2, start_steps=512, update_after=512, update_every=1000, steps_per_epoch=60,
                              epochs=4, buffer_size=n * 100, mini_batch_size=64, **kw))
    fused, plain, default = trs
    assert fused.collect_fused is True and fused.control_fused is True
    assert plain.collect_fused is False and default.collect_fused is False and default.control_fused is False
    fused.learn()
    plain.learn()
    _ring_equal(fused, plain)
    for (k, a), (_, b) in zip(list(fused.ac.state_dict().items()) + list(fused.ac_targ.state_dict().items()),
                              list(plain.ac.state_dict().items()) + list(plain.ac_targ.state_dict().items())):
        assert tg._same(a, b), k
    assert fused.updates == plain.updates > 0 and fused.total_steps == plain.total_steps == 4 * 60 * n
    assert fused._noise_calls == plain._noise_calls == 4 * 60 - 2
    for lf, lp in zip(fused.log, plain.log):
        assert lf["episodes"] == lp["episodes"] > 0 and lf["updates"] == lp["updates"]
        assert lf["ep_len"] == lp["ep_len"] and lf["ep_ret_min"] == lp["ep_ret_min"] and lf["ep_ret_max"] == lp["ep_ret_max"]
    assert tg._same(fused.obs, plain.obs) and tg._same(fused.ep_ret, plain.ep_ret)
    sf, sp = fused.env.state_dict(), plain.env.state_dict()
    for f in sf:
        assert (sf[f] == sp[f]) if f == "tick" else tg._same(sf[f], sp[f]), f
    assert fused.collect_launches > 0 and plain.collect_launches == 0
    for t in trs:
        t.env.close()


def test_ddpg_ring_is_bitwise_a_composed_loop_on_pds_ddpg_explore():
    """the statement of tests/test_gpu_collect_trainer.py for DDPG, on Hover Attitude + latency: warm-up fills one epoch; the
    second is collected by pds_collect_control on one side and by step_env -- which acts through pds_ddpg_explore under
    fused_collect=True -- on the other"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ddpg import DDPGTrainer
    n, trs = 256, []
    for _ in range(2):
        env = pds.make(vc.HOVER, num_envs=n, device=DEV, seed=22, max_episode_steps=6, control_mode="Attitude", use_latency=True)
        trs.append(DDPGTrainer(env, ac_kwargs=NETS, seed=3, warmup_steps=8 * n, update_after=8 * n, update_every=700,
                               steps_per_epoch=8, epochs=2, buffer_size=n * 16, mini_batch_size=64, act_noise=0.3,
                               fused_collect=True, control_fused=True))
    fused, composed = trs
    assert fused.collect_fused is True
    composed.collect_fused = False  # the per-step path of the same trainer
    fused.learn_one_epoch(); composed.learn_one_epoch()
    assert fused.in_warm_up and fused.collect_launches == 0
    _ring_equal(fused, composed)
    fused.learn_one_epoch(); composed.learn_one_epoch()
    assert fused.collect_launches == 4 and composed.collect_launches == 0  # K = 1 (an update is due from warm-up), 3, 3, 1
    assert fused.updates == composed.updates == 3
    _ring_equal(fused, composed)
    assert tg._same(fused.obs, composed.obs)
    assert fused.log[1]["episodes"] == composed.log[1]["episodes"] > 0
    fused.env.close(); composed.env.close()


# ---- an independent reference --------------------------------------------------------------------------------------------------
REFERENCE = [("hover-attituderate-lean", vc.HOVER, dict(LEAN, control_mode="AttitudeRate"), 2e-3),
             ("circle-pwm-lean-lat", vc.CIRCLE, dict(LEAN, use_latency=True, latency=0.02), 5e-5)]


@MODES
@pytest.mark.parametrize("name,env_id,kw,bar", REFERENCE, ids=[r[0] for r in REFERENCE])
def test_against_the_collection_loop_on_the_cpu_oracle(name, env_id, kw, bar, mode):
    """tests/collect_oracle.py expresses both configurations as it stands (its Case takes the env's kwargs).  One Hover
    AttitudeRate and one Circle latency collection, N = 128, K = 12 over a limit of 5, against its float32 run -- the reference the
    project's closed-loop bars are stated for (tests/test_gpu_parity.py: lockstep with the float32 oracle, relative error
    |d| / (1 + |x|) over the envs that agree on every flag): 2e-3 for a PID mode on the instant motor model at one sub-step, 5e-5
    for control_mode PWM.  At most max(1, N // 1000) envs may disagree on a flag (collect_oracle.check's cap).  The distance from
    the float64 run is printed beside it."""
    import collect_oracle as co
    import evaluate_oracle as eo
    from test_gpu_collect_reference import _fm
    c = co.Case(f"{name}-{co.MODE_NAME[mode]}", env_id, kw, mode, N=128, launches=(12,), limit=LIMIT, log_std=tuple(LOG_STD4))
    env, fm = _make(env_id, kw, c.N, c.limit, seed=c.env_seed), _fm(c)
    buf = tg._ring(c.N, c.D, c.capacity // c.N, c.fill)
    ls = torch.tensor(c.log_std, dtype=torch.float32, device=DEV)
    state = _fresh_state(env)
    from phoenix_drone_simulation_amd.fused import collect_tiles, fused_collect
    slab = torch.empty(collect_tiles(env), 8, device=DEV)
    fused_collect(env, fm, mode, c.K, c.act_limit, ls if mode == DDPG else None, c.noise_seed, c.first_call, buf.oa, buf.obs2, buf.rew,
                  buf.done, 0, *state, slab, control=True)
    env.close()
    f64 = lambda t: t.double().cpu().numpy()
    got = dict(oa=f64(buf.oa), obs2=f64(buf.obs2), rew=f64(buf.rew), done=f64(buf.done), obs=f64(state[0]), ep_ret=f64(state[1]),
               ep_len=f64(state[2]), slabs=[f64(slab)])
    worst = {}
    for precision in ("f32", "f64"):
        ref = c.reference(precision)
        agree = co.agreement(c, got, ref)
        rows, tiles_ok = co._row_mask(c, agree), co.tiles_compared(c, agree)
        vg, vr = co.float_views(c, got, rows, agree, tiles_ok), co.float_views(c, ref, rows, agree, tiles_ok)
        rel = {k: float((np.abs(vg[k] - vr[k]) / (1.0 + np.abs(vr[k]))).max()) for k in ("oa_obs", "oa_act", "obs2", "rew", "obs_out", "ep_ret")}
        worst[precision] = (max(rel.values()), int((~agree).sum()))
        print(f"MARGIN {c.name} {precision} bar={bar:g} excluded={worst[precision][1]} " + " ".join(f"{k}={v:.3e}" for k, v in rel.items()))
    assert int(c.reference("f32")["fin"].sum()) >= c.N  # every env meets the TimeLimit at least once
    err, excluded = worst["f32"]
    assert excluded <= eo.length_cap(c.N), (c.name, excluded)
    assert err < bar, (c.name, err, bar)
