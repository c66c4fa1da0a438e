"""The dispatch of pds_collect, swept, bit for bit against the composed per-step path (the helpers of tests/test_gpu_collect.py).
csrc/pds_collect.h builds ten env variants, two activations and every hidden shape of forward16_shape, a one-team and a two-team
form, a fast and a slow store path per piece; tests/test_gpu_collect.py flies four variants with one tanh actor of (32, 48)
units at act_limit 1 from a fresh reset.  Here: the support rule against tests/variant_cases.py collect_family (written from
the comment of csrc/pds_collect_args.h), all ten variants, every shape of evaluate_oracle.HIDDEN with relu and tanh, whole
pieces that are not 16-byte aligned, the two-team form in DDPG mode, act_limit 0.5 with four distinct log_std entries, a
noise seed and a call index beyond 32 bits, and two launches in a row against one composed run."""
import math

import pytest
import torch

import evaluate_oracle as eo
import test_gpu_collect as tg
import variant_cases as vc

pytestmark = pytest.mark.gpu
DEV = tg.DEV
DDPG, SAC = tg.DDPG, tg.SAC
MODES = pytest.mark.parametrize("mode", [DDPG, SAC], ids=["ddpg", "sac"])
LEAN = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0)
LIMIT = 3  # max_episode_steps: the TimeLimit falls inside every launch of 4 steps
LOG_STD4 = [math.log(0.1), math.log(0.3), math.log(0.5), math.log(0.7)]
BIG_SEED, BIG_CALL = (0xC0FFEE << 32) | 0x5EED0123, 2 ** 33 + 5


def _make(env_id, kw, N, limit=LIMIT):
    import phoenix_drone_simulation_amd as pds
    return pds.make(env_id, num_envs=N, device=DEV, seed=11, max_episode_steps=limit, **kw)


def _pair(env_id, kw, mode, N, launches, limit=LIMIT, act="tanh", hidden=(tg.H1, tg.H2), act_limit=1.0, log_std=None,
          seed=tg.SEED, first_call=1, blocks=None, obs_offset=0, check_inputs=None):
    """the fused launches (one pds_collect each, state carried over) against ONE composed run of sum(launches) steps, bitwise.
    obs_offset: the launch's obs tensor is a view that many floats into a larger buffer.  check_inputs(buf, obs): assertions on
    what the case means to exercise.  -> (fused slabs, composed per-step data)"""
    K = sum(launches)
    env_f, env_c = _make(env_id, kw, N, limit), _make(env_id, kw, N, limit)
    D = env_f.obs_dim
    fm = tg._actor(D, mode, act=act, hidden=hidden)
    ls = None if log_std is None else torch.tensor(log_std, dtype=torch.float32, device=DEV)
    buf_f, buf_c = tg._ring(N, D, blocks or K), tg._ring(N, D, blocks or K)
    kw_run = dict(log_std=ls, act_limit=act_limit, seed=seed)
    out_c = tg._composed(env_c, fm, mode, K, buf_c, first_call=first_call, **kw_run)
    big = torch.zeros(N * D + 8, device=DEV)
    obs = big[obs_offset:obs_offset + N * D].view(N, D)
    obs.copy_(env_f.reset()[0])
    state = (obs, torch.zeros(N, device=DEV), torch.zeros(N, device=DEV))
    if check_inputs is not None:
        check_inputs(buf_f, obs)
    slabs, call = [], first_call
    for k in launches:
        o, er, el, slab = tg._fused(env_f, fm, mode, k, buf_f, first_call=call, state=state, **kw_run)
        assert o is obs
        slabs.append(slab)
        call += k
    assert not bool(big[:obs_offset].any()) and not bool(big[obs_offset + N * D:].any())  # nothing written around the view
    tg._assert_bitwise(env_f, env_c, buf_f, buf_c, state, out_c[:3], (env_id, kw, mode, N, launches))
    env_f.close(); env_c.close()
    return slabs, out_c[3]


def _exact_statistics(slab, steps, N, every_tile_finishes=True):
    """count, length sum, min and max of a launch's slab against the composed run's steps, per tile; a tile without a finished
    episode (only where the caller allows one) holds the neutral values"""
    slab = slab.double().cpu()
    for t in range((N + 63) // 64):
        rows = slice(64 * t, 64 * (t + 1))
        lens = torch.cat([ln[rows][dn[rows]].double().cpu() for dn, _, _, _, ln in steps])
        assert slab[t, 0] == lens.numel()
        if lens.numel() == 0:
            assert not every_tile_finishes
            assert slab[t].tolist() == tg.NEUTRAL
        else:
            assert slab[t, 5] == lens.sum() and slab[t, 6] == lens.min() and slab[t, 7] == lens.max()


# ---- the support rule ------------------------------------------------------------------------------------------------------
def test_the_supported_set_has_the_size_the_rule_gives():
    """10 = Hover and Circle x {lean, full} x {with, without motor dynamics} + TakeOff x {lean, full}"""
    assert len(vc.COLLECT_SUPPORTED) == 10 == vc.COLLECT_COUNT
    count = {t: sum(1 for v in vc.COLLECT_SUPPORTED if v[1] == e) for t, e in vc.TASKS}
    assert count == {"hover": 4, "circle": 4, "takeoff": 2}
    for _, env_id, kw in vc.COLLECT_SUPPORTED:  # what pds_collect flies, pds_rollout flies
        assert vc.family(*vc.flags_of(env_id, kw)) == "pwm"


@pytest.mark.parametrize("task,env_id", vc.TASKS)
def test_the_library_agrees_with_the_rule_on_every_configuration(task, env_id):
    """collect_supported(env, actor, mode) == collect_family(...) and the actor's d_out is the mode's (DDPG 4, SAC 8), for every
    accepted combination of this task"""
    from phoenix_drone_simulation_amd.fused import collect_supported
    actors, wrong, n, yes = {}, [], 0, 0
    for vid, eid, kw, _ in vc.VARIANTS:
        if eid != env_id:
            continue
        env = _make(eid, kw, 64)
        rule = vc.collect_family(*vc.flags_of(eid, kw)) is not None
        for mode in (DDPG, SAC):
            if (env.obs_dim, mode) not in actors:
                actors[env.obs_dim, mode] = tg._actor(env.obs_dim, mode)
        for mode in (DDPG, SAC):
            for actor_mode in (DDPG, SAC):  # an actor of d_out 4 / 8
                want = rule and mode == actor_mode
                if collect_supported(env, actors[env.obs_dim, actor_mode], mode) != want:
                    wrong.append((vid, mode, actor_mode))
        env.close()
        n += 1
        yes += rule
    assert n == {"hover": 224, "circle": 224, "takeoff": 96}[task]
    assert yes == {"hover": 4, "circle": 4, "takeoff": 2}[task]
    assert not wrong, wrong


REFUSED = [
    ("dr_only", vc.HOVER, dict(motor_thrust_noise=0, observation_noise=-1)),
    ("observation_noise_only", vc.CIRCLE, dict(domain_randomization=-1, motor_thrust_noise=0)),
    ("takeoff_motor_dynamics", vc.TAKEOFF, dict(use_motor_dynamics=True)),
    ("takeoff_ground_effect", vc.TAKEOFF, dict(use_ground_effect=True)),
    ("hold", vc.HOVER, dict(observation_frequency=50)),
    ("attitude", vc.CIRCLE, dict(control_mode="Attitude")),
    ("latency_lean", vc.HOVER, dict(LEAN, use_latency=True, latency=0.02)),
]


@pytest.mark.parametrize("name,env_id,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_what_the_rule_refuses_is_refused_with_the_env_untouched(name, env_id, kw):
    from phoenix_drone_simulation_amd.fused import collect_supported
    assert vc.collect_family(*vc.flags_of(env_id, kw)) is None
    N = 128
    env = _make(env_id, kw, N)
    env.reset()
    env.step(torch.zeros(N, 4, device=DEV))
    snap = tg._snapshot(env)
    for mode in (DDPG, SAC):
        fm = tg._actor(env.obs_dim, mode)
        assert not collect_supported(env, fm, mode)
        with pytest.raises(NotImplementedError):
            tg._call(env, fm, mode)
        tg._unchanged(env, snap)
    env.step(torch.zeros(N, 4, device=DEV))  # still a handle that steps
    assert env.tick == snap[1] + 1
    env.close()


# ---- the sweeps --------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("vid,env_id,kw", vc.COLLECT_SUPPORTED, ids=[v[0] for v in vc.COLLECT_SUPPORTED])
def test_every_supported_variant_fused_equals_composed(vid, env_id, kw, mode):
    """N = 128 (two tiles), K = 4 over a TimeLimit of 3: every env finishes inside the launch, Hover envs also by termination"""
    slabs, steps = _pair(env_id, kw, mode, 128, (4,))
    n_term, n_trunc = tg._counts(steps)
    assert n_trunc >= 1
    _exact_statistics(slabs[0], steps, 128)


@MODES
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("hidden", eo.HIDDEN, ids=[f"{a}x{b}" for a, b in eo.HIDDEN])
def test_every_hidden_shape_and_activation(hidden, act, mode):
    """the hidden sizes at which forward16_shape (csrc/pds_mlp_fwd.h) takes another instantiation -- 1, 2, 3, 16, 17, 33, 49, 64
    units -- with relu and tanh in the network waves, on Hover lean, N = 64, K = 3; (64, 64) is the trainers' default"""
    _pair(vc.HOVER, LEAN, mode, 64, (3,), limit=2, act=act, hidden=hidden)


@MODES
@pytest.mark.parametrize("N", [67, 129])
def test_whole_pieces_that_are_not_16_byte_aligned(N, mode):
    """odd N with an even row width (Hover lean: 42 and 46 floats): the blocks of odd s start 8 bytes off a 16-byte boundary,
    and every network wave of every full tile takes collect_store_piece's slow path with rows == 16.  N = 67: a full tile and
    3 rows; N = 129: two full tiles and one row."""
    def inputs(buf, obs):
        D = obs.shape[1]
        assert D % 2 == 0
        for t, w in ((buf.oa, D + 4), (buf.obs2, D)):
            assert t.data_ptr() % 16 == 0
            assert (t.data_ptr() + 1 * N * w * 4) % 16 == 8 and (t.data_ptr() + 3 * N * w * 4) % 16 == 8
            assert (t.data_ptr() + 2 * N * w * 4) % 16 == 0
            assert (64 * w * 4) % 16 == 0 and (16 * w * 4) % 16 == 0  # ... and within a block every piece is as its first
    _pair(vc.HOVER, LEAN, mode, N, (4,), check_inputs=inputs)


@MODES
def test_an_observation_buffer_that_is_only_4_byte_aligned(mode):
    """N = 128 with `obs` a view one float into a larger buffer: o(K) goes out through the slow path of every piece, o(0) comes
    in through scalar loads; the floats around the view stay zero"""
    def inputs(buf, obs):
        assert obs.data_ptr() % 16 == 4 and obs.is_contiguous()
    _pair(vc.HOVER, LEAN, mode, 128, (4,), obs_offset=1, check_inputs=inputs)


def test_257_tiles_take_the_two_team_form_in_ddpg_mode():
    """N = 257 x 64, K = 2, DDPG: two teams per block, the last block half filled (tests/test_gpu_collect.py flies it in SAC
    mode only)"""
    _pair(vc.HOVER, LEAN, DDPG, 257 * 64, (2,), limit=12, log_std=LOG_STD4)


@MODES
@pytest.mark.parametrize("env_kw", [LEAN, {}], ids=["lean", "full"])
def test_act_limit_log_std_seed_and_call_index(env_kw, mode):
    """act_limit = 0.5, four distinct log_std entries (DDPG: a permuted component shows), a noise seed and a first call beyond 32
    bits (the key's and the counter's high words)"""
    slabs, steps = _pair(vc.HOVER, env_kw, mode, 128, (4,), act_limit=0.5, log_std=LOG_STD4, seed=BIG_SEED, first_call=BIG_CALL)
    _exact_statistics(slabs[0], steps, 128)


@MODES
def test_capacity_equal_to_n_every_step_on_the_same_block(mode):
    """capacity == N: every step lands on block 0 and the last one stays (the composed path's store() wraps the same way)"""
    _pair(vc.HOVER, LEAN, mode, 128, (3,), blocks=1)


@MODES
@pytest.mark.parametrize("env_kw", [LEAN, {}], ids=["lean", "full"])
def test_two_launches_in_a_row_are_one_composed_run(env_kw, mode):
    """K = 5, then K = 7 on one env and one ring under a limit of 8: the running return and length, o(K) and the call index carry
    over; the second launch starts in the middle of episodes.  Each launch's slab holds its own steps' episodes."""
    N = 128
    slabs, steps = _pair(vc.HOVER, env_kw, mode, N, (5, 7), limit=8, log_std=LOG_STD4, first_call=BIG_CALL)
    carried = torch.where(steps[4][0], torch.zeros_like(steps[4][4]), steps[4][4])  # the running length behind step 4
    assert bool((carried > 0).any())
    # under a limit of 8 only terminations end an episode within the first five steps: a tile may have none
    _exact_statistics(slabs[0], steps[:5], N, every_tile_finishes=False)
    _exact_statistics(slabs[1], steps[5:], N)  # ... and every env meets the TimeLimit within the second launch
