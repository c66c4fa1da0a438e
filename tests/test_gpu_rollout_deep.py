"""pds_rollout_deep (include/pds_rollout_deep.h, csrc/pds_rollout_deep.h): the rollout of an actor with three or four hidden layers
in one launch, the critic behind it -- PPOTrainer(deep_rollout=True).  Every check against the per-step path (pds_mlp_deep_forward
+ pds_gaussian_sample + pds_step + pds_rollout_record, the only path of these actors before, itself pinned to float64 references)
is bit for bit; the one exception is the three `stats` sums, which come from atomics in another order (the helper's rtol 1e-5,
atol 1e-3)."""
import ctypes as C

import pytest
import torch

import variant_cases as vc

pytestmark = pytest.mark.gpu

HOVER, CIRCLE, TAKEOFF = vc.HOVER, vc.CIRCLE, vc.TAKEOFF


def _ac(pi, pi_act, val=(64, 64), val_act="tanh"):
    return {"pi": {"hidden_sizes": tuple(pi), "activation": pi_act}, "val": {"hidden_sizes": tuple(val), "activation": val_act}}


# ---- 1. the recipe of test_trainer._fused_rollout_against_per_step_rollout: max_episode_steps 9 < T 12, two rollouts ------------
CASES = [
    ("hover-default-3-partial-tile", HOVER, {}, 130, dict(ac_kwargs=_ac((50, 30, 20), "relu"))),
    ("circle-lean-motor-4-critic-3", CIRCLE, dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0, use_motor_dynamics=True),
     64 * 5 - 3, dict(ac_kwargs=_ac((32, 32, 32, 32), "tanh", (64, 64, 64)))),
    ("takeoff-ground-effect-obs-noise-3", TAKEOFF, dict(use_ground_effect=True, domain_randomization=-1, motor_thrust_noise=0),
     64, dict(ac_kwargs=_ac((20, 7, 33), "relu"))),
    ("hover-dr-only-4-critic-4", HOVER, dict(observation_noise=-1, motor_thrust_noise=0),
     256, dict(ac_kwargs=_ac((5, 64, 3, 16), "tanh", (64, 64, 64, 64)))),
    ("hover-raw-observations-3", HOVER, {}, 130, dict(ac_kwargs=_ac((50, 30, 20), "relu"), use_standardized_obs=False)),
    # (Hover: its young policies terminate within 12 steps, some on the last one -- Circle's do not)
    ("hover-reset-each-rollout-4", HOVER, {}, 130, dict(ac_kwargs=_ac((32, 32, 32, 32), "tanh"), reset_each_rollout=True)),
]


@pytest.mark.parametrize("name,task,kw,n,trainer_kw", CASES, ids=[c[0] for c in CASES])
def test_deep_rollout_equals_per_step_rollout_bitwise(name, task, kw, n, trainer_kw):
    """every rollout buffer, the env's state, V(final_obs) where pds_gae reads it and what pds_gae makes of them, over two
    consecutive rollouts with cuts and the slot list (the helper asserts fused_rollout is True on the one-launch side, at least n
    finished envs, a non-empty cut set and, under reset_each_rollout, rows that terminated on the last step)"""
    from test_trainer import _fused_rollout_against_per_step_rollout
    _fused_rollout_against_per_step_rollout(task, kw, n, rollouts=2, trainer_kw=dict(trainer_kw, deep_rollout=True))


# ---- 2. every built code object once ---------------------------------------------------------------------------------------------
FAMILY = [v for v in vc.SUPPORTED if v[3] in ("pwm", "takeoff_ge")]
WITHHELD = set()  # (variant id, L) of the variants profiles/rollout_deep_kernel_resources.txt names as withheld: none
SHAPES = {3: ((50, 30, 20), (17, 33, 5)), 4: ((32, 32, 32, 32), (64, 1, 64, 1))}
# (cost_buf is not among them: the per-step rollout of the trainer does not fill it)
BUFFERS = ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "term_buf", "trunc_buf", "ep_ret", "ep_len", "last_val")
FIELDS = ("pos", "vel", "rpy", "omega", "last_action", "step_count")


def _pair(env_id, kw, n, T, limit, **trainer_kw):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    return [PPOTrainer(pds.make(env_id, num_envs=n, seed=3, max_episode_steps=limit, **kw), rollout_len=T, epochs=4, seed=5, fused=True,
                       graph_rollout=False, fused_rollout=fr, deep_rollout=True, **trainer_kw) for fr in (True, False)]


def _same_rollout(a, b, T):
    for name in BUFFERS:
        x, y = getattr(a, name), getattr(b, name)
        assert torch.equal(x, y), (name, (x != y).nonzero()[:4])
    assert torch.equal(a.obs, b.obs)
    cut = a.trunc_buf.bool().clone()
    cut[T - 1] |= a.term_buf[T - 1].bool()
    assert torch.equal(a.fval_buf[cut], b.fval_buf[cut])
    for f in FIELDS:
        assert torch.equal(a.env.get_state(f), b.env.get_state(f)), f
    assert a.env.tick == b.env.tick and a._sample_calls == b._sample_calls
    return cut


def test_the_family_has_48_variants():
    assert len(FAMILY) == 48 and [sum(1 for v in FAMILY if v[1] == t) for t in (HOVER, CIRCLE, TAKEOFF)] == [16, 16, 16]


@pytest.mark.parametrize("L", [3, 4])
@pytest.mark.parametrize("env_id", [HOVER, CIRCLE, TAKEOFF], ids=["hover", "circle", "takeoff"])
def test_every_code_object_equals_the_per_step_path(env_id, L):
    """the 16 variants of one translation unit: T = 4, n = 128 (two tiles), max_episode_steps = 3 -- every env finishes within the
    rollout (the TimeLimit cuts it in step 2 unless it terminated before) and the cut ones go through the slot list"""
    from phoenix_drone_simulation_amd import fused
    T, n = 4, 128
    mine = [v for v in FAMILY if v[1] == env_id]
    assert len(mine) == 16
    for k, (vid, _, kw, _) in enumerate(mine):
        a, b = _pair(env_id, kw, n, T, 3, ac_kwargs=_ac(SHAPES[L][k % 2], ("relu", "tanh")[k % 2]))
        built = a.env.lib.pds_rollout_deep_supported(a.env._handle, C.byref(a.fm_pi.md))
        assert built == (0 if (vid, L) in WITHHELD else 1), vid
        assert fused.rollout_deep_supported(a.env, a.fm_pi) is bool(built)
        if built:
            sa, sb = a.roll_out(), b.roll_out()
            torch.cuda.synchronize()
            assert a.fused_rollout is True and b.fused_rollout is False, vid
            _same_rollout(a, b, T)
            assert bool((a.term_buf | a.trunc_buf).bool().any(0).all()) and bool(a.trunc_buf[2].any()), vid
            torch.testing.assert_close(sa, sb, rtol=1e-5, atol=1e-3)
        a.env.close(); b.env.close()


# ---- 3. deterministic mode ---------------------------------------------------------------------------------------------------
def test_deterministic_actions_are_the_actor_means():
    T, n = 6, 130
    a, b = _pair(HOVER, {}, n, T, 5, ac_kwargs=_ac((50, 30, 20), "relu"))
    for tr in (a, b):
        tr.ac.obs_oms.update(tr.obs + 0.25)  # a standardisation that is not the identity
        tr.ac.eval()
    a._roll_out_fused_deep()
    b._roll_out_eager()
    torch.cuda.synchronize()
    mean, std, eps = a._oms()
    for t in range(T):
        assert torch.equal(a.act_buf[t], a.fm_pi.forward(a.obs_buf[t].contiguous(), mean=mean, std=std, eps=eps)), t
    assert torch.equal(a.logp_buf, b.logp_buf) and torch.equal(a.act_buf, b.act_buf) and torch.equal(a.obs_buf, b.obs_buf)
    assert a._sample_calls == b._sample_calls == T
    a.env.close(); b.env.close()


# ---- 4. trainers -----------------------------------------------------------------------------------------------------------------
def _same_state(a, b):
    for (ka, pa), (kb, pb) in zip(a.ac.state_dict().items(), b.ac.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb), ka


def test_ppo_learns_the_same_parameters_with_the_one_launch_rollout():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    mk = lambda dr: PPOTrainer(pds.make(CIRCLE, num_envs=256, seed=3), rollout_len=16, epochs=3, train_pi_iterations=4, train_v_iterations=1,
                               seed=5, ac_kwargs=_ac((32, 32, 32, 32), "tanh", (64, 64, 64)), deep_rollout=dr)
    a, b = mk(True), mk(False)
    assert a.deep_rollout is True and b.deep_rollout is False
    a.learn(); b.learn()
    torch.cuda.synchronize()
    assert a.fused_rollout is True and b.fused_rollout is False
    _same_state(a, b)
    a.env.close(); b.env.close()


def test_trpo_runs_the_architecture_search_entirely_on_fused_kernels():
    """deep_fused=True, deep_rollout=True together (the reference's experiments/01_find_NN_architecture, --alg trpo): the
    keyword reaches PPOTrainer through NPGTrainer's **kwargs"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.npg import TRPOTrainer
    mk = lambda dr: TRPOTrainer(pds.make(HOVER, num_envs=256, seed=3), rollout_len=16, epochs=3, train_v_iterations=1, seed=5, deep_fused=True,
                                ac_kwargs=_ac((50, 30, 20), "relu"), deep_rollout=dr)
    a, b = mk(True), mk(False)
    assert a.fused is True and a.fm_pi.npg_deep and a.deep_rollout is True and b.deep_rollout is False
    a.learn(); b.learn()
    torch.cuda.synchronize()
    assert a.fused_rollout is True and b.fused_rollout is False
    _same_state(a, b)
    a.env.close(); b.env.close()


def test_an_actor_with_two_hidden_layers_ignores_the_keyword():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    mk = lambda **kw: PPOTrainer(pds.make(HOVER, num_envs=256, seed=3), rollout_len=16, epochs=2, train_pi_iterations=4, train_v_iterations=1,
                                 seed=5, ac_kwargs=_ac((64, 64), "tanh"), **kw)
    a, b = mk(deep_rollout=True), mk()
    assert a.deep_rollout is False
    a.learn(); b.learn()
    torch.cuda.synchronize()
    assert a.fused_rollout is True and b.fused_rollout is True  # pds_rollout, as before
    _same_state(a, b)
    a.env.close(); b.env.close()
    # ... and beside a deep critic it stays per step, and fused_rollout=True still raises in the constructor
    env = pds.make(HOVER, num_envs=128, seed=3)
    kw = dict(rollout_len=4, epochs=2, seed=5, ac_kwargs=_ac((64, 64), "tanh", (64, 64, 64)), deep_rollout=True)
    tr = PPOTrainer(env, **kw)
    tr.roll_out()
    assert tr.deep_rollout is False and tr.fused_rollout is False
    with pytest.raises(NotImplementedError, match="fused_rollout"):
        PPOTrainer(env, fused_rollout=True, **kw)
    env.close()


def test_the_measured_threshold_keeps_the_per_step_path_unless_the_launch_is_asked_for(monkeypatch):
    """DEEP_ROLLOUT_PER_STEP_FROM (ppo.py, from profiles/rollout_deep_timing.txt) is 2^20 envs; set to this env's count here:
    fused_rollout=None settles on the per-step kernels, fused_rollout=True still takes the launch, below it None takes it too"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import ppo
    assert ppo.DEEP_ROLLOUT_PER_STEP_FROM == 1 << 20
    kw = dict(rollout_len=4, epochs=2, seed=5, ac_kwargs=_ac((50, 30, 20), "relu"), deep_rollout=True)
    for limit, fr, want in ((128, None, False), (128, True, True), (129, None, True)):
        monkeypatch.setattr(ppo, "DEEP_ROLLOUT_PER_STEP_FROM", limit)
        env = pds.make(HOVER, num_envs=128, seed=3)
        tr = ppo.PPOTrainer(env, fused_rollout=fr, **kw)
        tr.roll_out()
        assert tr.fused_rollout is want, (limit, fr)
        env.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
REFUSED_ENVS = [
    ("attitude_rate", CIRCLE, dict(control_mode="AttitudeRate")),
    ("latency_ring", HOVER, dict(use_latency=True, latency=0.02)),
    ("kalman_hold", HOVER, dict(observation_frequency=50)),
]


@pytest.mark.parametrize("name,env_id,kw", REFUSED_ENVS, ids=[r[0] for r in REFUSED_ENVS])
def test_envs_outside_the_family_are_refused_with_the_handle_unchanged(name, env_id, kw):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import fused
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    trainer_kw = dict(rollout_len=4, epochs=2, seed=5, fused=True, ac_kwargs=_ac((50, 30, 20), "relu"), deep_rollout=True)
    env = pds.make(env_id, num_envs=128, seed=3, **kw)
    tr = PPOTrainer(env, fused_rollout=True, **trainer_kw)  # the constructor no longer raises
    assert env.lib.pds_rollout_deep_supported(env._handle, C.byref(tr.fm_pi.md)) == 0 and not fused.rollout_deep_supported(env, tr.fm_pi)
    tick, pos = env.tick, env.get_state("pos").clone()
    with pytest.raises(NotImplementedError):
        tr.roll_out()
    assert env.tick == tick and torch.equal(env.get_state("pos"), pos)
    with pytest.raises(NotImplementedError):  # the entry point itself: PDS_EUNSUPPORTED before it touches the handle
        _native_call(tr)
    assert env.tick == tick and torch.equal(env.get_state("pos"), pos)
    env.close()
    env = pds.make(env_id, num_envs=128, seed=3, **kw)
    tr = PPOTrainer(env, **trainer_kw)  # fused_rollout=None: the per-step path
    tr.roll_out()
    assert tr.fused_rollout is False and env.tick == tick + 4
    env.close()


def _native_call(tr, T=None, pi=None, slots=None, act_off=0, **null):
    """pds_rollout_deep directly on the trainer's buffers -> raises what native.check raises for its code"""
    from phoenix_drone_simulation_amd import native
    env, T = tr.env, tr.T if T is None else T
    N, D = tr.N, env.obs_dim
    fin_rows = torch.zeros(T // int(env.cfg.max_episode_steps) + 2, N, D, device=env.device)
    fin_step = torch.full(fin_rows.shape[:2], -1, dtype=torch.int32, device=env.device)
    stats = torch.zeros(3, device=env.device)
    bufs = dict(log_std=tr.ac.pi.log_std, obs_buf=tr._obs_buf, act_buf=tr.act_buf, logp_buf=tr.logp_buf, rew_buf=tr.rew_buf, term_buf=tr.term_buf,
                trunc_buf=tr.trunc_buf, cost_buf=tr.cost_buf, fin_rows=fin_rows, fin_step=fin_step, ep_ret=tr.ep_ret, ep_len=tr.ep_len, stats=stats)
    p = {k: (None if k in null else C.c_void_p(v.data_ptr() + (act_off if k == "act_buf" else 0))) for k, v in bufs.items()}
    tr.fm_pi._bind()
    pi = C.byref(tr.fm_pi.md) if pi is None else (None if pi is False else C.byref(pi))
    mean, std, eps = tr._oms()
    rc = env.lib.pds_rollout_deep(env._handle, T, pi, C.c_void_p(mean.data_ptr()), C.c_void_p(std.data_ptr()), eps, p["log_std"], 5, None, 0, 0,
                                  p["obs_buf"], p["act_buf"], p["logp_buf"], p["rew_buf"], p["term_buf"], p["trunc_buf"], p["cost_buf"],
                                  p["fin_rows"], p["fin_step"], fin_rows.shape[0] if slots is None else slots, p["ep_ret"], p["ep_len"],
                                  p["stats"], None)
    torch.cuda.synchronize()
    native.check(env._handle, rc, "pds_rollout_deep")
    return fin_step


def test_every_einval_of_the_call_leaves_the_handle_as_it_was():
    """with a real handle: NULL pointers, T = 0, d_out 3, a hidden width of 65, slots = 0 and too few, a misaligned act_buf, a missing
    tensor -- ValueError (PDS_EINVAL), tick and pos unchanged, nothing written; pds_rollout_deep_supported answers 0 for the shapes"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    env = pds.make(HOVER, num_envs=128, seed=3, max_episode_steps=3)
    tr = PPOTrainer(env, rollout_len=4, epochs=2, seed=5, fused=True, ac_kwargs=_ac((50, 30, 20), "relu"), deep_rollout=True)
    lib, h, D = env.lib, env._handle, env.obs_dim
    tick, pos = env.tick, env.get_state("pos").clone()
    tr.fm_pi._bind()
    tensors = tr.fm_pi.params
    assert lib.pds_rollout_deep_supported(h, C.byref(tr.fm_pi.md)) == 1
    assert lib.pds_rollout_deep_supported(h, None) == native.EINVAL and lib.pds_rollout_deep_supported(None, C.byref(tr.fm_pi.md)) == native.EINVAL
    calls = [dict(pi=False), dict(log_std=None), dict(obs_buf=None), dict(act_buf=None), dict(fin_rows=None), dict(fin_step=None), dict(stats=None),
             dict(T=0), dict(slots=0), dict(slots=2), dict(act_off=4)]
    d_out3 = native.mlp_deep(D, (50, 30, 20), 3, "relu", tensors=tensors)
    wide = native.mlp_deep(D, (50, 65, 20), 4, "relu", tensors=tensors)
    two = native.mlp_deep(D, (50, 50), 4, "relu", tensors=tensors[:6])
    for m in (d_out3, wide, two):
        assert lib.pds_rollout_deep_supported(h, C.byref(m)) == 0
        calls.append(dict(pi=m))
    missing = native.mlp_deep(D, (50, 30, 20), 4, "relu", tensors=tensors)
    missing.b[3] = None
    calls.append(dict(pi=missing))
    for kw in calls:
        with pytest.raises(ValueError):
            _native_call(tr, **kw)
        assert env.tick == tick and torch.equal(env.get_state("pos"), pos), kw
    assert not bool(tr.act_buf.any()) and not bool(tr.rew_buf.any()) and not bool(tr._obs_buf.any())
    # the same call with nothing wrong flies: T = 4 > max_episode_steps = 3 needs 4 // 3 + 2 = 3 slots
    tr._obs_buf[0].copy_(tr.obs)
    fin_step = _native_call(tr)
    assert env.tick == tick + 4 and bool(tr.act_buf.any())
    # an env's first slot names step 2 exactly where the TimeLimit cut it there (no earlier step can hand a row over); the third
    # slot stays free: a cut in step 2 and the last step are the most one env can have
    assert bool(tr.trunc_buf[2].any()) and torch.equal(fin_step[0] == 2, tr.trunc_buf[2].bool()) and bool((fin_step[2] == -1).all())
    env.close()
