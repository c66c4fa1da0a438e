"""The dispatch tables of the LATER forms of the population evaluation, swept.  tests/test_gpu_evaluate_variants.py flies all 102
supported configurations in both team forms through pds_evaluate_policies; the metrics, stats and record forms are 612 more code
objects -- the same variant-specific env waves with the form's own statements in them (PDS_EM_STEP, PDS_ER_STEP, the alive mask of
the observation sums) -- and pds_evaluate_policies_history has 104 of its own: 26 env configurations x 4 input widths.  Here
EVERY one of them is flown, bit for bit against the composed path (whose env steps are pds_step's: the per-step kernels of that
configuration).  tests/variant_cases.py states both rules in its own words; the library must agree with them."""
import pytest
import torch

import variant_cases as vc
from test_gpu_evaluate_variants import E, LIMIT, MAX_STEPS, _population

pytestmark = pytest.mark.gpu


def _bits_differ(a, b):
    return [int((x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)).sum()) for x, y in zip(a, b)]


def _tensors(stats_out, record_out):
    """every tensor the two flights returned"""
    ret, length, cost, fm, sums = stats_out
    ret2, length2, cost2, fm2, fl = record_out
    return [ret, length, cost, fm.raw, sums.slab, sums.count.float(), ret2, length2, cost2, fm2.raw, fl.state, fl.action, fl.length,
            fl.last_action0] + ([] if fl.observation is None else [fl.observation])


@pytest.mark.parametrize("P", [3, 257], ids=["one_team", "257_tiles"])
@pytest.mark.parametrize("vid,env_id,kw,fam", vc.SUPPORTED, ids=[v[0] for v in vc.SUPPORTED])
def test_every_supported_configuration_stats_and_record_fused_equals_composed(vid, env_id, kw, fam, P):
    """on a pair of envs, a stats flight (obs_stats=True, metrics=True: pds_evaluate_policies_stats) and then a record flight
    (record=64, metrics=True: pds_evaluate_policies_record; the metrics form is the record form without its stores and the stats
    form without its sums), in the same order on both.  P = 3: one team per block; P = 257: two teams where the form's variant
    fits, the last block half filled.
    Without thrust noise and observation noise the record flight starts on the SAME pair, from the envs the stats flight left:
    there a reset is a function of the tick alone (domain randomisation is drawn from it), also behind tiles that stopped at steps
    of their own.  With thrust noise or observation noise it starts on a fresh pair of the same seed: the OU thrust state, the
    gyro bias and its low-pass carry over a reset by design (envs/base.py:411), a tile of the launch stops at its own step and
    the composed path flies every env to max_steps, so the two envs of a pair are not in the same state afterwards
    (tests/test_gpu_evaluate_history.py test_the_handle_afterwards says the same of the history launch)."""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import evaluate_population, fused_evaluation_built
    from test_gpu_evaluate import _equal
    make = lambda: pds.make(env_id, num_envs=P * E, seed=17, max_episode_steps=LIMIT, **kw)
    _, _, dr, tn, on, *_ = vc.flags_of(env_id, kw)
    same_pair = not (tn or on)
    pair = {True: make(), False: make()}
    assert fused_evaluation_built(pair[True])
    pop = _population(pair[True], P, seed=P)
    stats = {fused: evaluate_population(env, pop, fused=fused, max_steps=MAX_STEPS, obs_stats=True, metrics=True) for fused, env in pair.items()}
    if not same_pair:
        assert pair[True].sync_tick() == pair[False].sync_tick() == 1 + MAX_STEPS
        for env in pair.values():
            env.close()
        pair = {True: make(), False: make()}
    record = {fused: evaluate_population(env, pop, fused=fused, max_steps=MAX_STEPS, record=64, metrics=True) for fused, env in pair.items()}
    out = {fused: _tensors(stats[fused], record[fused]) for fused in (True, False)}
    assert _equal(out[True], out[False]), (vid, P, _bits_differ(out[True], out[False]))
    for length in (out[True][1], out[True][7]):
        assert float(length.min()) >= 1 and float(length.max()) <= LIMIT  # every episode finished: at the limit at the latest
        assert int((length == LIMIT).sum()) >= 1
    assert pair[True].sync_tick() == pair[False].sync_tick() == (2 if same_pair else 1) * (1 + MAX_STEPS)
    for env in pair.values():
        env.close()


# ---- the observation-history kernel -------------------------------------------------------------------------------------------
def test_the_history_set_has_the_size_the_rule_gives():
    """26 = Hover and Circle x 3 control modes x {lean, full} x {with, without motor dynamics} + TakeOff x {lean, full}"""
    assert len(vc.HISTORY_SUPPORTED) == 26 == vc.HISTORY_COUNT
    assert len({v[0] for v in vc.HISTORY_SUPPORTED}) == 26


@pytest.mark.parametrize("task,env_id", vc.TASKS)
def test_the_library_agrees_with_the_history_rule_on_every_configuration(task, env_id):
    """pds_evaluate_history_supported(handle, 4) == the rule of tests/variant_cases.py for every accepted combination of this
    task; and where the constructor builds the env with observation_history_size = 4 (it refuses some outside the rule, the
    latency ring among them), fused_history_evaluation_built(env) says the same"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import fused_history_evaluation_built
    wrong, n, built = [], 0, 0
    for vid, eid, kw, _ in vc.VARIANTS:
        if eid != env_id:
            continue
        want = vc.history_family(*vc.flags_of(eid, kw)) is not None
        env = pds.make(eid, num_envs=64, seed=1, **kw)
        if (env.lib.pds_evaluate_history_supported(env._handle, 4) == 1) != want:
            wrong.append(("abi", vid))
        env.close()
        try:
            env = pds.make(eid, num_envs=64, seed=1, observation_history_size=4, **kw)
        except NotImplementedError:
            if want:
                wrong.append(("constructor", vid))
        else:
            if fused_history_evaluation_built(env) != want:
                wrong.append(("built", vid))
            built += int(want)
            env.close()
        n += 1
    assert n == {"hover": 224, "circle": 224, "takeoff": 96}[task]
    assert built == {"hover": 12, "circle": 12, "takeoff": 2}[task]
    assert not wrong, wrong


def _half(env_id, kw):
    noisy = kw.get("observation_noise", 1) > 0
    return {vc.HOVER: 17 if noisy else 21, vc.CIRCLE: 20, vc.TAKEOFF: 24}[env_id]  # (o + 4 action entries; envs/*.py compute_observation)


@pytest.mark.parametrize("name,env_id,kw", vc.HISTORY_SUPPORTED, ids=[v[0] for v in vc.HISTORY_SUPPORTED])
def test_the_library_refuses_more_than_192_inputs(name, env_id, kw):
    import phoenix_drone_simulation_amd as pds
    half = _half(env_id, kw)
    env = pds.make(env_id, num_envs=64, seed=1, **kw)
    assert env.obs_dim == 2 * half
    last = 192 // half
    assert env.lib.pds_evaluate_history_supported(env._handle, last) == 1
    assert env.lib.pds_evaluate_history_supported(env._handle, last + 1) == 0
    env.close()


HISTORY_FLIGHTS = [(f"{name}-h{H}-w{width}", env_id, kw, H, width) for name, env_id, kw in vc.HISTORY_SUPPORTED
                   for H, width in vc.history_sizes(_half(env_id, kw))]


def test_the_history_sweep_has_104_flights_one_per_width_class():
    assert len(HISTORY_FLIGHTS) == 104
    for _, env_id, kw, H, width in HISTORY_FLIGHTS:
        lower = {64: 0, 96: 64, 128: 96, 192: 128}[width]
        assert H != 2 and lower < H * _half(env_id, kw) <= width or (width == 64 and H == 1)


@pytest.mark.parametrize("fid,env_id,kw,H,width", HISTORY_FLIGHTS, ids=[f[0] for f in HISTORY_FLIGHTS])
def test_every_history_configuration_fused_equals_composed(fid, env_id, kw, H, width):
    """all 26 configurations at one H per input width class (<= 64, <= 96, <= 128, <= 192 inputs; H != 2): P = 3, E = 64,
    metrics=True, the one-launch path equal to the composed path on the bits"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import evaluate_population, fused_history_evaluation_built
    from test_gpu_evaluate import _equal
    P = 3
    env_f = pds.make(env_id, num_envs=P * E, seed=17, max_episode_steps=LIMIT, observation_history_size=H, **kw)
    env_c = pds.make(env_id, num_envs=P * E, seed=17, max_episode_steps=LIMIT, observation_history_size=H, **kw)
    assert env_f.obs_dim == H * _half(env_id, kw) <= width and fused_history_evaluation_built(env_f)
    pop = _population(env_f, P, seed=H)
    fused = evaluate_population(env_f, pop, fused=True, history_fused=True, max_steps=MAX_STEPS, metrics=True)
    composed = evaluate_population(env_c, pop, fused=False, max_steps=MAX_STEPS, metrics=True)
    a, b = list(fused[:3]) + [fused[3].raw], list(composed[:3]) + [composed[3].raw]
    assert _equal(a, b), (fid, _bits_differ(a, b))
    length = fused[1]
    assert float(length.min()) >= 1 and float(length.max()) <= LIMIT and int((length == LIMIT).sum()) >= 1
    assert env_f.sync_tick() == env_c.sync_tick() == 1 + MAX_STEPS
    env_f.close(); env_c.close()
