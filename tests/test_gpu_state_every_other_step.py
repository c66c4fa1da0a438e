"""The lean single-step kernels store position / attitude / velocity / body rates (s0-s2) every other step and recompute them in
between (csrc/pds_types.h kCtrBehindBit, csrc/pds_step.h skip_state_variant, csrc/pds_api.hip materialize_state).  Nothing a caller
can see may depend on it: every case below runs one env in the default form against a twin created under
PDS_STATE_EVERY_STEP=1, which launches the kernels that store every step (=0: every other step at any size; unset, a handle
decides by its size) -- the instantiations a
-DPDS_STATE_EVERY_OTHER_STEP=0 build of the library has -- and compares bit for bit.

Odd ticks are skip steps: after reset() (tick 1) the steps 1, 3, 5, ... of a run skip, the steps 2, 4, ... write.

Action recipe: hover action + 0.5 N(0, 1), drawn on the host, with max_episode_steps = 7.  On the float32 CPU oracle
(oracle.OracleBatch, same seed, actions and sizes) Hover terminates 3-10 % of its envs per step under it, on odd and on even steps
alike, and the TimeLimit cuts the rest: 6.3 finished episodes per env in 40 steps, N = 1: three on skip steps, three on write
steps.  Circle needs about 20 steps to drift out of its 0.25 m and TakeOff never terminates: under the 7-step limit they finish
whole waves at steps 7, 14, 21, 28, 35 (three skip steps, two write steps, every size); Circle's terminations -- 1-6 % of the envs
per step from step 21 on with the default limit of 500 -- have a case of their own at the sizes with more than one wave."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ENV_ID = {"hover": "DroneHoverSimpleEnv-v0", "circle": "DroneCircleSimpleEnv-v0", "takeoff": "DroneTakeOffSimpleEnv-v0"}
DET = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0)
CONFIGS = [("hover", {}), ("circle", {}), ("takeoff", dict(use_ground_effect=True))]
SIZES = [1, 63, 64, 65, 257, 4096 + 3]
FIELDS = ("pos", "rpy", "vel", "omega", "quat", "last_action", "prev_action", "step_count", "quat_sign", "ref_offset")
SEED = 11


def _actions(K, N, dev, seed):
    g = torch.Generator()  # (drawn on the host: the same actions wherever the test runs, and for the CPU oracle)
    g.manual_seed(seed)
    return (-0.11 + 0.5 * torch.randn(K, N, 4, generator=g)).to(dev).contiguous()


def _pair(monkeypatch, task, kw, n, tile=None, **more):
    """(env in the default form, its twin that stores every step), both reset"""
    import phoenix_drone_simulation_amd as pds
    if tile is not None:
        monkeypatch.setenv("PDS_FORCE_TILE", tile)
    mk = lambda: pds.make(ENV_ID[task], num_envs=n, seed=SEED, **dict(dict(DET, max_episode_steps=7), **kw), **more)
    monkeypatch.setenv("PDS_STATE_EVERY_STEP", "0")  # (left to itself a handle of one round of blocks or less stores every step)
    new = mk()
    monkeypatch.setenv("PDS_STATE_EVERY_STEP", "1")
    ref = mk()
    monkeypatch.delenv("PDS_STATE_EVERY_STEP")
    if tile is not None:
        monkeypatch.delenv("PDS_FORCE_TILE")
    oa, _ = new.reset()
    ob, _ = ref.reset()
    assert torch.equal(oa, ob)
    return new, ref


def _same_step(ra, rb, where):
    """all outputs of one step; returns the finished envs"""
    for x, y, name in zip(ra[:4], rb[:4], ("obs", "reward", "terminated", "truncated")):
        assert torch.equal(x, y), (where, name)
    assert torch.equal(ra[4]["cost"], rb[4]["cost"]), (where, "cost")
    fin = ra[2] | ra[3]
    assert torch.equal(ra[4]["final_obs"][fin], rb[4]["final_obs"][fin]), (where, "final_obs")
    return fin


def _same_state(a, b, where):
    for name in FIELDS:
        assert torch.equal(a.get_state(name), b.get_state(name)), (where, name)


def _run(new, ref, acts, where):
    """the steps of acts on both; returns the number of envs that finished on skip steps and on write steps"""
    on_skip = on_write = 0
    for s in range(acts.shape[0]):
        skip = new.tick % 2 == 1  # the tick this launch reads
        fin = _same_step(new.step(acts[s]), ref.step(acts[s]), (where, s))
        if skip:
            on_skip += int(fin.sum())
        else:
            on_write += int(fin.sum())
    return on_skip, on_write


@pytest.mark.parametrize("tile", ["full", "half"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task,kw", CONFIGS)
def test_forty_steps_equal_the_kernels_that_store_every_step(task, kw, n, tile, monkeypatch):
    """40 steps (the last one a write step), the state, one more (a skip step: an odd total), the state again.  Envs finish on
    skip steps and on write steps -- the rows, final_obs and every later step of those envs are part of the comparison."""
    new, ref = _pair(monkeypatch, task, kw, n, tile)
    acts = _actions(41, n, new.device, seed=100 + n)
    on_skip, on_write = _run(new, ref, acts[:40], (task, n, tile))
    assert on_skip > 0 and on_write > 0, (on_skip, on_write)  # (not an empty comparison)
    assert new.tick == ref.tick == 41
    _same_state(new, ref, "after 40")
    _run(new, ref, acts[40:], (task, n, tile, "41st"))
    _same_state(new, ref, "after 41")
    _run(new, ref, acts[:3], (task, n, tile, "after get_state"))
    new.close(); ref.close()


@pytest.mark.parametrize("n", [257, 4096 + 3])
def test_circle_terminations_on_skip_and_on_write_steps(n, monkeypatch):
    """Circle under the default TimeLimit: single lanes of a wave finish (merged reset under a partial exec mask), from step 21 on."""
    new, ref = _pair(monkeypatch, "circle", dict(max_episode_steps=500), n)
    acts = _actions(41, n, new.device, seed=100 + n)
    on_skip, on_write = _run(new, ref, acts, ("circle", n))
    assert on_skip > 0 and on_write > 0, (on_skip, on_write)
    _same_state(new, ref, "after 41")
    _run(new, ref, acts[:4], ("circle", n, "after get_state"))
    new.close(); ref.close()


def _odd_pair(monkeypatch, task, kw, n=257, steps=5, **more):
    new, ref = _pair(monkeypatch, task, kw, n, **more)
    acts = _actions(steps + 12, n, new.device, seed=7)
    _run(new, ref, acts[:steps], (task, "lead-in"))
    assert new.tick % 2 == 0  # the last step was a skip step
    return new, ref, acts[steps:]


@pytest.mark.parametrize("task,kw", CONFIGS)
def test_entry_points_after_an_odd_number_of_steps(task, kw, monkeypatch):
    """What reads or edits the state after a skip step sees the state of that step: get_state, a masked reset, set_state of
    one field (the other fields of the same quads stay), step_k, count_nonfinite, set_tick -- each followed by steps."""
    n = 257
    dev = None
    for what in ("get_state", "masked_reset", "set_state", "step_k", "set_tick"):
        new, ref, acts = _odd_pair(monkeypatch, task, kw, n)
        dev = new.device
        if what == "get_state":
            for name in ("pos", "rpy", "vel", "omega"):
                assert torch.equal(new.get_state(name), ref.get_state(name)), name
            assert new.count_nonfinite() == ref.count_nonfinite()
        elif what == "masked_reset":
            mask = torch.arange(n, device=dev) % 3 == 0
            oa, _ = new.reset(mask=mask)
            ob, _ = ref.reset(mask=mask)
            assert torch.equal(oa, ob)
        elif what == "set_state":
            # (no get_state in front: the edit rewrites s0 and s1 around a velocity, with the position and the angles it finds)
            v = 0.01 * torch.arange(3 * n, dtype=torch.float32).reshape(n, 3).remainder(0.07)
            for e in (new, ref):
                e.set_state("vel", v)
        elif what == "step_k":
            ka, kb = new.step_k(acts[:3]), ref.step_k(acts[:3])
            for x, y in zip(ka[:4], kb[:4]):
                assert torch.equal(x, y)
            assert torch.equal(ka[4]["cost"], kb[4]["cost"])
        else:
            for e in (new, ref):
                assert e.lib.pds_set_tick(e._handle, int(e.tick) + 1) == 0  # the phase flips under a state that is behind
        _same_state(new, ref, what)
        _run(new, ref, acts[3:10], (task, what, "steps after"))
        _same_state(new, ref, (what, "end"))
        new.close(); ref.close()


@pytest.mark.parametrize("task,kw", CONFIGS)
def test_checkpoint_after_an_odd_number_of_steps_resumes_bitwise(task, kw, monkeypatch):
    import phoenix_drone_simulation_amd as pds
    n = 257
    new, ref, acts = _odd_pair(monkeypatch, task, kw, n)
    sd_new, sd_ref = new.state_dict(), ref.state_dict()
    for name in sd_ref:
        x, y = sd_new[name], sd_ref[name]
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, name
    monkeypatch.setenv("PDS_STATE_EVERY_STEP", "0")
    fresh = pds.make(ENV_ID[task], num_envs=n, seed=SEED, max_episode_steps=7, **dict(DET, **kw))
    monkeypatch.delenv("PDS_STATE_EVERY_STEP")
    fresh.reset()
    fresh.load_state_dict(sd_new)
    for s in range(10):
        rf, rr = fresh.step(acts[s]), ref.step(acts[s])
        _same_step(rf, rr, ("resumed", s))
        _same_step(new.step(acts[s]), rr, ("original", s))
    _same_state(fresh, ref, "resumed")
    for e in (new, ref, fresh):
        e.close()


@pytest.mark.parametrize("task,kw", [CONFIGS[0], CONFIGS[2]])
def test_rollout_after_an_odd_number_of_steps(task, kw, monkeypatch):
    """pds_rollout (one launch, T closed-loop steps) from a state that a skip step left behind."""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    n, T = 257, 6
    tr = []
    for every in (False, True):
        monkeypatch.setenv("PDS_STATE_EVERY_STEP", "1" if every else "0")
        env = pds.make(ENV_ID[task], num_envs=n, seed=SEED, max_episode_steps=7, **dict(DET, **kw))
        monkeypatch.delenv("PDS_STATE_EVERY_STEP", raising=False)
        tr.append(PPOTrainer(env, rollout_len=T, epochs=2, seed=5, fused=True, graph_rollout=False, fused_rollout=True))
    acts = _actions(3, n, tr[0].env.device, seed=3)
    for t_ in tr:
        for s in range(3):
            o = t_.env.step(acts[s])[0]
        t_.obs = o.clone()
    assert tr[0].env.tick % 2 == 0
    for t_ in tr:
        t_.roll_out()
    torch.cuda.synchronize()
    assert tr[0].fused_rollout is True and tr[1].fused_rollout is True
    for name in ("obs_buf", "act_buf", "rew_buf", "term_buf", "trunc_buf", "val_buf"):
        assert torch.equal(getattr(tr[0], name), getattr(tr[1], name)), name
    _same_state(tr[0].env, tr[1].env, "after the rollout")
    for t_ in tr:
        t_.env.close()


@pytest.mark.parametrize("task,kw", CONFIGS)
def test_graph_of_64_steps_replayed_twice_equals_128_eager_steps(task, kw, monkeypatch):
    """The phase comes from the tile's clock word in device memory, the flag from the env's counter word: a replay needs no
    host state.  The eager twin stores every step."""
    n, T = 4096 + 3, 64
    new, ref = _pair(monkeypatch, task, kw, n)
    dev = new.device
    acts = _actions(T, n, dev, seed=4)
    rec = torch.zeros(T, n, new.obs_dim, device=dev)
    rew = torch.zeros(T, n, device=dev)
    fin = torch.zeros(T, n, dtype=torch.bool, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for s in range(T):
            o, r, te, tr, info = new.step(acts[s])
            rec[s].copy_(o); rew[s].copy_(r); fin[s].copy_(te | tr)
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for s in range(T):
            o, r, te, tr, info = ref.step(acts[s])
            assert torch.equal(o, rec[s]) and torch.equal(r, rew[s]) and torch.equal(te | tr, fin[s]), (rep, s)
    assert int(fin.sum()) > 0
    assert new.sync_tick() == ref.tick == 1 + 2 * T
    _same_state(new, ref, "after the replays")
    _run(new, ref, acts[:3], (task, "eager again"))
    new.close(); ref.close()
