"""The metrics, stats and record forms of pds_evaluate_policies, the observation-history kernel and the composed path of
evaluation.evaluate_population against an INDEPENDENT reference: tests/flight_oracle.py -- one flight of the float64 CPU oracle
behind a numpy float64 MLP that also keeps the true state, the action, the observation and the oracle's last_action in front
of every step, the eight PDS_EM_* values restated from the text of include/pds.h, the observation sums, and a numpy history
stack.  The other tests of these forms compare the kernels with the composed path, which was written together with them: what
"x(s)" is, which action is `u`, whether the rates are the true ones, in which order the twelve columns come, when the sums
freeze -- here a slip in any of them fails (tests/test_flight_oracle_cpu.py: each moves the reference by more than 100 bars).

The rule (the cases are flight_oracle.FORM_CASES and HISTORY_CASES: P = 8, E = 128, limit 40-60; both paths are held to the
float64 reference separately and stay bitwise equal to each other):
  length    the rule of tests/test_gpu_evaluate_reference.py: equal, except for at most length_cap(N) envs (counted, printed)
  values    state (position, velocity, attitude, body rates), action, observation of every agreeing recorded env at every
            s < length; the four metric sums and tilt_max; every 16-env part of the slab of observation sums (parts that hold a
            disagreeing env are left out and counted): within BAR_UNITS = 4 UNITS of their group.  The unit is measured on the
            reference alone, flight_oracle.units_of: the float32 flight's distance from the float64 flight, floored at the
            float32 rounding of the group's largest magnitude.  4 is the margin of tests/test_gpu_evaluate_reference.py, for its
            reason: the device's FMA contraction and its own sincos sit about as far from libm float32 as that from float64.
  integers  saturated steps and the two crossing counts: equal on the agreeing envs, except for at most length_cap(N) (a rate
            within a rounding of zero changes sign); counted and printed.
No bar is set from the device's output.  Each comparison prints `MARGIN <case> <path> <quantity> unit= err= ratio= excluded=`;
profiles/evaluate_forms_parity_margins.txt keeps a run."""
import numpy as np
import pytest
import torch

import evaluate_oracle as eo
import flight_oracle as fo

pytestmark = pytest.mark.gpu
BAR_UNITS = 4.0
FORM_IDS = [n for _, n in fo.FORM_CASES]


def _population(case):
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    d, h1, h2 = case.shape
    return PolicyPopulation.from_flat(torch.from_numpy(case.rows.copy()), d, (h1, h2), case.activation,
                                      None if case.mean is None else torch.from_numpy(case.mean.copy()),
                                      None if case.std is None else torch.from_numpy(case.std.copy()), case.eps)


def _fly(case, fused, **kw):
    """evaluate_population on a fresh env of the case -> its tuple"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    extra = dict(case.kwargs)
    if getattr(case, "history", None) is not None:
        extra["observation_history_size"] = case.history
    env = pds.make(case.env_id, num_envs=case.N, seed=case.seed, max_episode_steps=case.limit, **extra)
    assert env.obs_dim == case.shape[0]
    out = evaluate_population(env, _population(case), fused=fused, max_steps=case.max_steps, **kw)
    assert env.sync_tick() == 1 + case.max_steps
    env.close()
    return out


def _margin(case, path, quantity, unit, err, excluded):
    ratio = err / unit
    print(f"MARGIN {case.name} {path} {quantity} unit={unit:.3e} err={err:.3e} ratio={ratio:.3f} excluded={excluded}")
    assert ratio <= BAR_UNITS, (case.name, path, quantity, err, unit, ratio)


def _agree(case, path, length, columns=None):
    """the length rule -> (agree mask, number excluded); `columns`: the first R envs per policy of a record"""
    l64 = fo.flight(case, "f64")["length"]
    length = length.numpy().astype(np.float64)
    l64 = l64 if columns is None else l64[:, :columns]
    assert length.shape == l64.shape
    agree = length == l64
    excluded = int((~agree).sum())
    assert excluded <= eo.length_cap(case.N), (case.name, path, excluded, np.argwhere(~agree)[:8].tolist())
    return agree, excluded


def check_metrics(case, path, form, fm, length):
    """the four sums and tilt_max within 4 units; the three integer metrics equal but for length_cap(N) envs"""
    f64, units = fo.flight(case, "f64"), fo.units_of(case)
    agree, excluded = _agree(case, path, length)
    raw = fm.raw.numpy().astype(np.float64)
    assert raw.shape == f64["metrics"].shape and torch.equal(fm.length, length)
    for j in fo.EM_SUMS + (4,):
        err = float(np.abs(raw[..., j] - f64["metrics"][..., j])[agree].max())
        _margin(case, path, f"{form}.{fo.EM[j]}", units[fo.EM[j]], err, excluded)
    wrong = agree & (raw[..., list(fo.EM_INTEGER)] != f64["metrics"][..., list(fo.EM_INTEGER)]).any(axis=-1)
    print(f"MARGIN {case.name} {path} {form}.integer_metrics exceptions={int(wrong.sum())} of {case.N} (cap {eo.length_cap(case.N)}) "
          f"excluded={excluded}")
    assert int(wrong.sum()) <= eo.length_cap(case.N), (case.name, path, np.argwhere(wrong)[:8].tolist())


def check_record(case, path, fl, R, with_observations):
    """state, action and observation of every agreeing recorded env at every s < length within 4 units of their group; rows
    s >= length zero; last_action0 the reference's u0"""
    f64, units = fo.flight(case, "f64"), fo.units_of(case)
    T = case.max_steps
    agree, excluded = _agree(case, path, fl.length, R)
    assert tuple(fl.state.shape) == (case.P, R, T, 12) and tuple(fl.action.shape) == (case.P, R, T, 4)
    state, action = fl.state.numpy().astype(np.float64), fl.action.numpy().astype(np.float64)
    L = fl.length.numpy().astype(int)
    past = np.arange(T)[None, None, :] >= L[:, :, None]
    assert not state[past].any() and not action[past].any()
    form = f"record{R}"
    for g, sl in fo.GROUPS.items():
        err = float(np.abs(state[..., sl] - f64["state"][:, :R, :, sl])[agree].max())
        _margin(case, path, f"{form}.{g}", units[g], err, excluded)
    _margin(case, path, f"{form}.action", units["action"], float(np.abs(action - f64["action"][:, :R])[agree].max()), excluded)
    if with_observations:
        obs = fl.observation.numpy().astype(np.float64)
        assert obs.shape == (case.P, R, T, case.shape[0]) and not obs[past].any()
        _margin(case, path, f"{form}.observation", units["observation"], float(np.abs(obs - f64["observation"][:, :R])[agree].max()), excluded)
    else:
        assert fl.observation is None
    # (u0 is drawn by the reset, before any step: every env counts)
    _margin(case, path, f"{form}.u0", units["u0"], float(np.abs(fl.last_action0.numpy().astype(np.float64) - f64["u0"][:, :R]).max()), 0)


def check_stats(case, path, sums, length):
    """every 16-env part of the slab against the float64 sum of the reference's per-env sums over the same envs; count = the sum
    of the lengths; moments() and pooled() against numpy's mean and M2 of the reference observations"""
    f64, units = fo.flight(case, "f64"), fo.units_of(case)
    agree, _ = _agree(case, path, length)
    D, N = case.shape[0], case.N
    slab = sums.slab.numpy().astype(np.float64)
    assert slab.shape == (N // 64, 4, 2, 64) and not slab[..., D:].any()
    whole = agree.reshape(-1, 16).all(axis=1)
    left_out = int((~whole).sum())
    assert left_out <= eo.length_cap(N)
    for j, name in ((0, "sum_d"), (1, "sum_d2")):
        want = fo.part_sums(f64[name].reshape(N, D))
        err = float(np.abs(slab[:, :, j, :D].reshape(N // 16, D) - want)[whole].max())
        _margin(case, path, f"stats.part_{name}", units["part_" + name], err, left_out)
    assert np.array_equal(sums.count.numpy(), length.numpy().astype(np.float64).sum(axis=1))
    # moments: per policy p without an excluded env, mean = shift + S1 / n and M2 = S2 - S1^2 / n.  With every part of S1
    # and S2 inside its bar b1 = 4 unit(part_sum_d), b2 = 4 unit(part_sum_d2), and K parts per policy: |S1 - S1_ref| <= K b1 =: e1,
    # so the mean is within e1 / n, and M2 within K b2 + (2 |S1_ref| e1 + e1^2) / n
    parts = case.E // 16
    e1, e2 = parts * BAR_UNITS * units["part_sum_d"], parts * BAR_UNITS * units["part_sum_d2"]
    on = np.arange(case.max_steps)[None, None, :] < f64["length"].astype(int)[:, :, None]
    n_dev, mean_dev, m2_dev = (x.numpy() for x in sums.moments())
    clean = agree.all(axis=1)
    assert clean.any()
    rows_of = lambda p: f64["observation"][p][on[p]]  # [count, D] float64: every observation policy p acted on in a first episode
    for p in np.flatnonzero(clean):
        o = rows_of(p)
        mean = o.mean(axis=0)
        m2 = ((o - mean) ** 2).sum(axis=0)
        n = o.shape[0]
        s1_ref = np.abs(f64["sum_d"][p].sum(axis=0))
        assert n_dev[p] == n
        assert (np.abs(mean_dev[p] - mean) <= e1 / n).all(), (case.name, path, p, float(np.abs(mean_dev[p] - mean).max()), e1 / n)
        tol = e2 + (2 * s1_ref * e1 + e1 * e1) / n
        assert (np.abs(m2_dev[p] - m2) <= tol).all(), (case.name, path, p, float((np.abs(m2_dev[p] - m2) / tol).max()))
    if clean.all():  # pooled over all policies: the P policies' bars add up
        o = np.concatenate([rows_of(p) for p in range(case.P)])
        n, mean = o.shape[0], o.mean(axis=0)
        m2 = ((o - mean) ** 2).sum(axis=0)
        n_all, mean_all, m2_all = (x.numpy() for x in sums.pooled())
        shift0 = sums.shift[0].numpy()
        s1_ref = np.abs((o - shift0).sum(axis=0))
        E1, E2 = case.P * e1, case.P * e2
        if case.mean is not None:  # re-centring to policy 0's shift e = shift_p - shift_0: S2 gains 2 e S1, an error of 2 |e| e1
            E2 = E2 + float(np.abs(sums.shift.numpy() - shift0).max()) * 2 * E1
        assert float(n_all) == n
        assert (np.abs(mean_all - mean) <= E1 / n).all()
        assert (np.abs(m2_all - m2) <= E2 + (2 * s1_ref * E1 + E1 * E1) / n).all()


def _same_bits(a, b):
    from test_gpu_evaluate import _equal
    return _equal(a, b)


def _record_tensors(out):
    fl, fm = out[-1], out[3]
    return list(out[:3]) + [fm.raw, fl.state, fl.action, fl.length, fl.last_action0] + ([] if fl.observation is None else [fl.observation])


@pytest.mark.parametrize("record_observations", [True, False], ids=["with_obs", "without_obs"])
@pytest.mark.parametrize("whole", [False, True], ids=["record64", "recordE"])
@pytest.mark.parametrize("kind,name", fo.FORM_CASES, ids=FORM_IDS)
def test_record_against_the_float64_reference(kind, name, whole, record_observations):
    """record = 64 (the first tile of every policy) and record = E, with and without the observations: the recorded flights and
    the metrics of the same launch, the kernel and the composed path each against the reference, and bitwise equal"""
    from test_gpu_evaluate_reference import check
    case = fo.form_case(kind, name)
    R = case.E if whole else 64
    outs = {}
    for path, fused in (("fused", True), ("composed", False)):
        out = _fly(case, fused, metrics=True, record=R, record_observations=record_observations)
        assert len(out) == 5
        check(case, out[:3], f"{path}.record{R}")
        check_metrics(case, path, f"record{R}", out[3], out[1])
        check_record(case, path, out[4], R, record_observations)
        outs[path] = _record_tensors(out)
    assert _same_bits(outs["fused"], outs["composed"])


@pytest.mark.parametrize("kind,name", fo.FORM_CASES, ids=FORM_IDS)
def test_metrics_and_stats_against_the_float64_reference(kind, name):
    """the metrics launch and the stats launch (its metrics, too), the kernel and the composed path each against the reference,
    and bitwise equal"""
    case = fo.form_case(kind, name)
    outs = {}
    for path, fused in (("fused", True), ("composed", False)):
        m = _fly(case, fused, metrics=True)
        check_metrics(case, path, "metrics", m[3], m[1])
        s = _fly(case, fused, metrics=True, obs_stats=True)
        assert len(s) == 5
        check_metrics(case, path, "stats", s[3], s[1])
        check_stats(case, path, s[4], s[1])
        outs[path] = list(m[:3]) + [m[3].raw] + list(s[:3]) + [s[3].raw, s[4].slab]
    assert _same_bits(outs["fused"], outs["composed"])
    f = outs["fused"]
    assert _same_bits(f[:4], f[4:8])  # the stats launch moves nothing of the metrics launch


@pytest.mark.parametrize("name", fo.HISTORY_CASES)
def test_history_against_the_float64_reference(name):
    """one case per input width class of pds_evaluate_policies_history (68, 60, 126 and 192 inputs): return, length and cost by
    the rule of tests/test_gpu_evaluate_reference.py check(), the metrics by the rule above -- the one-launch path and the
    composed path; the composed path with record = 64 (histories record through it): the recorded observation is the reference's
    HISTORY, the stack the actor read"""
    from test_gpu_evaluate_reference import check
    case = fo.history_case(name)
    assert case.shape[0] == fo.HISTORY_INPUTS[name]
    outs = {}
    for path, kw in (("fused", dict(fused=True, history_fused=True)), ("composed", dict(fused=False))):
        out = _fly(case, metrics=True, **kw)
        check(case, out[:3], path)
        check_metrics(case, path, "history", out[3], out[1])
        outs[path] = list(out[:3]) + [out[3].raw]
    assert _same_bits(outs["fused"], outs["composed"])
    rec = _fly(case, False, metrics=True, record=64)
    check_record(case, "composed", rec[4], 64, True)
    assert _same_bits(list(rec[:3]) + [rec[3].raw], outs["composed"])
    length = outs["fused"][1].numpy()
    if case.terminates:
        assert (length < case.limit).any() and (length == case.limit).any()
    else:
        assert (length == case.limit).all()


def test_history_restart_at_a_timelimit_cut_against_the_float64_reference():
    """what evaluate_population cannot show -- it reports nothing behind an env's first finish: the history of a per-step env with
    observation_history_size = 3 (pds_step + pds_history_advance, the steps of the composed path) restarts from the reset row at
    a TimeLimit cut as the reference's stack does.  Hover lean, limit 6 under 15 steps, the float32 actions of the float64
    flight handed to the device open loop: every env is cut at least twice.  The unit is the float32 oracle's distance from the
    float64 oracle under the same actions, over the envs whose done flags agree at every step; restarting one step late moves the
    reference by more than 100 bars."""
    import phoenix_drone_simulation_amd as pds
    case = fo.HistoryCase("restart_h3", eo.HOVER, eo.LEAN, 3, (17, 33), "tanh", 6, True, P=2, E=64, seed=5, rows_seed=7)
    case.max_steps = 15
    N, T, H = case.N, case.max_steps, case.history
    f64 = fo.flight(case, "f64")
    acts = np.ascontiguousarray(f64["action_all"].reshape(N, T, 4).transpose(1, 0, 2)).astype(np.float32)
    f32 = fo.fly(eo.TASK_OF[case.env_id], case.kwargs, case.rows, case.shape, case.activation, case.mean, case.std, case.eps, case.E, T,
                 case.limit, case.seed, "f32", history=H, actions=acts)
    assert np.array_equal(f32["action_all"], f64["action_all"])
    want = f64["observation_all"].reshape(N, T, -1)
    same32 = (f32["done_all"] == f64["done_all"]).all(axis=0)
    assert int((~same32).sum()) <= eo.length_cap(N)
    unit = max(float(np.abs(f32["observation_all"].reshape(N, T, -1) - want)[same32].max()), 2.0 ** -23 * float(np.abs(want).max()))
    late = fo.restack(f64["rows0"], f64["rows_all"], f64["done_all"], H, late=True).transpose(1, 0, 2)
    assert float(np.abs(late - want).max()) > 100 * BAR_UNITS * unit
    env = pds.make(case.env_id, num_envs=N, seed=case.seed, max_episode_steps=case.limit, observation_history_size=H, **case.kwargs)
    obs, _ = env.reset()
    got, done, cut = np.zeros_like(want), np.zeros((T, N), bool), np.zeros((T, N), bool)
    got[:, 0] = obs.cpu().numpy()
    for s in range(T):
        obs, _, term, trunc, _ = env.step(torch.from_numpy(acts[s]).to(env.device))
        done[s], cut[s] = (term | trunc).cpu().numpy(), (trunc & ~term).cpu().numpy()
        if s + 1 < T:
            got[:, s + 1] = obs.cpu().numpy()
    env.close()
    same = (done == f64["done_all"]).all(axis=0)
    excluded = int((~same).sum())
    assert excluded <= eo.length_cap(N)
    # every env restarted at least twice; the TimeLimit alone ended the same episodes as on the oracle, most envs' among them
    assert done.sum(axis=0).min() >= 2 and np.array_equal(cut[:, same], f64["cut_all"][:, same])
    assert f64["cut_all"].any(axis=0).sum() >= N // 2
    _margin(case, "per_step", "history_rows", unit, float(np.abs(got - want)[same].max()), excluded)
