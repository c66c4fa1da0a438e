"""Observation histories other than 2 on the latency ring, without a GPU: tests/history_latency_oracle.py (the reference's deque of
views, around one env of the CPU oracle) against the reference's own trajectories (tests/golden/history_latency.npz, written by
tests/refgen/gen_golden_history_latency.py); the closed-form rule that csrc/pds_history.hip and envs._advance_history_torch
implement, as a short numpy function, against that wrapper; the slips the wrapper must catch; and the row of
native.HISTORY_LATENCY_SIGNATURES against include/pds_history_latency.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_util as gu
import history_latency_oracle as hlo

# the float64 oracle against the reference: tests/test_oracle_golden.py's bar (test_oracle_f64_matches_reference)
RTOL, ATOL = 1e-12, 1e-13
G = np.load(os.path.join(gu.GOLDEN, "history_latency.npz"))
NAMES = [str(n) for n in G["names"]]
TASKS = dict(zip(NAMES, (str(t) for t in G["tasks"])))


def _fly_fixture(name):
    task, H = TASKS[name], int(G[name + "_H"])
    env = hlo.HistoryLatencyEnv(task, H, "f64", **hlo.fixture_kwargs(G, name, task))
    return env, hlo.fly(env, G[name + "_actions"], int(G[name + "_set_latency_at"]), float(G[name + "_set_latency"]))


def closed_form(f, actions, H, agg, freeze_at=-1, slip=None):
    """the rule of include/pds_history_latency.h on the oracle's own H = 2 rows (f: what history_latency_oracle.fly logged): shift
    and append; at step j <= H of an episode, where floor(j agg / B) > floor((j - 1) agg / B), the action columns of the slots
    0 .. H - j become the raw action; restart behind a finished episode.  set_latency: no rewrite until the next reset.  `slip`
    names one deliberate mistake."""
    half = f["row0"].shape[0] // 2
    restart = lambda row: np.concatenate([row[:half]] * (H - 1) + [row[half:]]).reshape(H, half)  # noqa: E731
    stack, j, out = restart(f["row0"]), 0, []
    for t, a in enumerate(actions):
        j = H + 1 if t == freeze_at else j + 1 if j <= H else j
        stack = np.concatenate([stack[1:], f["rows"][t][None, half:]])
        B, done = int(f["buf_size"][t]), bool(f["terminated"][t] or f["truncated"][t])
        jj = j - 1 if slip == "keyed on j - 1" else j
        top = H - jj + {"one slot fewer": 0, "one slot more": 2}.get(slip, 1)
        if 1 <= jj <= H and (jj * agg) // B > ((jj - 1) * agg) // B and not (slip == "final history left out" and done):
            stack[:min(top, H), half - 4:] = np.clip(a, -1, 1) if slip == "clipped action" else a
        out.append(stack.reshape(-1).copy())
        if done:
            stack, j = restart(f["reset_rows"][t]), 0
    return np.array(out)


@pytest.mark.parametrize("name", NAMES)
def test_the_wrapper_reproduces_the_reference_trajectories(name):
    """reset, the recorded actions, a reset behind every finished episode (and the recorded set_latency call), every history,
    reward, flag, cost and buf_size of the reference, at the float64 oracle's bar"""
    env, f = _fly_fixture(name)
    T = G[name + "_actions"].shape[0]
    assert f["obs"].shape == G[name + "_obs"].shape == (T, int(G[name + "_H"]) * env.half)
    gu.assert_close(f["obs0"], G[name + "_obs0"], RTOL, ATOL, f"{name} reset obs")
    assert np.array_equal(f["terminated"], G[name + "_terminated"]) and np.array_equal(f["truncated"], G[name + "_truncated"])
    assert np.array_equal(f["buf_size"], G[name + "_buf_size"]) and np.array_equal(f["cost"], G[name + "_cost"])
    worst = float(np.abs(f["obs"] - G[name + "_obs"]).max())
    print(f"{name}: max distance of a history {worst:.3e}, {int((f['terminated'] | f['truncated']).sum())} episodes ended")
    gu.assert_close(f["obs"], G[name + "_obs"], RTOL, ATOL, f"{name} obs")
    gu.assert_close(f["reset_obs"], G[name + "_reset_obs"], RTOL, ATOL, f"{name} reset obs behind an episode")
    gu.assert_close(f["reward"], G[name + "_reward"], RTOL, ATOL * 10, f"{name} reward")


@pytest.mark.parametrize("name", NAMES)
def test_the_closed_form_rule_is_the_wrapper_exactly(name):
    """the rule on the oracle's rows gives the wrapper's histories bit for bit on every trajectory of the fixture, the set_latency
    freeze included -- two statements that share nothing but the oracle's rows (the wrapper reads the ring, the rule counts steps)"""
    env, f = _fly_fixture(name)
    got = closed_form(f, G[name + "_actions"], int(G[name + "_H"]), int(G[name + "_agg"]), int(G[name + "_set_latency_at"]))
    assert np.array_equal(got, f["obs"]), np.argwhere(got != f["obs"])[:4]
    if name.endswith("set015"):  # the freeze is visible: without it the rule disagrees
        loose = closed_form(f, G[name + "_actions"], int(G[name + "_H"]), int(G[name + "_agg"]), -1)
        assert np.abs(loose - f["obs"]).max() > 1e-3


# two flights on the oracle whose episodes end INSIDE the first H steps (limit 5 under H = 8, limit 4 = H) and whose actions leave
# [-1, 1]: what the fixture's gentle flights do not do
TEETH = [("hover", 8, 0.015, 3, 5), ("hover", 4, 0.025, 1, 4)]
SLIPS = ["one slot fewer", "one slot more", "keyed on j - 1", "final history left out", "clipped action"]


@pytest.mark.parametrize("slip", SLIPS)
@pytest.mark.parametrize("task,H,latency,agg,limit", TEETH, ids=[f"h{c[1]}_limit{c[4]}" for c in TEETH])
def test_the_wrapper_catches_the_slip(task, H, latency, agg, limit, slip):
    """the rule with one deliberate mistake moves away from the wrapper by more than 100 bars (and without the mistake it is the
    wrapper exactly on these flights too)"""
    rs = np.random.RandomState(7)
    actions = -0.1 + 0.8 * rs.standard_normal((40, 4))
    assert (np.abs(actions) > 1).mean() > 0.1
    env = hlo.HistoryLatencyEnv(task, H, "f64", observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0.0,
                                enable_reset_distribution=0, use_latency=1, latency=latency, aggregate_phy_steps=agg,
                                max_episode_steps=limit)
    f = hlo.fly(env, actions)
    assert (f["terminated"] | f["truncated"]).sum() >= 40 // limit
    assert np.array_equal(closed_form(f, actions, H, agg), f["obs"])
    d = float(np.abs(closed_form(f, actions, H, agg, slip=slip) - f["obs"]).max())
    bar = ATOL + RTOL * float(np.abs(f["obs"]).max())
    print(f"TEETH H = {H}, limit {limit}, {slip}: moved {d:.3e} = {d / bar:.1e} bars")
    assert d > 100 * bar


def test_the_table_matches_the_header_and_the_library_exports_the_symbol(monkeypatch):
    """the rows of pds_history_advance_latency, pds_rollout_history_latency_supported and pds_rollout_history_latency against
    include/pds_history_latency.h, by the comparison of tests/test_host_cpu.py; include/pds.h does not declare them; the library
    exports them, `load` binds them and they refuse what the header says they refuse"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    name, query, rollout = "pds_history_advance_latency", "pds_rollout_history_latency_supported", "pds_rollout_history_latency"
    table = native.HISTORY_LATENCY_SIGNATURES
    assert list(table) == [name, query, rollout] and not set(table) & set(native.SIGNATURES)
    assert not any(re.search(rf"\b{n}\b", th._header()) for n in table)
    assert table[rollout] == native.SIGNATURES["pds_rollout_history"] and table[query] == native.SIGNATURES["pds_evaluate_history_supported"]

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_history_latency.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == 3 and not bad, bad
    restype, argtypes = table[name]
    plain = native.SIGNATURES["pds_history_advance"][1]
    assert argtypes[:11] == plain[:11] and argtypes[-1] == plain[-1] and len(argtypes) == len(plain) + 5
    _, bad = th._table_mismatches(dict(table, **{name: (restype, argtypes[:-1])}), native)
    assert bad == [f"{name}: 16 argtypes for 17 parameters"]
    lib = native.load()
    fn = getattr(lib, name)
    assert fn.argtypes == argtypes and fn.restype is restype
    assert fn(4, 21, 4, None, None, None, None, 1, None, None, None, None, None, None, 2, 1, None) == native.EINVAL  # (NULL arrays)
    assert getattr(lib, query)(None, 4) == native.EINVAL
    scalars = (C.c_int, C.c_int64, C.c_uint64, C.c_float)
    assert getattr(lib, rollout)(*[0 if t in scalars else None for t in table[rollout][1]]) == native.EINVAL  # (a NULL handle)


def test_the_four_units_are_built_and_every_unit_on_disk_is_listed():
    import glob
    from phoenix_drone_simulation_amd import build
    want = {f"pds_rollout_hist_{v}_lat.hip" for v in ("hover", "circle", "hover_pid", "circle_pid")}
    assert want <= set(build._UNITS) and len(build._UNITS) == len(set(build._UNITS))
    on_disk = {os.path.basename(f) for f in glob.glob(os.path.join(os.path.dirname(build.__file__), "csrc", "*.hip"))}
    assert on_disk == set(build._UNITS)
