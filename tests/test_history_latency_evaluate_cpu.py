"""The host side of the one-launch evaluation of observation-history policies on the latency ring (no GPU): the five rows of
native.HISTORY_LATENCY_EVALUATE_SIGNATURES against include/pds_history_latency_evaluate.h, the translation units in build._UNITS,
the plan of evaluate_population with and without the new keyword on a stand-in env, and the float64 reference flight of
tests/flight_latency_oracle.py: its float32 run pinned to its float64 run, its histories equal to the closed-form rule restated
open loop, and every slip a kernel could make shown to move the recorded observation by more than 100 bars."""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flight_latency_oracle as flo
import flight_oracle as fo

QUERIES = ["pds_evaluate_history_latency_supported", "pds_evaluate_history_latency_stats_supported"]
CALLS = ["pds_evaluate_policies_history_latency", "pds_evaluate_policies_history_latency_record", "pds_evaluate_policies_history_latency_stats"]
BAR_UNITS = 4.0  # the bar of tests/test_gpu_evaluate_forms_reference.py


# ---- header, table, library, units -------------------------------------------------------------------------------------------------
def test_the_table_matches_the_header_and_the_library_exports_the_symbols(monkeypatch):
    """the five rows against include/pds_history_latency_evaluate.h by the comparison of tests/test_host_cpu.py; a row that lost an
    argument must not pass; include/pds.h and include/pds_history_latency.h do not declare the names and the other tables do not
    hold them; the library exports them, `load` binds them, and they answer a NULL handle PDS_EINVAL"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.HISTORY_LATENCY_EVALUATE_SIGNATURES
    assert list(table) == QUERIES + CALLS
    for other in (native.SIGNATURES, native.HISTORY_RECORD_SIGNATURES, native.HISTORY_STATS_SIGNATURES, native.HISTORY_LATENCY_SIGNATURES,
                  native.COLLECT_CONTROL_SIGNATURES):
        assert not set(table) & set(other)
    for header in ("pds.h", "pds_history_latency.h", "pds_history_record.h", "pds_history_stats.h"):
        text = open(os.path.join(th.ROOT, "include", header)).read()
        assert not any(re.search(rf"\b{n}\b", text) for n in table), header
    n, bad = th._table_mismatches(native.SIGNATURES, native)  # (include/pds.h and its table still agree)
    assert n == len(native.SIGNATURES) and not bad, bad

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_history_latency_evaluate.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == 5 and not bad, bad
    # the argument lists of the three non-latency twins
    assert table[CALLS[0]] == native.SIGNATURES["pds_evaluate_policies_history"]
    assert table[CALLS[1]] == native.HISTORY_RECORD_SIGNATURES["pds_evaluate_policies_history_record"]
    assert table[CALLS[2]] == native.HISTORY_STATS_SIGNATURES["pds_evaluate_policies_history_stats"]
    assert table[QUERIES[0]] == table[QUERIES[1]] == native.SIGNATURES["pds_evaluate_history_supported"]
    restype, argtypes = table[CALLS[1]]
    _, bad = th._table_mismatches(dict(table, **{CALLS[1]: (restype, argtypes[:-1])}), native)
    assert bad == [f"{CALLS[1]}: {len(argtypes) - 1} argtypes for {len(argtypes)} parameters"]
    wrong = list(argtypes); wrong[1] = C.c_int64  # history is an int
    _, bad = th._table_mismatches(dict(table, **{CALLS[1]: (restype, wrong)}), native)
    assert len(bad) == 1 and "argument 1" in bad[0]
    lib = native.load()
    scalars = (C.c_int, C.c_int64, C.c_uint64, C.c_float)
    for name in QUERIES + CALLS:
        fn = getattr(lib, name)
        assert fn.argtypes == table[name][1] and fn.restype is table[name][0]
        assert fn(*[0 if t in scalars else None for t in table[name][1]]) == native.EINVAL, name  # (a NULL handle)


def test_the_twelve_units_are_built_and_every_unit_on_disk_is_listed():
    from phoenix_drone_simulation_amd import build
    tasks = ("hover", "circle", "hover_pid", "circle_pid")
    want = {f"pds_evaluate_hist_{v}_lat.hip" for v in tasks} | {f"pds_evaluate_hist_lat_{f}_{v}.hip" for f in ("record", "stats") for v in tasks}
    assert len(want) == 12 and want <= set(build._UNITS) and len(build._UNITS) == len(set(build._UNITS))
    on_disk = {os.path.basename(f) for f in glob.glob(os.path.join(build._CSRC, "*.hip"))}
    assert on_disk == set(build._UNITS)
    assert {f for f in on_disk if f.startswith("pds_evaluate_hist_") and re.search(r"_lat(_|\.hip$)", f)} == want
    for unit in want:  # each mirrors a unit of the history rollout on the ring
        task = re.sub(r"pds_evaluate_hist_(lat_(record|stats)_)?|_lat\.hip$|\.hip$", "", unit)
        assert os.path.exists(os.path.join(build._CSRC, f"pds_rollout_hist_{task}_lat.hip")), unit
    assert any(d.endswith("pds_history_latency_evaluate.h") for d in build._DEPS)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
HALF, H = 17, 4


class _Env:  # what the plan reads of an env, with a history of four halves
    num_envs, obs_dim, _max_episode_steps, observation_history_size = 256, H * HALF, 500, H


def _pop(d_in=H * HALF):
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    n = 8 * d_in + 8 + 8 * 8 + 8 + 4 * 8 + 4
    return PolicyPopulation.from_flat(torch.zeros(2, n), d_in, (8, 8), "tanh")


def _patched(monkeypatch, answers):
    """the five predicates answer from `answers` (absent: False) and say that they were asked"""
    from phoenix_drone_simulation_amd import evaluation
    asked = []
    for key, name in (("history", "fused_history_evaluation_built"), ("history_stats", "fused_history_stats_evaluation_built"),
                      ("standard", "fused_evaluation_built"), ("latency", "fused_history_latency_evaluation_built"),
                      ("latency_stats", "fused_history_latency_stats_evaluation_built")):
        monkeypatch.setattr(evaluation, name, lambda env, key=key: asked.append(key) or answers.get(key, False))
    return evaluation, asked


_CALLS = [dict(fused=f, metrics=m, obs_stats=o, history_fused=hf, record=r, history_stats_fused=hs)
          for f in (True, False, "auto") for m in (False, True) for o in (False, True) for hf in (False, True) for r in (None, 64)
          for hs in (False, True)]


@pytest.mark.parametrize("on_the_ring", [False, True], ids=["no_ring", "ring"])
def test_with_the_keyword_at_its_default_the_plan_is_what_it_was(monkeypatch, on_the_ring):
    """a table of 96 calls: _plan_population_call -- whose signature is what it was -- and the plan evaluate_population makes with
    history_latency_fused left out or False return the same tuple or raise the same error, and never ask the new predicates,
    whether the env is on the ring (the old predicates answer False) or not"""
    answers = dict(latency=True, latency_stats=True) if on_the_ring else dict(history=True, history_stats=True, latency=False)
    ev, asked = _patched(monkeypatch, answers)
    assert list(inspect.signature(ev._plan_population_call).parameters)[-1] == "history_stats_fused"

    def run(fn, kw, **more):
        try:
            return fn(_Env(), _pop(), kw["fused"], None, kw["metrics"], kw["obs_stats"], kw["history_fused"], kw["record"], 1 << 30,
                      kw["history_stats_fused"], **more)
        except (NotImplementedError, ValueError) as e:
            return type(e), str(e)

    kernels = 0
    for kw in _CALLS:
        old = run(ev._plan_population_call, kw)
        assert run(ev._plan_population, kw) == old and run(ev._plan_population, kw, history_latency_fused=False) == old, kw
        kernels += isinstance(old[0], int) and bool(old[5])
    assert not {"latency", "latency_stats"} & set(asked)
    assert kernels == (0 if on_the_ring else 20)


def test_the_keyword_plans_the_latency_forms(monkeypatch):
    ev, asked = _patched(monkeypatch, dict(latency=True, latency_stats=True))
    plan = lambda **kw: ev._plan_population(_Env(), _pop(), kw.get("fused", True), None, kw.get("metrics", False), kw.get("obs_stats", False),  # noqa: E731
                                            kw.get("history_fused", True), kw.get("record"), 1 << 30, kw.get("history_stats_fused", False),
                                            kw.get("history_latency_fused", True))
    assert plan() == (2, 128, 500, None, "plain", True, H) and asked == ["history", "latency"]
    assert plan(metrics=True)[4:] == ("metrics", True, H) and plan(record=64)[3:] == (64, "record", True, H)
    del asked[:]
    assert plan(obs_stats=True, history_stats_fused=True)[4:] == ("stats", True, H) and asked == ["history_stats", "latency_stats"]
    # obs_stats without history_stats_fused stays composed, as without the ring
    assert plan(obs_stats=True, fused="auto")[4:] == ("stats", False, H)
    with pytest.raises(NotImplementedError, match="pds_evaluate_policies_history"):
        plan(obs_stats=True)
    # without history_fused the keyword changes nothing
    with pytest.raises(NotImplementedError, match="observation_history_size 2"):
        plan(history_fused=False)
    assert plan(fused=False)[5:] == (False, H)
    # where no latency kernel is built: True raises, "auto" runs the composed path
    ev, asked = _patched(monkeypatch, {})
    with pytest.raises(NotImplementedError, match="pds_evaluate_policies_history"):
        plan()
    assert plan(fused="auto")[5:] == (False, H) and asked == ["history", "latency", "history", "latency"]
    for value in (1, 0, "auto", None):
        with pytest.raises(ValueError, match="history_latency_fused"):
            plan(history_latency_fused=value)


def test_the_keyword_is_opt_in_everywhere():
    from phoenix_drone_simulation_amd import es, evaluation
    ps = inspect.signature(evaluation.evaluate_population).parameters
    assert ps["history_latency_fused"].default is False and ps["history_latency_fused"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(es.ESTrainer.__init__).parameters["history_latency_fused"].default is False
    assert inspect.signature(evaluation._plan_population).parameters["history_latency_fused"].default is False


def test_the_predicates_answer_false_without_asking_the_library():
    """an env without history_latency, and one whose views set_latency froze: False, the handle not looked at"""
    from phoenix_drone_simulation_amd import evaluation as ev

    class Lib:
        def __getattr__(self, name):
            raise AssertionError(f"the library was asked: {name}")

    class Env:
        lib, _handle, observation_history_size, history_latency, _hist_frozen = Lib(), None, 4, False, False

    for fn in (ev.fused_history_latency_evaluation_built, ev.fused_history_latency_stats_evaluation_built):
        env = Env()
        assert fn(env) is False
        env.history_latency, env._hist_frozen = True, True
        assert fn(env) is False


# ---- the reference flight -----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_rings_the_rule_distinguishes():
    """rings of 1, 2 and 3 rows, 1 and 2 sub-steps, H = 1; and one case whose condition holds at some but not all j <= H"""
    seen = set()
    for name in flo.CASES:
        fl = flo.flight(flo.case(name), "f64")
        assert (fl["buf_size"], fl["agg"]) == flo.RING[name]
        seen.add((fl["buf_size"], fl["agg"], fl["history"]))
    assert {b for b, _, _ in seen} == {1, 2, 3} and {a for _, a, _ in seen} == {1, 2} and 1 in {h for _, _, h in seen}
    partial = [(B, agg, Hc) for B, agg, Hc in seen if 0 < sum(j * agg // B > (j - 1) * agg // B for j in range(1, Hc + 1)) < Hc]
    assert (3, 2, 4) in partial  # j = 1: 2 // 3 = 0 (off), j = 2: 4 // 3 = 1 (on), j = 3: 2 (on), j = 4: 8 // 3 = 2 (off)


@pytest.mark.parametrize("name", flo.CASES)
def test_the_float32_flight_agrees_with_the_float64_flight_on_every_length(name):
    """the actor seeds are chosen so: no env is left out of any comparison.  Both endings occur -- episodes that terminate and
    episodes the TimeLimit cuts -- and envs go on into a second episode inside the flight"""
    case = flo.case(name)
    f32, f64 = flo.flight(case, "f32"), flo.flight(case, "f64")
    assert np.array_equal(f32["length"], f64["length"]) and fo.agreeing(case).all()
    assert np.array_equal(f32["done_all"], f64["done_all"])
    L = f64["length"]
    assert L.min() >= 1 and L.max() == case.limit < case.max_steps
    if name == "hover_lean_h6_b2":  # (its policy 0 crashes: terminations before the TimeLimit, at steps that differ)
        assert (L[0] < case.limit).all() and len(np.unique(L[0])) > 1 and (L[1] == case.limit).all()


@pytest.mark.parametrize("name", flo.CASES)
def test_the_float32_flight_is_pinned_to_the_float64_flight(name):
    """every unit is the float32 flight's own distance from the float64 flight, floored at the float32 rounding of the group's
    magnitude: the float32 flight is within 1 unit by construction, and the units stay small against the quantities -- 1e-4 of
    the group's largest magnitude (float32 dynamics over at most 14 steps)"""
    case = flo.case(name)
    f32, f64, units = flo.flight(case, "f32"), flo.flight(case, "f64"), flo.units_of(case)
    T = case.max_steps
    for g, sl in fo.GROUPS.items():
        top = np.abs(f64["state"][..., sl]).max()
        assert np.abs(f32["state"][..., sl] - f64["state"][..., sl]).max() <= units[g] <= max(1e-4 * top, 2.0 ** -23 * top), (g, units[g], top)
    for g in ("action", "observation", "u0"):
        top = np.abs(f64[g]).max()
        assert np.abs(f32[g] - f64[g]).max() <= units[g] <= 1e-4 * top, (g, units[g], top)
    for j in fo.EM_SUMS:
        top = np.abs(f64["metrics"][..., j]).max()
        assert np.abs(f32["metrics"][..., j] - f64["metrics"][..., j]).max() <= units[fo.EM[j]] <= max(1e-4, (T + 4) * 2.0 ** -24) * max(top, 1.0)
    assert np.array_equal(f32["metrics"][..., list(fo.EM_INTEGER)], f64["metrics"][..., list(fo.EM_INTEGER)])
    assert np.array_equal(f32["ret"] != 0, f64["ret"] != 0) and np.abs(f32["ret"] - f64["ret"]).max() <= 1e-4 * np.abs(f64["ret"]).max()
    assert np.array_equal(f32["cost"], f64["cost"])


def _histories(fl, case, slip=None):
    P, E = case.P, case.E
    N = P * E
    B, agg = fl["buf_size"], fl["agg"]
    stacks = flo.restack(fl["rows0"], fl["rows_all"], fl["done_all"], fl["action_all"].reshape(N, case.max_steps, 4), case.history, B, agg, slip)
    return stacks.transpose(1, 0, 2).reshape(P, E, case.max_steps, -1)


@pytest.mark.parametrize("name", flo.CASES)
def test_the_views_give_what_the_closed_form_rule_gives(name):
    """the histories HistoryLatencyEnv returned, every step of every env whatever episode it is in, are the closed-form rule's over
    the same rows and actions, exactly: the rule the kernel implements is the reference's mechanism"""
    case = flo.case(name)
    for precision in ("f64", "f32"):
        fl = flo.flight(case, precision)
        assert np.array_equal(_histories(fl, case), fl["observation_all"]), precision


def test_every_slip_a_kernel_could_make_would_show():
    """no rule at all, the clipped action for the raw one, j off by one, one slot too many, one too few: each moves the recorded
    observation of the float64 flight by more than 100 bars (a bar = 4 units of `observation`) in at least one case, over the
    recorded steps (s < length) alone.  And "the rule always on" -- no_rule's opposite -- shows on the ring of 3 rows with 2
    sub-steps, whose condition fails at j = 1 and j = 4."""
    worst = {slip: 0.0 for slip in flo.SLIPS}
    for name in flo.CASES:
        case = flo.case(name)
        fl, units = flo.flight(case, "f64"), flo.units_of(case)
        on = (np.arange(case.max_steps)[None, None, :] < fl["length"][:, :, None])[..., None]
        bar = BAR_UNITS * units["observation"]
        for slip in flo.SLIPS:
            moved = float(np.abs(np.where(on, _histories(fl, case, slip), 0) - fl["observation"]).max()) / bar
            worst[slip] = max(worst[slip], moved)
    print("bars moved:", {k: round(v, 1) for k, v in worst.items()})
    assert all(v > 100 for v in worst.values()), worst
    case = flo.case("hover_lean_motor_h4_b3_agg2")
    fl, units = flo.flight(case, "f64"), flo.units_of(case)
    N = case.N
    always = flo.restack(fl["rows0"], fl["rows_all"], fl["done_all"], fl["action_all"].reshape(N, case.max_steps, 4), case.history, 1, 1)
    always = always.transpose(1, 0, 2).reshape(case.P, case.E, case.max_steps, -1)
    assert np.abs(always - fl["observation_all"]).max() > 100 * BAR_UNITS * units["observation"]
