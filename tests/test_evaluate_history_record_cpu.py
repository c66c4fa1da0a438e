"""The host side of the recorded flights of observation-history policies (no GPU): the new symbol's row in
native.HISTORY_RECORD_SIGNATURES against its declaration in include/pds_history_record.h (include/pds.h and native.SIGNATURES are
pinned entry for entry by tests/test_host_cpu.py, so the entry point stands beside them), the choice of path of
evaluation._plan_population_call on a stand-in env with observation_history_size 4, and the translation units of the record form
of evaluate_hist_kernel in build._UNITS."""
import ctypes as C
import glob
import os
import re

import pytest
import torch

NAME = "pds_evaluate_policies_history_record"
HALF, H = 17, 4  # Hover with observation noise: 17 per half, 68 network inputs


def test_the_table_matches_the_header_and_the_library_exports_the_symbol(monkeypatch):
    """the row of pds_evaluate_policies_history_record against include/pds_history_record.h, by the comparison of
    tests/test_host_cpu.py (its _table_mismatches, reading this header); a row that lost an argument, or holds a wrong class, must
    not pass; include/pds.h and native.SIGNATURES still agree without the symbol; the library exports it, `load` binds it and it
    refuses a NULL handle"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.HISTORY_RECORD_SIGNATURES
    assert list(table) == [NAME] and NAME not in native.SIGNATURES
    n, bad = th._table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) and not bad, bad

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_history_record.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == 1 and not bad, bad
    restype, argtypes = table[NAME]
    assert len(argtypes) == 19
    _, bad = th._table_mismatches({NAME: (restype, argtypes[:-1])}, native)
    assert bad == [f"{NAME}: 18 argtypes for 19 parameters"]
    wrong = list(argtypes); wrong[15] = C.c_int  # record_per_policy is an int64_t
    _, bad = th._table_mismatches({NAME: (restype, wrong)}, native)
    assert len(bad) == 1 and "argument 15" in bad[0]
    _, bad = th._table_mismatches({}, native)
    assert len(bad) == 1 and bad[0].startswith("names")
    # the history entry point's arguments, then those the record form adds to the metrics entry point, then the stream
    history = native.SIGNATURES["pds_evaluate_policies_history"][1]
    record = native.SIGNATURES["pds_evaluate_policies_record"][1]
    assert argtypes[:15] == history[:15] and argtypes[15:] == record[14:]
    lib = native.load()
    fn = getattr(lib, NAME)
    assert fn.argtypes == argtypes and fn.restype is restype
    assert fn(None, 4, 1, 64, None, None, None, None, 0.0, 1, None, None, None, None, None, 64, None, None, None) == native.EINVAL


class _Env:  # what _plan_population_call reads of an env, with a history of four halves
    num_envs, obs_dim, _max_episode_steps, observation_history_size = 256, H * HALF, 500, H


def _pop(d_in=H * HALF):
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    n = 8 * d_in + 8 + 8 * 8 + 8 + 4 * 8 + 4
    return PolicyPopulation.from_flat(torch.zeros(2, n), d_in, (8, 8), "tanh")


def _plan(monkeypatch, built=True, **kw):
    from phoenix_drone_simulation_amd import evaluation
    asked = []
    monkeypatch.setattr(evaluation, "fused_history_evaluation_built", lambda env: asked.append("history") or built)
    monkeypatch.setattr(evaluation, "fused_evaluation_built", lambda env: asked.append("standard") or False)
    args = dict(fused=True, max_steps=None, metrics=False, obs_stats=False, history_fused=False, record=None, record_limit_bytes=1 << 30)
    args.update(kw)
    out = evaluation._plan_population_call(_Env(), _pop(), args["fused"], args["max_steps"], args["metrics"], args["obs_stats"],
                                           args["history_fused"], args["record"], args["record_limit_bytes"])
    return out, asked


def test_history_fused_with_a_record_plans_the_history_kernel(monkeypatch):
    (P, E, T, R, form, use_kernel, h), asked = _plan(monkeypatch, history_fused=True, record=64)
    assert (P, E, T, R, form, use_kernel, h) == (2, 128, 500, 64, "record", True, H) and asked == ["history"]
    (*_, form, use_kernel, h), _ = _plan(monkeypatch, history_fused=True, record=128, metrics=True, fused="auto")
    assert (form, use_kernel, h) == ("record", True, H)
    # where the library has no kernel: "auto" flies the composed path, True raises
    (*_, form, use_kernel, h), _ = _plan(monkeypatch, built=False, history_fused=True, record=64, fused="auto")
    assert (form, use_kernel) == ("record", False)
    with pytest.raises(NotImplementedError, match="pds_evaluate_policies_history"):
        _plan(monkeypatch, built=False, history_fused=True, record=64)


def test_without_history_fused_the_plan_is_what_it_was(monkeypatch):
    """the default: a history env has no kernel under fused=True (NotImplementedError) and flies the composed path under "auto"
    and False, with a record or without"""
    for record in (None, 64):
        with pytest.raises(NotImplementedError, match="observation_history_size 2"):
            _plan(monkeypatch, record=record)
        (P, E, T, R, form, use_kernel, h), asked = _plan(monkeypatch, record=record, fused="auto")
        assert (R, form, use_kernel, h) == (record, "record" if record else "plain", False, None) and asked == ["standard"]
        (*_, use_kernel, h), asked = _plan(monkeypatch, record=record, fused=False)
        assert (use_kernel, h) == (False, None) and asked == []


def test_record_with_obs_stats_still_raises(monkeypatch):
    with pytest.raises(ValueError, match="obs_stats"):
        _plan(monkeypatch, history_fused=True, record=64, obs_stats=True)


def test_the_record_limit_counts_the_whole_history(monkeypatch):
    """record_limit_bytes against max_steps x P x R x (64 + 4 H half): the recorded observation is the history"""
    need = 500 * 2 * 128 * (64 + 4 * H * HALF)
    (*_, form, use_kernel, h), _ = _plan(monkeypatch, history_fused=True, record=128, record_limit_bytes=need)
    assert (form, use_kernel, h) == ("record", True, H)
    with pytest.raises(ValueError, match="record_limit_bytes"):
        _plan(monkeypatch, history_fused=True, record=128, record_limit_bytes=need - 1)
    assert need > 500 * 2 * 128 * (64 + 4 * 2 * HALF)  # (what a limit computed from one row of the env would have let through)


def test_the_five_units_are_built_and_every_unit_on_disk_is_listed():
    from phoenix_drone_simulation_amd import build
    want = {f"pds_evaluate_hist_record_{v}.hip" for v in ("hover", "circle", "takeoff", "hover_pid", "circle_pid")}
    assert want <= set(build._UNITS) and len(build._UNITS) == len(set(build._UNITS))
    on_disk = {os.path.basename(f) for f in glob.glob(os.path.join(build._CSRC, "pds_evaluate_hist_record_*.hip"))}
    assert on_disk == want
    for unit in want:
        assert os.path.exists(os.path.join(build._CSRC, unit.replace("_record", ""))), unit  # each mirrors a unit of the history launch
