"""The host side of the stats and the record form of the population evaluation for actors with three and four hidden layers (no
GPU): the rows of native.EVALUATE_DEEP_FORMS_SIGNATURES against their declarations in include/pds_evaluate_deep_forms.h (by the
comparison of tests/test_evaluate_deep_cpu.py), the library's exports, the twelve translation units in build._UNITS, the plan of
evaluate_population(..., deep_forms_fused=True) on stand-in envs, the constructor checks of ESTrainer at depth 3 and 4, and the
float32 / float64 agreement of tests/flight_deep_oracle.py that tests/test_gpu_evaluate_deep_forms.py rests its bars on."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import evaluate_oracle as eo
import flight_deep_oracle as fdo
import flight_oracle as fo

NAMES = ["pds_evaluate_deep_forms_supported", "pds_evaluate_policies_deep_stats", "pds_evaluate_policies_deep_record"]
P = 4096  # stands for a device pointer: every call below is refused before anything reads it
UNITS = {f"pds_evaluate_{form}_deep_{task}_l{L}.hip" for form in ("stats", "record") for task in ("hover", "circle", "takeoff") for L in (3, 4)}


def test_the_table_matches_the_header_and_the_library_exports_the_symbols(monkeypatch):
    """a row that lost an argument, or holds a wrong class, must not pass; the new names are in neither pinned table"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.EVALUATE_DEEP_FORMS_SIGNATURES
    assert list(table) == NAMES
    assert not set(table) & set(native.SIGNATURES) and not set(table) & set(native.EVALUATE_DEEP_SIGNATURES)
    assert not any(name in th._header() for name in NAMES)  # include/pds.h does not declare the new names
    deep_header = open(os.path.join(th.ROOT, "include", "pds_evaluate_deep.h")).read()
    assert not any(name in deep_header for name in NAMES)  # nor does the pinned header of the plain / metrics call

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_evaluate_deep_forms.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == len(NAMES) and not bad, bad
    deep = native.EVALUATE_DEEP_SIGNATURES["pds_evaluate_policies_deep"][1]
    stats, record = table["pds_evaluate_policies_deep_stats"][1], table["pds_evaluate_policies_deep_record"][1]
    # pds_evaluate_policies_deep's row with d_obs_sums / record_per_policy, d_flight, d_obs_rec in front of the stream
    assert stats == deep[:-1] + [C.c_void_p, C.c_void_p] and record == deep[:-1] + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    assert stats[4:] == native.SIGNATURES["pds_evaluate_policies_stats"][1][4:]
    assert record[4:] == native.SIGNATURES["pds_evaluate_policies_record"][1][4:]
    restype = table["pds_evaluate_policies_deep_stats"][0]
    _, bad = th._table_mismatches(dict(table, pds_evaluate_policies_deep_stats=(restype, stats[:-1])), native)
    assert bad == ["pds_evaluate_policies_deep_stats: 15 argtypes for 16 parameters"]
    wrong = list(record); wrong[14] = C.c_int  # record_per_policy is an int64_t
    _, bad = th._table_mismatches(dict(table, pds_evaluate_policies_deep_record=(restype, wrong)), native)
    assert len(bad) == 1 and "argument 14" in bad[0]
    _, bad = th._table_mismatches({k: table[k] for k in NAMES[1:]}, native)
    assert len(bad) == 1 and bad[0].startswith("names")
    assert (native.EVALUATE_DEEP_FORM_STATS, native.EVALUATE_DEEP_FORM_RECORD) == (0, 1)
    assert re.search(r"#define\s+PDS_EVALUATE_DEEP_FORM_STATS\s+0\b", header()) and re.search(r"#define\s+PDS_EVALUATE_DEEP_FORM_RECORD\s+1\b", header())
    lib = native.load()
    for name in NAMES:
        assert hasattr(lib, name), f"libpds_hip.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.argtypes == table[name][1] and fn.restype is table[name][0]


def test_the_twelve_units_and_headers_are_in_the_build():
    from phoenix_drone_simulation_amd import build
    assert len(UNITS) == 12 and UNITS <= set(build._UNITS) and len(build._UNITS) == len(set(build._UNITS))
    on_disk = {f for f in os.listdir(build._CSRC) if re.match(r"pds_evaluate_(stats|record)_deep_", f)}
    assert on_disk == UNITS
    assert "pds_evaluate_deep_forms_args.h" in build._HEADERS and os.path.exists(os.path.join(build._CSRC, "pds_evaluate_deep_forms_args.h"))
    assert any(os.path.normpath(d).endswith(os.path.join("include", "pds_evaluate_deep_forms.h")) for d in build._DEPS)
    for form in ("stats", "record"):
        for task in ("hover", "circle", "takeoff"):
            for L in (3, 4):
                with open(os.path.join(build._CSRC, f"pds_evaluate_{form}_deep_{task}_l{L}.hip")) as f:
                    text = f.read()
                assert (f"PDS_EVALUATE_DEEP_FORM_UNIT(launch_evaluate_{form}_deep_{task}_l{L}, PDS_TASK_{task.upper()}, {L}, "
                        f"EvalForm::{form.capitalize()})") in text
    with open(os.path.join(build._CSRC, "pds_evaluate_deep.h")) as f:
        text = f.read()
    # the forms are stated with what csrc/pds_evaluate.h states, not a second time
    for piece in ("es_lds<1>()", "es_tree_add", "eval_record_column", "PDS_ER_STEP", "EsSums<NIN", "eval_keeps_alive_mask(F)"):
        assert piece in text, piece
    for restated in ("#define PDS_ER_STEP", "es_tree_add(float", "eval_record_column(const"):
        assert restated not in text, restated
    with open(os.path.join(build._CSRC, "pds_evaluate_deep_forms_args.h")) as f:
        args = f.read()
    assert "static_assert(sizeof(EvalDeepStatsArgs) ==" in args and "static_assert(sizeof(EvalDeepRecordArgs) ==" in args
    with open(os.path.join(build._CSRC, "pds_evaluate_deep_args.h")) as f:
        assert "sizeof(EvalDeepArgs) == 848" in f.read()  # (left alone)


def test_a_null_handle_shape_or_an_unknown_form_is_einval_before_any_device_call():
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    m = native.mlp_deep(34, (50, 30, 20), 4, "relu", base=P)
    for form in (0, 1):
        assert lib.pds_evaluate_deep_forms_supported(None, C.byref(m), form) == native.EINVAL
    assert lib.pds_evaluate_deep_forms_supported(None, None, 0) == native.EINVAL
    assert lib.pds_evaluate_policies_deep_stats(None, 2, 64, C.byref(m), P, None, None, 1e-5, 5, P, P, P, P, None, P, None) == native.EINVAL
    assert lib.pds_evaluate_policies_deep_record(None, 2, 64, C.byref(m), P, None, None, 1e-5, 5, P, P, P, P, None, 64, P, None, None) == native.EINVAL


# ---- the plan of evaluate_population (stand-in envs: nothing is flown) ----------------------------------------------------------
class _Lib:
    def __init__(self, deep, forms):
        self.deep, self.forms, self.asked = deep, forms, []

    def pds_evaluate_deep_supported(self, handle, shape):
        self.asked.append("deep")
        return self.deep

    def pds_evaluate_deep_forms_supported(self, handle, shape, form):
        self.asked.append(("forms", form))
        return self.forms

    def pds_evaluate_supported(self, handle):
        self.asked.append("two")
        return 1


def _env(forms_built, deep_built=True, history=2):
    return types.SimpleNamespace(num_envs=2 * 64, obs_dim=34, _max_episode_steps=20, observation_history_size=history, _handle=None,
                                 lib=_Lib(1 if deep_built else 0, 1 if forms_built else 0))


def _plan(env, pop, fused, deep_forms_fused=None, **kw):
    from phoenix_drone_simulation_amd.evaluation import _plan_population
    a = dict(max_steps=None, metrics=False, obs_stats=False, history_fused=False, record=None, record_limit_bytes=1 << 30)
    a.update(kw)
    extra = {} if deep_forms_fused is None else dict(deep_forms_fused=deep_forms_fused)
    return _plan_population(env, pop, fused, a["max_steps"], a["metrics"], a["obs_stats"], a["history_fused"], a["record"], a["record_limit_bytes"],
                            **extra)


FORMS = ((dict(obs_stats=True), "stats", 0), (dict(record=64), "record", 1), (dict(metrics=True, record=64), "record", 1))


def test_the_plan_without_the_keyword_is_what_it_was():
    from test_evaluate_deep_cpu import _deep_pop
    pop = _deep_pop()
    for keyword in (None, False):
        env = _env(True)
        for kw, form, _ in FORMS:
            assert _plan(env, pop, "auto", keyword, **kw)[4:] == (form, False, None) and _plan(env, pop, False, keyword, **kw)[4:] == (form, False, None)
            with pytest.raises(NotImplementedError):
                _plan(env, pop, True, keyword, **kw)
        assert not any(isinstance(a, tuple) for a in env.lib.asked)  # the new question is not asked
        for kw, form in ((dict(), "plain"), (dict(metrics=True), "metrics")):
            assert _plan(env, pop, "auto", keyword, **kw)[4:] == (form, True, None)


def test_the_plan_with_the_keyword():
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, fused_deep_forms_evaluation_built
    from test_evaluate_deep_cpu import _deep_pop
    pop = _deep_pop()
    built, not_built = _env(True), _env(False)
    for kw, form, code in FORMS:
        assert fused_deep_forms_evaluation_built(built, pop, form) and not fused_deep_forms_evaluation_built(not_built, pop, form)
        assert built.lib.asked[-1] == ("forms", code)
        assert _plan(built, pop, "auto", True, **kw)[4:] == (form, True, None) and _plan(built, pop, True, True, **kw)[4:] == (form, True, None)
        assert _plan(built, pop, False, True, **kw)[4:] == (form, False, None)
        assert _plan(not_built, pop, "auto", True, **kw)[4:] == (form, False, None)
        with pytest.raises(NotImplementedError):
            _plan(not_built, pop, True, True, **kw)
    # the plain and the metrics call go the way they went, whatever the new question would answer
    for kw, form in ((dict(), "plain"), (dict(metrics=True), "metrics")):
        assert _plan(not_built, pop, True, True, **kw)[4:] == (form, True, None)
    with pytest.raises(ValueError, match="deep_forms_fused"):
        _plan(built, pop, "auto", "yes", obs_stats=True)
    with pytest.raises(ValueError, match="form"):
        fused_deep_forms_evaluation_built(built, pop, "metrics")
    # record_limit_bytes raises before anything is asked or allocated
    env = _env(True)
    with pytest.raises(ValueError, match="record_limit_bytes"):
        _plan(env, pop, True, True, record=64, record_limit_bytes=1000)
    assert env.lib.asked == []
    # an observation history: no path at these depths
    hist = _env(True, history=4)
    assert not fused_deep_forms_evaluation_built(hist, pop, "stats")
    # a population with two hidden layers: the keyword changes nothing, the new question is not asked
    two = PolicyPopulation.from_flat(torch.zeros(2, 50 * 34 + 50 + 50 * 50 + 50 + 4 * 50 + 4), 34, (50, 50), "relu")
    env = _env(True)
    assert not fused_deep_forms_evaluation_built(env, two, "stats") and env.lib.asked == []
    assert _plan(env, two, "auto", True, obs_stats=True)[4:] == ("stats", True, None) and env.lib.asked == ["two"]


def test_the_kernel_call_of_each_form(monkeypatch):
    """_fly_kernel hands a deep population's stats / record flight to the new entry points: d_metrics, then what the form adds;
    record_observations=False arrives as a NULL d_obs_rec"""
    from phoenix_drone_simulation_amd import evaluation
    from test_evaluate_deep_cpu import _deep_pop
    pop = _deep_pop()
    seen = []
    monkeypatch.setattr(evaluation.native, "call", lambda name, *a, **k: seen.append((name, a)))
    env = types.SimpleNamespace(device="cpu", num_envs=2 * 64, _handle=None)
    obs = torch.zeros(128, 34)
    flight, obs_rec = torch.zeros(5, 4, 128, 4), torch.zeros(5, 128, 34)
    out = evaluation._fly_kernel(env, pop, obs, 2, 64, 5, "stats", None, None)
    assert seen[-1][0] == "pds_evaluate_policies_deep_stats" and len(seen[-1][1]) == 15
    assert seen[-1][1][-1] is out[4] and tuple(out[4].shape) == (2, 4, 2, 64) and seen[-1][1][-2] is out[3]
    for rec, want in (((None, 64, flight, obs_rec), obs_rec), ((None, 64, flight, None), None)):
        out = evaluation._fly_kernel(env, pop, obs, 2, 64, 5, "record", None, rec)
        name, a = seen[-1]
        assert name == "pds_evaluate_policies_deep_record" and len(a) == 17 and a[-3] == 64 and a[-2] is flight and a[-1] is want and a[-4] is out[3]
    evaluation._fly_kernel(env, pop, obs, 2, 64, 5, "metrics", None, None)
    assert seen[-1][0] == "pds_evaluate_policies_deep" and len(seen[-1][1]) == 14


# ---- ESTrainer at depth 3 and 4: what needs no device ----------------------------------------------------------------------------
def _stub_env(history=2, n=128):
    return types.SimpleNamespace(num_envs=n, obs_dim=34, act_dim=4, device=torch.device("cpu"), observation_history_size=history)


def test_the_trainer_refuses_shapes_outside_the_range():
    from phoenix_drone_simulation_amd.es import ESTrainer
    for hidden in ((50,), (8, 8, 8, 8, 8), ()):
        with pytest.raises(ValueError, match="2 to 4 hidden layers"):
            ESTrainer(_stub_env(), 2, hidden_sizes=hidden)
    for hidden in ((50, 65, 20), (64, 64, 64, 65), (50, 0, 20)):
        with pytest.raises(ValueError, match="1 to 64"):
            ESTrainer(_stub_env(), 2, hidden_sizes=hidden)
    for hidden in ((5, 7, 3), (4, 4, 4, 4)):
        with pytest.raises(ValueError, match="observation_history_size 2 only"):
            ESTrainer(_stub_env(history=4), 2, hidden_sizes=hidden)


@pytest.mark.parametrize("hidden", [(5, 7, 3), (4, 4, 4, 4), (50, 30, 20), (32, 32, 32, 32)])
def test_the_deep_centre_is_one_flat_row_in_the_deep_layout(hidden):
    """constructed on CPU tensors (nothing is launched): `mu` holds W1 b1 .. W(L+1) b(L+1), the actor's parameters are views
    into it, the struct pds_mlp_deep points at them, and the row is what PolicyPopulation.from_flat takes"""
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.es import ESTrainer
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, _flat_params
    tr = ESTrainer(_stub_env(), 2, hidden_sizes=hidden, activation="tanh", fused=False, deep_forms_fused=True)
    assert tr.deep and tr.deep_forms_fused and tr.hidden_sizes == hidden
    assert tr.n == fdo.param_count((34,) + hidden + (4,)) == native.load().pds_mlp_deep_param_count(C.byref(tr._mlp))
    assert isinstance(tr._mlp, native.MlpDeep) and tr._mlp.n_hidden == len(hidden)
    assert torch.equal(_flat_params(tr.ac.pi.net), tr.mu)
    off = tr.mu.data_ptr()
    lin = [l for l in tr.ac.pi.net if isinstance(l, torch.nn.Linear)]
    assert len(lin) == len(hidden) + 1
    for l, layer in enumerate(lin):
        assert layer.weight.data_ptr() == off == tr._mlp.w[l]
        off += 4 * layer.weight.numel()
        assert layer.bias.data_ptr() == off == tr._mlp.b[l]
        off += 4 * layer.bias.numel()
    pop = PolicyPopulation.from_flat(tr.mu.unsqueeze(0), 34, hidden, "tanh")
    assert pop.deep and pop.param_count == tr.n
    two = ESTrainer(_stub_env(), 2, hidden_sizes=(5, 7), fused=False)  # two hidden layers: struct pds_mlp, as before
    assert not two.deep and isinstance(two._mlp, native.Mlp)


# ---- the reference the GPU test's bars rest on -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fdo.DEEP_CASES)
def test_the_oracle_flights_agree_and_the_units_are_usable(name):
    """float32 against float64 flight of every case: the lengths differ in at most length_cap(N) envs -- the cap check() applies,
    asserted on the reference alone, so that the GPU test's exclusion cannot hide a failure --, also among the recorded first 64
    envs of a policy; the units of the sums and of the record's groups are finite and positive"""
    c = fdo.deep_case(name)
    f32, f64 = fdo.flight(c, "f32"), fdo.flight(c, "f64")
    disagree = f32["length"] != f64["length"]
    cap = eo.length_cap(c.N)
    print(f"{name}: {int(disagree.sum())} of {c.N} envs disagree in length (cap {cap}); {int(disagree[:, :64].sum())} among the recorded")
    assert int(disagree.sum()) <= cap and int(disagree[:, :64].sum()) <= cap
    assert int((~(~disagree).reshape(-1, 16).all(axis=1)).sum()) <= cap  # the 16-env parts of the slab that hold such an env
    units = fdo.units_of(c)
    for k in ("part_sum_d", "part_sum_d2", "action", "observation", "u0") + tuple(fo.GROUPS):
        print(f"UNIT {name} {k} {units[k]:.3e}")
        assert np.isfinite(units[k]) and units[k] > 0, k
    for k in ("sum_d", "sum_d2", "state", "action", "observation"):
        assert np.isfinite(f64[k]).all() and np.isfinite(f32[k]).all(), k
