"""The host side of the population evaluation for actors with three and four hidden layers (no GPU): the rows of
native.EVALUATE_DEEP_SIGNATURES against their declarations in include/pds_evaluate_deep.h (include/pds.h and native.SIGNATURES are
pinned entry for entry by tests/test_host_cpu.py, so the entry points stand beside them), the library's exports, the six
translation units in build._UNITS, PolicyPopulation at depth 3 and 4 -- its parameter count against torch, the row layout through
policy(p) and back, its refusals -- a population with two hidden layers as it was, and the plan of evaluate_population for a deep
population on stand-in envs."""
import ctypes as C
import os
import re
import types

import pytest
import torch
import torch.nn as nn

NAMES = ["pds_evaluate_deep_supported", "pds_evaluate_policies_deep"]
P = 4096  # stands for a device pointer: every call below is refused before anything reads it


def test_the_table_matches_the_header_and_the_library_exports_the_symbols(monkeypatch):
    """by the comparison of tests/test_host_cpu.py (its _table_mismatches, reading this header); a row that lost an argument, or
    holds a wrong class, must not pass; include/pds.h and native.SIGNATURES still agree without the symbols"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.EVALUATE_DEEP_SIGNATURES
    assert list(table) == NAMES and not set(table) & set(native.SIGNATURES)
    n, bad = th._table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) and not bad, bad
    assert not any(name in th._header() for name in NAMES)  # include/pds.h does not declare the new names

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_evaluate_deep.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == len(NAMES) and not bad, bad
    restype, argtypes = table["pds_evaluate_policies_deep"]
    metrics = native.SIGNATURES["pds_evaluate_policies_metrics"][1]
    assert argtypes[:3] == metrics[:3] and argtypes[3] is C.c_void_p and argtypes[4:] == metrics[4:]  # ..._metrics' row behind the struct
    _, bad = th._table_mismatches(dict(table, pds_evaluate_policies_deep=(restype, argtypes[:-1])), native)
    assert bad == ["pds_evaluate_policies_deep: 14 argtypes for 15 parameters"]
    wrong = list(argtypes); wrong[1] = C.c_int  # P is an int64_t
    _, bad = th._table_mismatches(dict(table, pds_evaluate_policies_deep=(restype, wrong)), native)
    assert len(bad) == 1 and "argument 1" in bad[0]
    _, bad = th._table_mismatches({k: table[k] for k in NAMES[1:]}, native)
    assert len(bad) == 1 and bad[0].startswith("names")
    lib = native.load()
    for name in NAMES:
        assert hasattr(lib, name), f"libpds_hip.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.argtypes == table[name][1] and fn.restype is table[name][0]


def test_the_units_and_headers_are_in_the_build():
    from phoenix_drone_simulation_amd import build
    want = {f"pds_evaluate_deep_{task}_l{L}.hip" for task in ("hover", "circle", "takeoff") for L in (3, 4)}
    assert len(want) == 6 and want <= set(build._UNITS) and len(build._UNITS) == len(set(build._UNITS))
    on_disk = {f for f in os.listdir(build._CSRC) if f.startswith("pds_evaluate_deep") and f.endswith(".hip")}
    assert on_disk == want
    assert {"pds_evaluate_deep.h", "pds_evaluate_deep_args.h"} <= set(build._HEADERS)
    assert any(os.path.normpath(d).endswith(os.path.join("include", "pds_evaluate_deep.h")) for d in build._DEPS)
    for f in want | {"pds_evaluate_deep.h", "pds_evaluate_deep_args.h"}:
        assert os.path.exists(os.path.join(build._CSRC, f)), f
    for task in ("hover", "circle", "takeoff"):
        for L in (3, 4):
            with open(os.path.join(build._CSRC, f"pds_evaluate_deep_{task}_l{L}.hip")) as f:
                text = f.read()
            assert f"PDS_EVALUATE_DEEP_UNIT(launch_evaluate_deep_{task}_l{L}, PDS_TASK_{task.upper()}, {L})" in text
    with open(os.path.join(build._CSRC, "pds_evaluate_deep.h")) as f:
        text = f.read()
    # the env wave is evaluate_kernel's statement macros, the network pass the function pds_mlp_deep_forward runs
    for macro in ("PDS_EVAL_WAVE_ACCUMULATORS", "PDS_EVAL_STEP_HEAD", "PDS_EM_STEP", "PDS_EVAL_RECORD_STEP", "PDS_EVAL_STILL",
                  "PDS_EVAL_STEP_TAIL", "PDS_EVAL_WAVE_END", "PDS_EM_INIT", "PDS_EM_STORE"):
        assert macro in text and f"#define {macro}" not in text, macro
    assert "deep_forward<0, L, false>" in text and "deep_forward<1, L, false>" in text and "deep_stage<L, kRolloutThreads>" in text


def test_a_null_handle_or_shape_is_einval_before_any_device_call():
    """the pointers are made up and no test here has a device (nor, without one, a handle: pds_create needs the device): a call
    that got as far as a launch would not return this code.  The other PDS_EINVALs need a handle:
    tests/test_gpu_evaluate_deep.py test_every_einval_of_the_call_leaves_the_handle_as_it_was"""
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    m = native.mlp_deep(34, (50, 30, 20), 4, "relu", base=P)
    assert lib.pds_evaluate_deep_supported(None, C.byref(m)) == native.EINVAL
    assert lib.pds_evaluate_deep_supported(None, None) == native.EINVAL
    assert lib.pds_evaluate_policies_deep(None, 2, 64, C.byref(m), P, None, None, 1e-5, 5, P, P, P, P, None, None) == native.EINVAL
    assert lib.pds_evaluate_policies_deep(None, 2, 64, None, None, None, None, 1e-5, 0, None, None, None, None, None, None) == native.EINVAL


def _sequential(d_in, hidden, activation, seed, identity=True):
    torch.manual_seed(seed)
    sizes = [d_in, *hidden, 4]
    mods = []
    for j in range(len(sizes) - 1):
        mods.append(nn.Linear(sizes[j], sizes[j + 1]))
        if j < len(sizes) - 2:
            mods.append({"relu": nn.ReLU, "tanh": nn.Tanh}[activation]())
    return nn.Sequential(*mods, *([nn.Identity()] if identity else []))


@pytest.mark.parametrize("hidden,activation", [((50, 30, 20), "relu"), ((32, 32, 32, 32), "tanh"), ((1, 1, 1), "tanh"), ((64, 1, 64, 1), "relu")])
def test_a_deep_population_constructs_and_round_trips(hidden, activation):
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, _actor_shape, _flat_params
    d = 34
    nets = [_sequential(d, hidden, activation, s, identity=bool(s % 2)) for s in range(3)]
    count = sum(p.numel() for p in nets[0].parameters())
    theta = torch.stack([torch.cat([p.detach().reshape(-1) for p in n.parameters()]) for n in nets])  # torch's parameter order
    pop = PolicyPopulation.from_flat(theta, d, hidden, activation)
    assert pop.deep and pop.P == 3 and pop.param_count == count == theta.shape[1] and pop.hidden_sizes == tuple(hidden)
    assert torch.equal(pop.theta, theta)
    assert native.load().pds_mlp_deep_param_count(C.byref(pop.mlp(0))) == count
    for n in nets:
        assert _actor_shape(n) == (d, tuple(hidden), 4, activation) and torch.equal(_flat_params(n), theta[nets.index(n)])
    x = torch.randn(7, d)
    for p, n in enumerate(nets):
        back = pop.policy(p)
        assert _actor_shape(back) == (d, tuple(hidden), 4, activation) and isinstance(back[-1], nn.Identity)
        with torch.no_grad():
            assert torch.equal(back(x), n(x))
    again = PolicyPopulation._from_nets([pop.policy(p) for p in range(3)], [None] * 3, [None] * 3, [None] * 3)
    assert torch.equal(again.theta, theta) and again.hidden_sizes == tuple(hidden) and again.activation == activation and again.deep
    # mlp(p): a struct pds_mlp_deep whose pointers walk row p in torch order
    m = pop.mlp(2)
    assert isinstance(m, native.MlpDeep) and m.n_hidden == len(hidden) and list(m.hidden)[:len(hidden)] == list(hidden)
    assert (m.d_in, m.d_out, m.activation) == (d, 4, native.ACTIVATIONS[activation])
    off = pop.theta.data_ptr() + 4 * 2 * count
    for l, lin in enumerate(l for l in nets[0] if isinstance(l, nn.Linear)):
        assert m.w[l] == off
        off += 4 * lin.weight.numel()
        assert m.b[l] == off
        off += 4 * lin.bias.numel()
    moved = pop.to("cpu")
    assert moved is not pop and moved.deep and torch.equal(moved.theta, theta) and moved.param_count == count
    # with a standardisation, as from_json_policies / from_actor_critics hand it over
    mean, std = torch.randn(3, d), torch.rand(3, d) + 0.5
    js = [types.SimpleNamespace(net=n, mean=mean[i], std=std[i], eps=1e-4) for i, n in enumerate(nets)]
    jp = PolicyPopulation.from_json_policies(js)
    assert jp.deep and torch.equal(jp.theta, theta) and torch.equal(jp.mean, mean) and torch.equal(jp.std, std) and jp.eps == 1e-4
    acs = [types.SimpleNamespace(pi=types.SimpleNamespace(net=n), obs_oms=None) for n in nets]
    assert torch.equal(PolicyPopulation.from_actor_critics(acs).theta, theta)


def test_the_refusals_fire():
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, _actor_shape
    d = 34
    count = lambda hidden: sum(b * a + b for a, b in zip((d,) + hidden, hidden + (4,)))
    for hidden in ((50,), (8, 8, 8, 8, 8), ()):  # depth 1, 5 and 0
        with pytest.raises(ValueError, match="hidden layers"):
            PolicyPopulation.from_flat(torch.zeros(2, count(hidden)), d, hidden, "relu")
    for hidden in ((50, 65, 20), (64, 64, 64, 65), (50, 0, 20)):  # a width above 64, or none
        with pytest.raises(ValueError, match="width"):
            PolicyPopulation.from_flat(torch.zeros(2, count(hidden)), d, hidden, "relu")
    with pytest.raises(ValueError, match="theta"):
        PolicyPopulation.from_flat(torch.zeros(2, count((50, 30, 20)) - 1), d, (50, 30, 20), "relu")
    with pytest.raises(ValueError, match="activation"):
        PolicyPopulation.from_flat(torch.zeros(2, count((50, 30, 20))), d, (50, 30, 20), "softplus")
    with pytest.raises(ValueError):
        _actor_shape(_sequential(d, (50,), "relu", 0))
    with pytest.raises(ValueError):
        _actor_shape(_sequential(d, (8, 8, 8, 8, 8), "relu", 0))
    with pytest.raises(ValueError):  # two activation types
        _actor_shape(nn.Sequential(nn.Linear(d, 8), nn.ReLU(), nn.Linear(8, 8), nn.Tanh(), nn.Linear(8, 8), nn.ReLU(), nn.Linear(8, 4)))
    with pytest.raises(ValueError, match="activation"):
        _actor_shape(nn.Sequential(nn.Linear(d, 8), nn.ELU(), nn.Linear(8, 8), nn.ELU(), nn.Linear(8, 8), nn.ELU(), nn.Linear(8, 4)))
    a, b = _sequential(d, (50, 30, 20), "relu", 0), _sequential(d, (50, 20, 30), "relu", 1)
    for other in (b, _sequential(d, (50, 30), "relu", 2), _sequential(d, (50, 30, 20), "tanh", 3), _sequential(d, (50, 30, 20, 20), "relu", 4)):
        with pytest.raises(ValueError, match="mixed"):
            PolicyPopulation._from_nets([a, other], [None] * 2, [None] * 2, [None] * 2)


def test_a_population_with_two_hidden_layers_is_what_it_was():
    """theta, param_count and mlp() by the statements the class had: h1 d + h1 + h2 h1 + h2 + 4 h2 + 4 floats a row, struct pds_mlp
    with its six pointers laid out from the row's address; widths above 64 still construct (the library refuses them)"""
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    d, h1, h2 = 34, 50, 50
    n = h1 * d + h1 + h2 * h1 + h2 + 4 * h2 + 4
    torch.manual_seed(0)
    theta = torch.randn(3, n)
    pop = PolicyPopulation.from_flat(theta, d, (h1, h2), "relu")
    assert not pop.deep and pop.param_count == n and torch.equal(pop.theta, theta) and pop.hidden_sizes == (h1, h2)
    m = pop.mlp(1)
    assert isinstance(m, native.Mlp) and (m.d_in, m.h1, m.h2, m.d_out, m.activation) == (d, h1, h2, 4, 0)
    base = pop.theta.data_ptr() + 4 * n
    want = [base]
    for k in (h1 * d, h1, h2 * h1, h2, 4 * h2):
        want.append(want[-1] + 4 * k)
    assert [m.w1, m.b1, m.w2, m.b2, m.w3, m.b3] == want
    net = pop.policy(0)
    assert [type(l) for l in net] == [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear, nn.Identity]
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in net.parameters()]), theta[0])
    wide = PolicyPopulation.from_flat(torch.zeros(1, 100 * d + 100 + 100 * 100 + 100 + 4 * 100 + 4), d, (100, 100), "tanh")
    assert wide.param_count == 100 * d + 100 + 100 * 100 + 100 + 4 * 100 + 4


# ---- the plan of evaluate_population (stand-in envs: nothing is flown) ----------------------------------------------------------
class _Lib:
    def __init__(self, deep, two=1):
        self.deep, self.two, self.asked = deep, two, []

    def pds_evaluate_deep_supported(self, handle, shape):
        self.asked.append("deep")
        return self.deep

    def pds_evaluate_supported(self, handle):
        self.asked.append("two")
        return self.two


def _env(deep_built, history=2, obs_dim=34, n=2 * 64):
    return types.SimpleNamespace(num_envs=n, obs_dim=obs_dim, _max_episode_steps=20, observation_history_size=history, _handle=None,
                                 lib=_Lib(1 if deep_built else 0))


def _deep_pop(d=34, hidden=(50, 30, 20)):
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    n = sum(b * a + b for a, b in zip((d,) + hidden, hidden + (4,)))
    return PolicyPopulation.from_flat(torch.zeros(2, n), d, hidden, "relu")


def _plan(env, pop, fused, **kw):
    from phoenix_drone_simulation_amd.evaluation import _plan_population
    a = dict(max_steps=None, metrics=False, obs_stats=False, history_fused=False, record=None, record_limit_bytes=1 << 30)
    a.update(kw)
    return _plan_population(env, pop, fused, a["max_steps"], a["metrics"], a["obs_stats"], a["history_fused"], a["record"], a["record_limit_bytes"])


def test_the_plan_of_a_deep_population():
    from phoenix_drone_simulation_amd.evaluation import fused_deep_evaluation_built
    pop = _deep_pop()
    built, not_built = _env(True), _env(False)
    assert fused_deep_evaluation_built(built, pop) and not fused_deep_evaluation_built(not_built, pop)
    for kw, form in ((dict(), "plain"), (dict(metrics=True), "metrics")):
        assert _plan(built, pop, "auto", **kw)[4:] == (form, True, None) and _plan(built, pop, True, **kw)[4:] == (form, True, None)
        assert _plan(built, pop, False, **kw)[4:] == (form, False, None)
        assert _plan(not_built, pop, "auto", **kw)[4:] == (form, False, None)
        with pytest.raises(NotImplementedError):
            _plan(not_built, pop, True, **kw)
    for kw, form in ((dict(obs_stats=True), "stats"), (dict(record=64), "record"), (dict(metrics=True, record=64), "record")):
        assert _plan(built, pop, "auto", **kw)[4:] == (form, False, None) and _plan(built, pop, False, **kw)[4:] == (form, False, None)
        with pytest.raises(NotImplementedError):
            _plan(built, pop, True, **kw)
    # the question of the two-hidden-layer kernel is never asked for a deep population, and the history keywords change nothing
    assert "two" not in built.lib.asked and "two" not in not_built.lib.asked
    assert _plan(built, pop, "auto", history_fused=True)[4:] == ("plain", True, None)
    # an observation history: no path at these depths, whatever `fused` says
    hist = _env(True, history=4, obs_dim=68)
    wide = _deep_pop(d=68)
    assert not fused_deep_evaluation_built(hist, wide)
    for fused in (True, "auto", False):
        with pytest.raises(NotImplementedError, match="64 inputs"):
            _plan(hist, wide, fused)
    # the checks in front of the plan are the ones every population meets
    with pytest.raises(ValueError, match="inputs"):
        _plan(_env(True, obs_dim=40), pop, "auto")
    with pytest.raises(ValueError, match="multiple of 64"):
        _plan(_env(True, n=2 * 32), pop, "auto")
    # a population with two hidden layers asks its own question only
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation
    two = PolicyPopulation.from_flat(torch.zeros(2, 50 * 34 + 50 + 50 * 50 + 50 + 4 * 50 + 4), 34, (50, 50), "relu")
    env = _env(True)
    assert not fused_deep_evaluation_built(env, two) and _plan(env, two, "auto")[4:] == ("plain", True, None) and env.lib.asked == ["two"]


def test_the_deep_guard_of_native_call_admits_the_table(monkeypatch):
    """an object that carries a struct pds_mlp_deep (fused.FusedMLP with deep=True) passes native.call into the entry points of
    EVALUATE_DEEP_SIGNATURES, and is still refused by an entry point that reads a struct pds_mlp"""
    from phoenix_drone_simulation_amd import native
    seen = {}

    class Carrier:
        deep, n_hidden = True, 3
        md = native.mlp_deep(34, (50, 30, 20), 4, "relu", base=P)

        def _bind(self):
            seen["bound"] = True

    stub = types.SimpleNamespace(pds_evaluate_policies_deep=lambda *a: seen.setdefault("args", a) and 0,
                                 pds_evaluate_policies_metrics=lambda *a: 0)
    monkeypatch.setattr(native, "load", lambda: stub)
    native.call("pds_evaluate_policies_deep", None, 2, 64, Carrier())
    assert seen["bound"] and len(seen["args"]) == 4
    with pytest.raises(NotImplementedError, match="2 hidden layers"):
        native.call("pds_evaluate_policies_metrics", None, 2, 64, Carrier())
