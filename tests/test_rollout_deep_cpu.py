"""The host side of the one-launch rollout for actors with three and four hidden layers (no GPU): the rows of
native.ROLLOUT_DEEP_SIGNATURES against their declarations in include/pds_rollout_deep.h (include/pds.h and native.SIGNATURES are
pinned entry for entry by tests/test_host_cpu.py, so the entry points stand beside them), the library's exports, the six
translation units in build._UNITS, the pieces the kernel reuses and does not restate, the NULL refusals, the deep guard of
native.call, and the --deep-rollout flag of examples/train_ppo.py under every --alg."""
import ctypes as C
import importlib.util
import os
import re
import types

import pytest

NAMES = ["pds_rollout_deep_supported", "pds_rollout_deep"]
P = 4096  # stands for a device pointer: every call below is refused before anything reads it


def test_the_table_matches_the_header_and_the_library_exports_the_symbols(monkeypatch):
    """by the comparison of tests/test_host_cpu.py (its _table_mismatches, reading this header); a row that lost an argument, or
    holds a wrong class, must not pass; include/pds.h and native.SIGNATURES still agree without the symbols"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.ROLLOUT_DEEP_SIGNATURES
    assert list(table) == NAMES and not set(table) & set(native.SIGNATURES)
    n, bad = th._table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) and not bad, bad
    assert not any(name in th._header() for name in NAMES)  # include/pds.h does not declare the new names

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_rollout_deep.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == len(NAMES) and not bad, bad
    restype, argtypes = table["pds_rollout_deep"]
    hist = native.SIGNATURES["pds_rollout_history"][1]
    # pds_rollout_history's row without `history` and with the struct pds_mlp_deep pointer
    assert len(argtypes) == len(hist) - 1 == 25 and argtypes[:2] == hist[:2] and argtypes[2] is C.c_void_p and argtypes[3:] == hist[4:]
    _, bad = th._table_mismatches(dict(table, pds_rollout_deep=(restype, argtypes[:-1])), native)
    assert bad == ["pds_rollout_deep: 24 argtypes for 25 parameters"]
    wrong = list(argtypes); wrong[7] = C.c_int  # seed is a uint64_t
    _, bad = th._table_mismatches(dict(table, pds_rollout_deep=(restype, wrong)), native)
    assert len(bad) == 1 and "argument 7" in bad[0]
    _, bad = th._table_mismatches({k: table[k] for k in NAMES[1:]}, native)
    assert len(bad) == 1 and bad[0].startswith("names")
    lib = native.load()
    for name in NAMES:
        assert hasattr(lib, name), f"libpds_hip.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.argtypes == table[name][1] and fn.restype is table[name][0]


def test_the_units_and_headers_are_in_the_build():
    from phoenix_drone_simulation_amd import build
    want = {f"pds_rollout_deep_{task}_l{L}.hip" for task in ("hover", "circle", "takeoff") for L in (3, 4)}
    assert len(want) == 6 and want <= set(build._UNITS) and len(build._UNITS) == len(set(build._UNITS))
    assert set(build._UNITS[-6:]) == want  # appended
    on_disk = {f for f in os.listdir(build._CSRC) if f.startswith("pds_rollout_deep") and f.endswith(".hip")}
    assert on_disk == want
    assert {"pds_rollout_deep.h", "pds_rollout_deep_args.h"} <= set(build._HEADERS)
    assert any(os.path.normpath(d).endswith(os.path.join("include", "pds_rollout_deep.h")) for d in build._DEPS)
    for f in want | {"pds_rollout_deep.h", "pds_rollout_deep_args.h"}:
        assert os.path.exists(os.path.join(build._CSRC, f)), f
    for task in ("hover", "circle", "takeoff"):
        for L in (3, 4):
            with open(os.path.join(build._CSRC, f"pds_rollout_deep_{task}_l{L}.hip")) as f:
                text = f.read()
            assert f"PDS_ROLLOUT_DEEP_UNIT(launch_rollout_deep_{task}_l{L}, PDS_TASK_{task.upper()}, {L})" in text
    with open(os.path.join(build._CSRC, "pds_rollout_deep.h")) as f:
        text = f.read()
    # the env wave and the sampling are the statement macros of csrc/pds_rollout.h, the network pass the function
    # pds_mlp_deep_forward runs: used here, defined there
    for macro in ("PDS_ENV_WAVE_BEGIN", "PDS_OPAQUE_STEP_COPIES", "PDS_NEXT_TICK", "PDS_RECORD_STEP", "PDS_ENV_WAVE_END",
                  "PDS_DRAW_ACTION_NOISE", "PDS_EMIT_ACTION"):
        assert macro in text and f"#define {macro}" not in text, macro
    assert "deep_forward<0, L, false>" in text and "deep_forward<1, L, false>" in text and "deep_stage<L, kRolloutThreads>" in text
    # both loops run exactly T iterations and every wait has its post: two of each in the kernel, no stop protocol
    code = re.sub(r"//[^\n]*", "", text)
    assert code.count("for (int s = 0; s < T; ++s)") == 2
    assert code.count("rollout_wait_ge(") == 2 and code.count("rollout_post(") == 2 and "kEvalStop" not in code
    with open(os.path.join(build._CSRC, "pds_rollout_deep_args.h")) as f:
        args = f.read()
    assert "offsetof(RolloutDeepArgs, s) == 0" in args and "rollout_deep_variant_built" in args


def test_a_null_handle_or_actor_is_einval_before_any_device_call():
    """the pointers are made up and no test here has a device (nor, without one, a handle: pds_create needs the device): a call
    that got as far as a launch would not return this code.  The other PDS_EINVALs need a handle: tests/test_gpu_rollout_deep.py"""
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    m = native.mlp_deep(34, (50, 30, 20), 4, "relu", base=P)
    assert lib.pds_rollout_deep_supported(None, C.byref(m)) == native.EINVAL
    assert lib.pds_rollout_deep_supported(None, None) == native.EINVAL
    tail = [P] * 9 + [2] + [P] * 3 + [None]
    assert lib.pds_rollout_deep(None, 4, C.byref(m), None, None, 1e-5, P, 0, None, 0, 0, *tail) == native.EINVAL
    assert lib.pds_rollout_deep(None, 0, None, None, None, 1e-5, None, 0, None, 0, 0, *([None] * 9 + [0] + [None] * 4)) == native.EINVAL


def test_the_deep_guard_of_native_call_admits_the_table(monkeypatch):
    """an object that carries a struct pds_mlp_deep (fused.FusedMLP with deep=True) passes native.call into pds_rollout_deep, and is
    still refused by the one-launch rollouts that read a struct pds_mlp"""
    from phoenix_drone_simulation_amd import native
    seen = {}

    class Carrier:
        deep, n_hidden = True, 3
        md = native.mlp_deep(34, (50, 30, 20), 4, "relu", base=P)

        def _bind(self):
            seen["bound"] = True

    stub = types.SimpleNamespace(pds_rollout_deep=lambda *a: seen.setdefault("args", a) and 0,
                                 pds_rollout=lambda *a: 0, pds_rollout_history=lambda *a: 0)
    monkeypatch.setattr(native, "load", lambda: stub)
    native.call("pds_rollout_deep", None, 4, Carrier())
    assert seen["bound"] and len(seen["args"]) == 3
    for name in ("pds_rollout", "pds_rollout_history"):
        with pytest.raises(NotImplementedError, match="2 hidden layers"):
            native.call(name, None, 4, Carrier())


def test_rollout_deep_supported_asks_the_library_only_for_a_deep_actor_on_the_handles_own_row(monkeypatch):
    from phoenix_drone_simulation_amd import fused, native
    asked = []
    stub = types.SimpleNamespace(pds_rollout_deep_supported=lambda h, m: asked.append(h) or 1)
    monkeypatch.setattr(native, "load", lambda: stub)
    md = native.mlp_deep(34, (50, 30, 20), 4, "relu", base=P)
    deep, two = types.SimpleNamespace(deep=True, md=md), types.SimpleNamespace(deep=False)
    env = types.SimpleNamespace(_handle=7, observation_history_size=2)
    assert fused.rollout_deep_supported(env, deep) is True and asked == [7]
    assert fused.rollout_deep_supported(env, two) is False and asked == [7]
    assert fused.rollout_deep_supported(types.SimpleNamespace(_handle=7, observation_history_size=4), deep) is False and asked == [7]
    stub.pds_rollout_deep_supported = lambda h, m: 0
    assert fused.rollout_deep_supported(env, deep) is False
    with pytest.raises(NotImplementedError, match="rollout_deep_supported"):  # before any launch
        fused.fused_rollout_deep(env, deep, 4, *([None] * 19))


def _train_ppo():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "train_ppo.py")
    spec = importlib.util.spec_from_file_location("examples_train_ppo", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("alg", ["ppo", "npg", "trpo"])
def test_train_ppo_takes_deep_rollout_with_every_alg(alg):
    mod = _train_ppo()
    _, args = mod.parse_args(["--alg", alg, "--pi-hidden", "50", "30", "20", "--deep-rollout"])
    assert args.deep_rollout is True and args.alg == alg and args.deep_fused is False
    _, args = mod.parse_args(["--alg", alg])
    assert args.deep_rollout is False
    if alg != "ppo":  # the reference's architecture search entirely on fused kernels
        _, args = mod.parse_args(["--alg", alg, "--pi-hidden", "32", "32", "32", "32", "--deep-fused", "--deep-rollout"])
        assert args.deep_fused and args.deep_rollout
    else:
        with pytest.raises(SystemExit):
            mod.parse_args(["--alg", "ppo", "--deep-fused", "--deep-rollout"])
