"""The host side of the recorded flights (no GPU): evaluation.Flights on hand-made arrays -- episode(), pairs(), metrics(), the CSV
round trip through simopt.MiniTrajectories.from_csv_dir, mini_trajectories() against create_trajectory_slices -- the argument
refusals of evaluate_population(record=...) in front of any library call, and the new symbol's declaration."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

LENGTHS = [[60, 3, 0], [47, 41, 1]]  # P = 2, R = 3, T = 60: one full, short ones, an empty one, one just long enough for a slice


def _flights(D=5, control_mode="PWM", seed=0):
    """hand-made: random rows below each length, zeros from there on (what a record holds); actions beyond [-1, 1] among them"""
    from phoenix_drone_simulation_amd.evaluation import Flights
    g = torch.Generator().manual_seed(seed)
    P, R, T = 2, 3, 60
    length = torch.tensor(LENGTHS, dtype=torch.float32)
    on = (torch.arange(T).view(1, 1, T) < length.unsqueeze(-1)).unsqueeze(-1)
    state = torch.where(on, 0.3 * torch.randn(P, R, T, 12, generator=g), torch.zeros(()))
    action = torch.where(on, 0.8 * torch.randn(P, R, T, 4, generator=g), torch.zeros(()))
    obs = torch.where(on, torch.randn(P, R, T, D, generator=g), torch.zeros(()))
    u0 = 0.1 * torch.randn(P, R, 4, generator=g)
    return Flights(state, action, obs, length, 0.01, u0, control_mode=control_mode)


def test_episode_cuts_at_the_length():
    fl = _flights()
    assert (fl.P, fl.R) == (2, 3)
    for p in range(2):
        for e in range(3):
            L, ep = LENGTHS[p][e], fl.episode(p, e)
            assert tuple(ep["state"].shape) == (L, 12) and tuple(ep["action"].shape) == (L, 4) and tuple(ep["observation"].shape) == (L, 5)
            assert torch.equal(ep["state"], fl.state[p, e, :L]) and torch.equal(ep["action"], fl.action[p, e, :L])
            assert torch.equal(ep["observation"], fl.observation[p, e, :L])
            if L:
                assert bool((ep["state"] != 0).all())  # (nothing of the zero rows past the end)


def test_pairs_shapes_and_contents():
    from phoenix_drone_simulation_amd.evaluation import Flights
    fl = _flights()
    X, Y = fl.pairs()
    rows = sum(max(L - 1, 0) for row in LENGTHS for L in row)
    assert tuple(X.shape) == tuple(Y.shape) == (rows, 5) and X.dtype == torch.float32
    k = 0
    for p in range(2):
        for e in range(3):
            o = fl.observation[p, e]
            for s in range(LENGTHS[p][e] - 1):
                assert torch.equal(X[k], o[s]) and torch.equal(Y[k], o[s + 1])
                k += 1
    assert k == rows
    bare = Flights(fl.state, fl.action, None, fl.length, 0.01)
    assert bare.episode(0, 0)["observation"] is None
    with pytest.raises(ValueError, match="observations"):
        bare.pairs()


def test_metrics_is_metrics_from_arrays_per_episode():
    from phoenix_drone_simulation_amd.evaluation import METRIC_NAMES, metrics_from_arrays
    fl = _flights()
    lengths = [[60, 3, 5], [47, 41, 1]]  # (metrics_from_arrays takes flights of at least one row)
    fl.length = torch.tensor(lengths, dtype=torch.float32)
    m = fl.metrics()
    assert m.shape == (2, 3, len(METRIC_NAMES)) and m.dtype == np.float64
    for p in range(2):
        for e in range(3):
            L = lengths[p][e]
            x, a = fl.state[p, e, :L].numpy(), fl.action[p, e, :L].numpy()
            want = metrics_from_arrays(x[:, 6:9], x[:, 9:12], a, fl.last_action0[p, e].numpy())
            assert np.array_equal(m[p, e], want), (p, e)
    assert m[0, 0, 5] >= 1  # the hand-made actions saturate somewhere


def test_shapes_are_checked():
    from phoenix_drone_simulation_amd.evaluation import Flights
    z = torch.zeros
    with pytest.raises(ValueError):
        Flights(z(2, 3, 10, 11), z(2, 3, 10, 4), None, z(2, 3), 0.01)
    with pytest.raises(ValueError):
        Flights(z(2, 3, 10, 12), z(2, 3, 9, 4), None, z(2, 3), 0.01)
    with pytest.raises(ValueError):
        Flights(z(2, 3, 10, 12), z(2, 3, 10, 4), z(2, 3, 9, 5), z(2, 3), 0.01)
    with pytest.raises(ValueError):
        Flights(z(2, 3, 10, 12), z(2, 3, 10, 4), None, torch.full((2, 3), 11.0), 0.01)


def _slices(fl, T=35, pre_steps=5, skip=10):
    """create_trajectory_slices on each episode that is long enough, from the definition of the PWM the motors took"""
    from phoenix_drone_simulation_amd.simopt import MiniTrajectories
    parts = []
    for p in range(fl.P):
        for e in range(fl.R):
            L = int(fl.length[p, e])
            if L > T + pre_steps:
                pwm = (np.clip(fl.action[p, e, :L].double().numpy(), -1.0, 1.0) + 1.0) * 30000.0
                parts.append(MiniTrajectories.create_trajectory_slices(fl.state[p, e, :L].double().numpy(), pwm, T, pre_steps, skip))
    return [np.concatenate([part[k] for part in parts]) for k in range(3)]


def test_mini_trajectories_are_the_slices_of_each_episode_long_enough():
    fl = _flights()
    mt = fl.mini_trajectories()
    obs, acs, pre = _slices(fl)
    # L = 60: starts 5, 15; L = 47: 5; L = 41 (> 40): 5; the episodes of 3, 0 and 1 steps give none
    assert len(mt) == 4 and mt.mini_trajectory_size == 35 and mt.pre_steps == 5
    assert np.array_equal(mt.observations, obs) and np.array_equal(mt.actions, acs) and np.array_equal(mt.pre_inputs, pre)
    assert float(np.abs(mt.actions).max()) <= 1.0 and float(fl.action.abs().max()) > 1.0  # the clipped actions
    assert np.array_equal(mt.observations[0], fl.state[0, 0, 5:40].double().numpy())
    short = fl.mini_trajectories(T=10, pre_steps=2, skip=7)
    assert np.array_equal(short.observations, _slices(fl, 10, 2, 7)[0])
    with pytest.raises(ValueError, match="longer"):
        fl.mini_trajectories(T=58, pre_steps=5)
    with pytest.raises(ValueError, match="PWM"):
        _flights(control_mode="AttitudeRate").mini_trajectories()


def test_csv_round_trip(tmp_path):
    """to_csv_dir -> MiniTrajectories.from_csv_dir == mini_trajectories().  The states are float32 values written with repr() and
    read by pandas' default float parser, which is fast and not correctly rounded in float64: they must come back within 2^-24
    relative, half a float32 ulp, i.e. as the same float32 values the record holds.  The actions also go through the battery model
    and its inverse in float64 (a square root and a few products on values up to 65 535: 1e-9 absolute on actions of size 1 is
    far above their rounding and the parser's)."""
    pytest.importorskip("pandas")
    from phoenix_drone_simulation_amd.simopt import OBS_COLUMNS, PWM_COLUMNS, MiniTrajectories
    fl = _flights()
    files = fl.to_csv_dir(str(tmp_path / "logs"))
    assert len(files) == 6 and all(os.path.exists(f) for f in files)
    head = open(files[0]).readline().strip().split(",")
    assert head == OBS_COLUMNS + PWM_COLUMNS + ["bat"]
    assert len(open(files[0]).read().split()) == 1 + 60 and len(open(files[1]).read().split()) == 1 + 3
    back = MiniTrajectories.from_csv_dir(str(tmp_path / "logs"))
    want = fl.mini_trajectories()
    assert len(back) == len(want) == 4
    np.testing.assert_allclose(back.observations, want.observations, rtol=2.0 ** -24, atol=0)
    assert np.array_equal(back.observations.astype(np.float32), want.observations.astype(np.float32))
    np.testing.assert_allclose(back.actions, want.actions, rtol=0, atol=1e-9)
    np.testing.assert_allclose(back.pre_inputs, want.pre_inputs, rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="PWM"):
        _flights(control_mode="Attitude").to_csv_dir(str(tmp_path / "no"))
    assert not (tmp_path / "no").exists()


class _Env:  # what evaluate_population reads in front of its first call into the library: anything else is an AttributeError
    num_envs, obs_dim, _max_episode_steps = 256, 34, 500


@pytest.mark.parametrize("kw,match", [
    (dict(record=0), "multiple of 64"),
    (dict(record=63), "multiple of 64"),
    (dict(record=192), "multiple of 64"),  # R > E = 128
    (dict(record=64.5), "record"),
    (dict(record=64, obs_stats=True), "obs_stats"),
    (dict(record=128, record_limit_bytes=500 * 2 * 128 * (64 + 4 * 34) - 1), "record_limit_bytes"),
    (dict(record=128, max_steps=10 ** 6), "record_limit_bytes"),  # the default limit: 1 GiB
])
def test_record_arguments_are_refused_before_any_library_call(kw, match):
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    n = 8 * 34 + 8 + 8 * 8 + 8 + 4 * 8 + 4
    pop = PolicyPopulation.from_flat(torch.zeros(2, n), 34, (8, 8), "tanh")
    with pytest.raises(ValueError, match=match):
        evaluate_population(_Env(), pop, **kw)


def test_an_accepted_record_reaches_the_env():
    """the same stand-in with arguments that pass: the call goes on to ask the env (AttributeError here), at the byte limit too"""
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    n = 8 * 34 + 8 + 8 * 8 + 8 + 4 * 8 + 4
    pop = PolicyPopulation.from_flat(torch.zeros(2, n), 34, (8, 8), "tanh")
    with pytest.raises(AttributeError):
        evaluate_population(_Env(), pop, record=128, record_limit_bytes=500 * 2 * 128 * (64 + 4 * 34))


def test_the_record_table_matches_its_header_and_the_library_exports_the_symbol():
    """the row of pds_evaluate_policies_record in native.SIGNATURES against include/pds.h, by the comparison of tests/test_host_cpu.py;
    a row that lost an argument, or holds a wrong class, must not pass; the library exports the symbol and refuses a NULL handle"""
    from phoenix_drone_simulation_amd import native
    from test_host_cpu import _table_mismatches
    n, bad = _table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) and not bad, bad
    restype, argtypes = native.SIGNATURES["pds_evaluate_policies_record"]
    _, bad = _table_mismatches(dict(native.SIGNATURES, pds_evaluate_policies_record=(restype, argtypes[:-1])), native)
    assert bad == ["pds_evaluate_policies_record: 17 argtypes for 18 parameters"]
    wrong = list(argtypes); wrong[14] = C.c_int  # record_per_policy is an int64_t
    _, bad = _table_mismatches(dict(native.SIGNATURES, pds_evaluate_policies_record=(restype, wrong)), native)
    assert len(bad) == 1 and "argument 14" in bad[0]
    _, bad = _table_mismatches({}, native)
    assert len(bad) == 1 and bad[0].startswith("names")
    assert "pds_evaluate_policies_record" in native.SIGNATURES
    metrics = native.SIGNATURES["pds_evaluate_policies_metrics"][1]
    assert argtypes[:14] == metrics[:14] and argtypes[-1] is metrics[-1]  # the metrics entry point's arguments, the three new ones, the stream
    lib = native.load()
    assert lib.pds_evaluate_policies_record.argtypes == argtypes and lib.pds_evaluate_policies_record.restype is restype
    assert lib.pds_evaluate_policies_record(None, 1, 64, None, None, None, None, 0.0, 1, None, None, None, None, None, 64, None, None,
                                            None) == native.EINVAL
