"""Host side of the flight-quality metrics (phoenix_drone_simulation_amd.evaluation: metrics_from_arrays, FlightMetrics;
es.penalised_return; include/pds.h pds_evaluate_policies_metrics): the definitions on hand-made sequences, the units of the
derived table, the fitness formula, and the declaration / binding of the entry point.  No device."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("roll_sq", "pitch_sq", "rate_sq", "action_rate_sq", "tilt_max", "saturated_steps", "roll_rate_crossings",
         "pitch_rate_crossings")


def test_metric_names_are_the_header_s_enum_in_order():
    from phoenix_drone_simulation_amd.evaluation import METRIC_NAMES
    assert tuple(METRIC_NAMES) == NAMES
    hdr = open(os.path.join(ROOT, "include", "pds.h")).read()
    enum = re.findall(r"PDS_EM_([A-Z_]+) = (\d)", hdr)
    assert [(n.lower(), int(v)) for n, v in enum] == [(n, j) for j, n in enumerate(NAMES)]
    assert re.search(r"#define PDS_EVAL_METRICS 8\b", hdr)


def test_crossing_rule_counts_sign_changes_of_the_strict_less_than():
    """wx = [1, -1, 1, 0, -0.0, -1]: (x < 0) is F T F F F T -- a zero of either sign is not negative -- so 3 changes"""
    from phoenix_drone_simulation_amd.evaluation import metrics_from_arrays
    wx = np.array([1.0, -1.0, 1.0, 0.0, -0.0, -1.0])
    L = len(wx)
    omega = np.stack([wx, np.ones(L), np.zeros(L)], axis=1)
    m = metrics_from_arrays(np.zeros((L, 3)), omega, np.zeros((L, 4)), np.zeros(4))
    assert m.dtype == np.float64 and m.shape == (8,)
    assert m[6] == 3 and m[7] == 0
    assert m[2] == 4 + L  # sum of wx^2 + wy^2 + wz^2


def test_sums_action_rate_and_saturation_on_a_hand_made_flight():
    from phoenix_drone_simulation_amd.evaluation import metrics_from_arrays
    rpy = np.array([[0.1, -0.2, 3.0], [-0.3, 0.1, 3.0], [0.2, 0.25, 3.0]])
    omega = np.array([[1.0, -2.0, 0.5], [-1.0, -2.0, 0.5], [-1.0, 2.0, 0.5]])
    actions = np.array([[0.5, 0.5, 0.5, 0.5], [1.5, 0.5, 0.5, 0.5], [1.0, -1.0, 0.5, -1.25]])
    u0 = np.array([0.25, 0.5, 0.5, 0.5])
    m = metrics_from_arrays(rpy, omega, actions, u0)
    assert m[0] == pytest.approx(0.01 + 0.09 + 0.04, rel=1e-15)
    assert m[1] == pytest.approx(0.04 + 0.01 + 0.0625, rel=1e-15)
    assert m[2] == pytest.approx(3 * (1 + 4 + 0.25), rel=1e-15)
    # d(0) = a(0) - u0, d(s) = a(s) - a(s - 1)
    assert m[3] == pytest.approx(0.0625 + 1.0 + (0.25 + 2.25 + 0.0 + 1.75 ** 2), rel=1e-15)
    assert m[4] == 0.3           # the yaw column does not count
    assert m[5] == 2             # 1.5 and -1.25 exceed 1; exactly 1.0 and -1.0 do not
    assert m[6] == 1 and m[7] == 1


def test_tilt_max_passes_over_a_nan_in_the_middle():
    from phoenix_drone_simulation_amd.evaluation import metrics_from_arrays
    rpy = np.array([[0.1, 0.05, 0.0], [np.nan, 0.2, 0.0], [0.15, np.nan, 0.0], [np.nan, np.nan, 0.0], [-0.12, 0.0, 0.0]])
    m = metrics_from_arrays(rpy, np.zeros((5, 3)), np.zeros((5, 4)), np.zeros(4))
    assert m[4] == 0.2           # the NaN angles are passed over, the other angle of the same step still counts
    assert math.isnan(m[0]) and math.isnan(m[1])  # the sums do carry them


def test_one_step():
    from phoenix_drone_simulation_amd.evaluation import metrics_from_arrays
    m = metrics_from_arrays([[0.5, -0.25, 1.0]], [[-1.0, 2.0, 3.0]], [[2.0, 0.0, 0.0, 0.0]], [1.0, 0.0, 0.0, 0.5])
    assert list(m) == [0.25, 0.0625, 14.0, 1.25, 0.5, 1.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        metrics_from_arrays(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 4)), np.zeros(4))
    with pytest.raises(ValueError):
        metrics_from_arrays(np.zeros((2, 3)), np.zeros((3, 3)), np.zeros((2, 4)), np.zeros(4))


def test_table_units_and_division_by_the_length():
    from phoenix_drone_simulation_amd.evaluation import FlightMetrics
    rad = math.pi / 180.0
    raw = torch.zeros(2, 2, 8)
    length = torch.tensor([[100.0, 50.0], [200.0, 200.0]])
    # policy 0, episode 0: 100 steps at a constant 2 deg roll and 3 deg pitch, 10 crossings of the roll rate in 1 s
    raw[0, 0] = torch.tensor([100 * (2 * rad) ** 2, 100 * (3 * rad) ** 2, 7.0, 25.0, 4 * rad, 10.0, 10.0, 4.0])
    raw[0, 1] = torch.tensor([50 * (4 * rad) ** 2, 0.0, 0.0, 5.0, 6 * rad, 0.0, 0.0, 2.0])
    raw[1, :, 5] = 200.0  # every step saturated
    fm = FlightMetrics(raw, length, step_seconds=0.01)
    assert torch.equal(fm.roll_sq, raw[..., 0]) and torch.equal(fm.pitch_rate_crossings, raw[..., 7])
    assert fm.tilt_max.shape == (2, 2) and fm.step_seconds == 0.01
    with pytest.raises(AttributeError):
        fm.no_such_metric
    ep = fm.per_episode()
    assert float(ep["flight_time"][0, 0]) == pytest.approx(1.0) and float(ep["flight_time"][0, 1]) == pytest.approx(0.5)
    assert float(ep["mse_roll_deg2"][0, 0]) == pytest.approx(4.0, rel=1e-5)
    assert float(ep["mse_pitch_deg2"][0, 0]) == pytest.approx(9.0, rel=1e-5)
    assert float(ep["freq_roll_rate_hz"][0, 0]) == pytest.approx(5.0)      # 10 sign changes in 1 s: 5 oscillations
    assert float(ep["freq_pitch_rate_hz"][0, 1]) == pytest.approx(2.0)     # 2 in 0.5 s
    t = fm.table()
    assert set(t) == {"flight_time", "mse_roll_deg2", "mse_pitch_deg2", "freq_roll_rate_hz", "freq_pitch_rate_hz", "action_rate",
                      "saturated_share", "tilt_max_deg"}
    for v in t.values():
        assert tuple(v.shape) == (2,)
    assert float(t["flight_time"][0]) == pytest.approx(0.75) and float(t["flight_time"][1]) == pytest.approx(2.0)
    assert float(t["mse_roll_deg2"][0]) == pytest.approx((4.0 + 16.0) / 2, rel=1e-5)
    assert float(t["action_rate"][0]) == pytest.approx((25.0 / 100 + 5.0 / 50) / 2)
    assert float(t["saturated_share"][0]) == pytest.approx(0.05) and float(t["saturated_share"][1]) == pytest.approx(1.0)
    assert float(t["tilt_max_deg"][0]) == pytest.approx(5.0, rel=1e-5)
    with pytest.raises(ValueError):
        FlightMetrics(torch.zeros(2, 2, 7), length, 0.01)


def test_penalised_return_formula_and_unknown_names():
    from phoenix_drone_simulation_amd.es import penalised_return
    from phoenix_drone_simulation_amd.evaluation import FlightMetrics
    g = torch.Generator().manual_seed(0)
    ret, length = torch.randn(4, 64, generator=g), torch.full((4, 64), 10.0)
    raw = torch.rand(4, 64, 8, generator=g)
    fm = FlightMetrics(raw, length, 0.01)
    f = penalised_return({"action_rate_sq": 0.5, "rate_sq": 2.0})
    got = f(ret, length, torch.zeros(4, 64), fm)
    want = (ret - 0.5 * raw[..., 3] - 2.0 * raw[..., 2]).mean(dim=1)
    assert tuple(got.shape) == (4,) and torch.allclose(got, want, rtol=1e-6, atol=1e-6)
    assert torch.equal(penalised_return({})(ret, length, None, fm), ret.mean(dim=1))
    with pytest.raises(ValueError, match="jerk"):
        penalised_return({"jerk": 1.0})


def test_trainer_rejects_a_fitness_that_is_not_callable_before_it_touches_the_env():
    import types
    from phoenix_drone_simulation_amd.es import ESTrainer
    with pytest.raises(ValueError, match="fitness"):
        ESTrainer(types.SimpleNamespace(num_envs=128), 2, fitness="return")


def test_the_entry_point_is_declared_exported_and_bound():
    from phoenix_drone_simulation_amd import native
    hdr = open(os.path.join(ROOT, "include", "pds.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+pds_evaluate_policies_metrics\s*\(", hdr)
    assert "pds_evaluate_policies_metrics" in native.EXPORTS
    lib = native.load()
    assert len(lib.pds_evaluate_policies_metrics.argtypes) == len(lib.pds_evaluate_policies.argtypes) + 1 == 15
    assert lib.pds_evaluate_policies_metrics(None, 1, 64, None, None, None, None, 0.0, 1, None, None, None, None, None, None) == native.EINVAL


def test_metrics_needs_the_same_layout_checks_as_the_plain_call():
    import types
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    n = 8 * 34 + 8 + 8 * 8 + 8 + 4 * 8 + 4
    pop = PolicyPopulation.from_flat(torch.zeros(3, n), 34, (8, 8), "tanh")
    with pytest.raises(ValueError, match="multiple of 64"):
        evaluate_population(types.SimpleNamespace(num_envs=3 * 32), pop, metrics=True)
