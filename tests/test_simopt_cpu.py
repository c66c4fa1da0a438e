"""Sim-opt objective, the parts that need no GPU: the recipe restated on the CPU oracle against the reference's recorded
values (tests/golden/simopt.npz, written by tools/refgen/gen_golden_simopt.py from the reference itself), the data side
(MiniTrajectories) against the reference's slices, and the host-side arithmetic of the kernel's inputs."""
import numpy as np
import pytest

import simopt_oracle as so
from oracle import oracle

import phoenix_drone_simulation_amd as pds
from phoenix_drone_simulation_amd import simopt

# The project's single-step bar (tests/test_oracle_golden.py): 1e-6 relative + 1e-7 absolute.
RTOL, ATOL = 1e-6, 1e-7
# Largest relative distance of the FLOAT32 oracle's losses from the reference's float64 ones over the three fixture blocks,
# measured by test_f32_oracle_deviation_is_the_recorded_one below (block p40, candidate 6).  tests/test_gpu_simopt.py builds
# its bar from this number; profiles/simopt_parity_margins.txt records it next to the GPU's margin.
F32_ORACLE_MAX_REL = 1.7483e-4


@pytest.fixture(scope="module")
def golden():
    return np.load(so.GOLDEN)


@pytest.mark.parametrize("name", so.BLOCKS)
def test_oracle_recipe_reproduces_every_evaluate_once(golden, name):
    """Double reset, ring zeroing, R @ / R.T @, clipping of T, latency off below one step: the float64 oracle running the
    restated recipe gives the reference's simulated observations and losses."""
    b = so.load_block(name, golden)
    losses, sims = so.evaluate_block(b, "f64", want_sims=True)
    for i, (p, m) in enumerate(b["sim_pairs"]):
        np.testing.assert_allclose(sims[p, m], b["sim_obs"][i], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(losses, b["evaluate_once"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(losses.mean(1), b["evaluate"], rtol=RTOL, atol=ATOL)


def test_f32_oracle_deviation_is_the_recorded_one(golden):
    """What float32 arithmetic alone costs on this fixture: the GPU bar is 4 x this maximum (tests/test_gpu_simopt.py)."""
    worst = 0.0
    for name in so.BLOCKS:
        b = so.load_block(name, golden)
        ref = b["evaluate_once"]
        worst = max(worst, float((np.abs(so.evaluate_block(b, "f32") - ref) / np.abs(ref)).max()))
    print(f"f32 oracle vs reference: max relative loss deviation {worst:.4e}")
    assert worst <= F32_ORACLE_MAX_REL * 1.0005, worst   # (the constant is the measurement rounded to 5 digits)
    assert worst >= F32_ORACLE_MAX_REL * 0.5, worst      # ... and has not silently become a much looser bar than needed


@pytest.mark.parametrize("name", so.BLOCKS)
def test_from_logs_equals_the_reference_slices(golden, name):
    b = so.load_block(name, golden)
    cleaned = simopt.MiniTrajectories.exclude_battery_compensation(b["log_pwms"], b["log_voltages"])
    assert np.array_equal(cleaned, b["pwms_cleaned"])
    data = simopt.MiniTrajectories.from_logs(b["log_obs"], b["log_pwms"], b["log_voltages"], T=35, pre_steps=int(b["pre_steps"]))
    assert np.array_equal(data.observations, b["observations"])
    assert np.array_equal(data.actions, b["actions"])
    assert np.array_equal(data.pre_inputs, b["pre_inputs"])
    assert len(data) == len(b["observations"]) and data.pre_steps == int(b["pre_steps"]) and data.mini_trajectory_size == 35
    two = simopt.MiniTrajectories.from_logs([b["log_obs"]] * 2, [b["log_pwms"]] * 2, [b["log_voltages"]] * 2,
                                            pre_steps=int(b["pre_steps"]))
    assert len(two) == 2 * len(data) and np.array_equal(two.actions[len(data):], data.actions)
    sub = data.select([3, 1])
    assert np.array_equal(sub.observations, data.observations[[3, 1]])


def test_from_csv_dir_reads_the_reference_columns(golden, tmp_path):
    import pandas as pd
    b = so.load_block("a1", golden)
    cols = simopt.OBS_COLUMNS + simopt.PWM_COLUMNS + ["bat"]
    df = pd.DataFrame(np.hstack([b["log_obs"], b["log_pwms"], b["log_voltages"]]), columns=cols)
    df.insert(0, "time", np.arange(len(df)) * 0.01)
    (tmp_path / "flight").mkdir()
    df.to_csv(tmp_path / "flight" / "log0.csv", index=False)
    df.iloc[:20].to_csv(tmp_path / "flight" / "too_short.csv", index=False)
    data = simopt.MiniTrajectories.from_csv_dir(str(tmp_path))
    # (through the CSV's decimal text: pandas' default float parser is accurate to a few ulps, not round-trip exact)
    np.testing.assert_allclose(data.observations, b["observations"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(data.actions, b["actions"], rtol=1e-12, atol=1e-15)
    with pytest.raises(FileNotFoundError):
        simopt.MiniTrajectories.from_csv_dir(str(tmp_path / "flight" / "nothing_here"))


def test_start_state_is_the_oracle_reset(golden):
    """Row 0 of the kernel's observation table: the state the reference's second reset produces from the logged row."""
    b = so.load_block("a1", golden)
    env = so.make_env("f64")
    rs = np.random.RandomState(3)
    rows = np.vstack([b["observations"][:, 0], rs.uniform(-1, 1, size=(6, 12)) * [1, 1, 1, 1, 1, 1, 1.2, 1.2, 3.5, 4, 4, 4]])
    got = simopt.start_state(rows)
    for row, g in zip(rows, got):
        R = oracle.matrix_from_quat(oracle.quat_from_euler(row[6:9]))
        w = R @ row[9:12]
        for i in range(3):
            env.cfg.init_xyz[i], env.cfg.init_xyz_dot[i], env.cfg.init_rpy[i], env.cfg.init_rpy_dot[i] = row[i], row[3 + i], row[6 + i], w[i]
        env.reset()
        want = np.concatenate([env.get("xyz"), env.get("xyz_dot"), env.get("rpy"), env.get("rpy_dot")])
        np.testing.assert_allclose(g, want, rtol=1e-12, atol=1e-14)


def test_kernel_layout(golden):
    b = so.load_block("p40", golden)
    data = simopt.MiniTrajectories.from_arrays(b["observations"], b["actions"], b["pre_inputs"])
    acts, obs, pre = data.kernel_layout()
    M, T = len(data), 35
    assert acts.shape == (T, M, 4) and obs.shape == (T, 3, M, 4) and pre.shape == (40, M, 4)
    assert acts.dtype == obs.dtype == pre.dtype == np.float32
    assert np.array_equal(acts[7, 5], b["actions"][5, 7].astype(np.float32))
    assert np.array_equal(pre[39, 2], b["pre_inputs"][2, 39].astype(np.float32))
    assert np.array_equal(obs[9, :, 4].reshape(12), b["observations"][4, 9].astype(np.float32))
    assert np.array_equal(obs[0, :, 4].reshape(12), simopt.start_state(b["observations"][4, 0]).astype(np.float32))


def test_latency_steps_is_the_float64_division():
    ts = 0.01
    lat = np.array([0.0, 0.005, 0.0099999, 0.01, 0.0105, 0.02, 0.03, 0.0305, 0.05, 0.0905, np.nan])
    want = [0 if not v >= ts else int(v / ts) for v in lat[:-1]] + [0]
    assert want[3] == 1 and want[6] == 3 and want[7] == 3 and want[9] == 9
    assert simopt.latency_steps(lat, ts).tolist() == want
    cands = np.load(so.GOLDEN)["candidates"]
    assert simopt.latency_steps(np.clip(cands[:, 2], 0, np.inf), ts).tolist() == [2, 0, 1, 0, 5, 4, 1, 0]


def test_module_imports_without_a_gpu_and_the_objective_needs_one(golden):
    import torch
    assert pds.simopt is simopt and pds.SimOptObjective is simopt.SimOptObjective
    assert np.array_equal(simopt.PARAMETER_LOW, [1.5, 0.010, 0.0]) and np.array_equal(simopt.PARAMETER_HIGH, [2.5, 0.5, 0.05])
    b = so.load_block("a1", golden)
    data = simopt.MiniTrajectories.from_arrays(b["observations"], b["actions"], b["pre_inputs"])
    if torch.cuda.is_available():
        obj = simopt.SimOptObjective('DroneHoverSimpleEnv-v0', data)
        assert obj.parameter_space.contains(np.array([2.0, 0.08, 0.02], np.float32))
    else:
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            simopt.SimOptObjective('DroneHoverSimpleEnv-v0', data)
