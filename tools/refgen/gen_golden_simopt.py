#!/usr/bin/env python3
"""Generate tests/golden/simopt.npz by running the REFERENCE's sim-opt objective itself (build container only).

Imports `phoenix_drone_simulation` from a checkout of the reference (--reference, or the PDS_REFERENCE environment variable)
with the stand-in modules of oracle/refgen/standins/ on sys.path for its absent third-party imports, as
oracle/refgen/gen_golden.py does, plus a dummy torch.utils.tensorboard.  Only DATA is written: inputs and expected outputs.

What runs is the reference's recipe: a subclass of ObjectiveFunctionPyBullet whose _load_simulation returns
DroneHoverSimpleEnv(motor_thrust_noise=0, observation_noise=-1, domain_randomization=-1, enable_reset_distribution=False) with
drone.use_motor_dynamics = True, and whose _load_real_world_data returns a buffer filled from SYNTHETIC logs -- the same env
flown at known parameters under a gentle open-loop excitation around hover -- written as the 12 log columns + PWMs + a constant
battery voltage and pushed through the reference's own exclude_battery_compensation / create_trajectory_slices.

Blocks: `a1` (aggregate_phy_steps 1, pre_steps 5), `a2` (aggregate_phy_steps 2, pre_steps 5), `p40` (1, pre_steps 40).  Per
block: the log, the slices, 8 candidates, evaluate_once of every (candidate, slice), evaluate per candidate, and the simulated
observations (first 13 columns) of two pairs.

Usage: python tools/refgen/gen_golden_simopt.py --reference /path/to/phoenix-drone-simulation [--out tests/golden]
"""
import argparse
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))

TRUTH = np.array([2.0, 0.08, 0.02])
LOG_STEPS, T, VOLTAGE = 260, 35, 3.9
# the truth; latency below one time step; T below T_s (buf_size 1); the lower bounds; the upper bounds (buf_size 5);
# buf_size 4; buf_size 1; a negative latency (clipped at 0)
CANDIDATES = np.array([[2.0, 0.08, 0.02],
                       [2.1, 0.06, 0.005],
                       [1.9, 0.004, 0.0105],
                       [1.5, 0.010, 0.000],
                       [2.5, 0.500, 0.050],
                       [2.2, 0.12, 0.0405],
                       [2.0, 0.10, 0.0155],
                       [2.3, 0.05, -0.01]])
SIM_PAIRS = np.array([[0, 0], [5, 7]])  # (candidate, slice) whose simulated observations are kept


def load_reference(path):
    sys.path.insert(0, os.path.join(ROOT, "oracle", "refgen", "standins"))
    sys.path.insert(0, path)
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    import phoenix_drone_simulation  # noqa: F401
    from phoenix_drone_simulation.envs.hover import DroneHoverSimpleEnv
    from phoenix_drone_simulation.simopt.core import RealWorldDataBuffer, DataBufferBase
    from phoenix_drone_simulation.simopt.pybullet import ObjectiveFunctionPyBullet
    return DroneHoverSimpleEnv, RealWorldDataBuffer, DataBufferBase, ObjectiveFunctionPyBullet


def excitation(truth, steps, dt, seed=0):
    """hover + 0.15 sin(2 pi 1.3 t) on all motors + 0.03 x the mean of three sines at 2-5 Hz with random phases per motor."""
    rs = np.random.RandomState(seed)
    phase = rs.uniform(0, 2 * np.pi, size=(3, 4))
    freq = rs.uniform(2.0, 5.0, size=(3, 4))
    hover = (1.0 / truth[0]) * 2 - 1
    t = np.arange(steps)[:, None, None] * dt
    a = hover + 0.03 * np.sin(2 * np.pi * freq * t + phase).sum(1) / 3 + 0.15 * np.sin(2 * np.pi * 1.3 * t[:, 0])
    return np.clip(a, -1, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("PDS_REFERENCE"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or PDS_REFERENCE): path of the reference checkout")
    Env, RealWorldDataBuffer, DataBufferBase, Objective = load_reference(args.reference)

    def make_env(agg):
        e = Env(aggregate_phy_steps=agg, motor_thrust_noise=0.0, observation_noise=-1, domain_randomization=-1,
                enable_reset_distribution=False)
        e.drone.use_motor_dynamics = True
        return e

    def fly(agg):
        """The log: 12 columns (x y z, xyz_dot, rpy, rpy_dot) and the PWMs the flight controller would have logged."""
        e = make_env(agg)
        e.drone.update_motor_dynamics(new_motor_time_constant=TRUTH[1], new_thrust_to_weight_ratio=TRUTH[0])
        e.drone.set_latency(TRUTH[2])
        e.reset()
        e.drone.x = np.full(4, np.sqrt(1.0 / TRUTH[0]))  # motors at their hover state
        steps = LOG_STEPS // agg  # the same 2.6 s of flight: one log row per env.step
        acs = excitation(TRUTH, steps, 0.01 * agg)
        obs = []
        for a in acs:
            o = e.observation_history[-1].copy()
            obs.append(np.concatenate([o[0:3], o[7:10], e.drone.rpy.copy(), o[10:13]]))
            e.step(a)
        obs = np.array(obs)
        assert obs[:, 2].min() > 0.3 and np.abs(obs[:, 6:8]).max() < 0.3, "the open-loop flight must stay airborne and upright"
        # invert the battery compensation at a constant voltage so that the reference's own cleaning gives the PWMs back
        pwms = (acs + 1) * 30000.0
        thrust = pwms / 65535 * 60
        volts = -0.0006239 * thrust ** 2 + 0.088 * thrust
        raw = volts / VOLTAGE * 65535
        return obs, raw, np.full((steps, 1), VOLTAGE)

    class Buffer(DataBufferBase):
        def __init__(self, obs, acs, pre):
            self.mini_trajectory_size, self.pre_steps = obs.shape[1], pre.shape[1]
            self.observations, self.actions, self.pre_inputs = obs, acs, pre

        def load_from_disk(self):
            pass

        def reset(self):
            pass

    out = {"truth": TRUTH, "candidates": CANDIDATES, "sim_pairs": SIM_PAIRS, "gamma": np.float64(0.95)}
    for name, agg, pre_steps in (("a1", 1, 5), ("a2", 2, 5), ("p40", 1, 40)):
        log_obs, log_pwms, log_volts = fly(agg)
        cleaned = RealWorldDataBuffer.exclude_battery_compensation(log_pwms, log_volts)
        rw = object.__new__(RealWorldDataBuffer)
        rw.mini_trajectory_size, rw.pre_steps = T, pre_steps
        obs_s, acs_s, pre_s = rw.create_trajectory_slices(log_obs, cleaned)
        sims = {}

        class Obj(Objective):
            record = None

            def _load_simulation(self):
                return make_env(agg)

            def _load_real_world_data(self):
                return Buffer(obs_s, acs_s, pre_s)

            @classmethod
            def loss_function(cls, obs_sim, obs_real):
                if cls.record is not None:
                    cls.record.append(np.array(obs_sim[:13], dtype=np.float64))
                return super().loss_function(obs_sim=obs_sim, obs_real=obs_real)

        f = Obj(files_path="", seed=0)
        M = obs_s.shape[0]
        once = np.zeros((len(CANDIDATES), M))
        for p, params in enumerate(CANDIDATES):
            f.set_parameters(params)
            for m in range(M):
                keep = any((p, m) == tuple(x) for x in SIM_PAIRS)
                Obj.record = [] if keep else None
                once[p, m] = f.evaluate_once(obs_s[m], acs_s[m], pre_inputs=pre_s[m])
                if keep:
                    sims[(p, m)] = np.array(Obj.record)
        Obj.record = None
        score = np.array([f.evaluate(params) for params in CANDIDATES])
        np.testing.assert_allclose(score, once.mean(1), rtol=1e-12)
        out.update({f"{name}_aggregate_phy_steps": np.int64(agg), f"{name}_pre_steps": np.int64(pre_steps),
                    f"{name}_log_obs": log_obs, f"{name}_log_pwms": log_pwms, f"{name}_log_voltages": log_volts,
                    f"{name}_pwms_cleaned": cleaned, f"{name}_observations": obs_s, f"{name}_actions": acs_s,
                    f"{name}_pre_inputs": pre_s, f"{name}_evaluate_once": once, f"{name}_evaluate": score,
                    f"{name}_sim_obs": np.array([sims[tuple(x)] for x in SIM_PAIRS])})
        print(name, "M", M, "score", np.round(score, 4), "z", log_obs[:, 2].min(), log_obs[:, 2].max(),
              "max |roll, pitch|", np.abs(log_obs[:, 6:8]).max())
    path = os.path.join(args.out, "simopt.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
