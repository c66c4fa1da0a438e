#!/usr/bin/env python3
"""Golden trajectories of the REFERENCE envs with observation_history_size = H on the latency ring (build container only):
tests/golden/history_latency.npz.  Experiment 04 of the reference trains with history sizes 1, 2, 4, 6, 8, experiment 07 crosses
control mode, motor time constant and latency; this file is where the two meet.

The recipe is oracle/refgen/gen_golden_history.py's: a deterministic configuration (no sensor / thrust noise, no domain
randomisation, no reset distribution), so the trajectory is a pure function of the action sequence: reset, step a recorded action
sequence, reset again behind every finished episode, step on.  The latency model is switched on the way gen_golden.py does it:
`drone.use_latency = True` after construction (the Simple agent is built without it), the ring keeps its constructor size
max(1, int(latency // time_step)).  One trajectory calls drone.set_latency(x) in the middle of an episode.  Only data is written
(actions in; observations, rewards, flags and buf_size out).

What makes these trajectories differ from history.npz: after a reset the reference's action_history holds VIEWS of
action_buffer[-1] (envs/agents.py:386, envs/base.py:424-429), and apply_action rewrites that row while they are still in the
history.  The generator counts the steps at which such a rewrite is visible and fails if a trajectory has none (except the control
with buf_size > H, which must have none)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, os.path.join(ROOT, "oracle", "refgen", "standins"))
sys.path.insert(0, "/root/reference")

import gymnasium as gym  # noqa: E402  (stand-in)
import phoenix_drone_simulation  # noqa: E402,F401

ENV_IDS = {"hover": "DroneHoverSimpleEnv-v0", "circle": "DroneCircleSimpleEnv-v0", "takeoff": "DroneTakeOffSimpleEnv-v0"}

# name, task, H, latency, aggregate_phy_steps (None: the env takes no such keyword), steps, set_latency value or None, TimeLimit
# (TakeOff never terminates, envs/takeoff.py:96-100: its episodes end at a limit of 25 steps, which the loop below applies the way
# gymnasium's TimeLimit wrapper does -- truncated = True at the limit-th step of an episode)
CASES = [
    ("hover_h4_l025_a1", "hover", 4, 0.025, 1, 90, None, 500),
    ("hover_h4_l035_a2", "hover", 4, 0.035, 2, 80, None, 500),
    ("circle_h6_l020_a1", "circle", 6, 0.02, 1, 80, None, 500),
    ("circle_h8_l045_a1", "circle", 8, 0.045, 1, 90, None, 500),
    ("takeoff_h4_l035", "takeoff", 4, 0.035, None, 80, None, 25),
    ("hover_h1_l015_a1", "hover", 1, 0.015, 1, 60, None, 500),
    ("hover_h8_l015_a3", "hover", 8, 0.015, 3, 90, None, 500),
    ("hover_h3_l050_a1", "hover", 3, 0.05, 1, 80, None, 500),  # the control: buf_size > H, nothing may change
    ("hover_h4_l025_a1_set015", "hover", 4, 0.025, 1, 90, 0.015, 500),
]


def run(task, H, latency, agg, steps, seed, set_latency, limit):
    kw = dict(observation_history_size=H, observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0.0,
              enable_reset_distribution=False, latency=latency)
    if agg is not None:
        kw["aggregate_phy_steps"] = agg
    env = gym.make(ENV_IDS[task], **kw)
    e = env.unwrapped
    e.drone.use_latency = True
    rs = np.random.RandomState(seed)
    obs0, _ = env.reset()
    hover = -1.0 + 2.0 / 2.25
    out = {k: [] for k in ("actions", "obs", "reward", "terminated", "truncated", "cost", "reset_obs", "buf_size")}
    j, visible, set_at = 0, 0, -1
    for t in range(steps):
        if set_latency is not None and set_at < 0 and t >= 20 and j == 1:
            e.drone.set_latency(set_latency)  # one step into an episode: H - 1 views are still in the history
            set_at = t
        drift = (0.012 * j if task != "takeoff" else 0.0) * np.array([1, -1, -1, 1.0])
        a = hover + (0.25 if task == "takeoff" else 0.0) + 0.15 * rs.standard_normal(4) + drift
        views = sum(np.shares_memory(x, e.drone.action_buffer) for x in e.action_history)
        row = e.drone.action_buffer[-1].copy()
        o, r, te, tr, info = env.step(a)
        j += 1
        tr = bool(tr) or j >= limit
        visible += int(views > 0 and not np.array_equal(row, e.drone.action_buffer[-1]))
        out["actions"].append(a); out["obs"].append(np.array(o, dtype=np.float64)); out["reward"].append(float(r))
        out["terminated"].append(bool(te)); out["truncated"].append(bool(tr)); out["cost"].append(float(info.get("cost", 0.0)))
        out["buf_size"].append(int(e.drone.buf_size))
        if te or tr:
            o2, _ = env.reset()
            j = 0
            out["reset_obs"].append(np.array(o2, dtype=np.float64))
        else:
            out["reset_obs"].append(np.zeros_like(np.array(o, dtype=np.float64)))
    d = {k: np.array(v) for k, v in out.items()}
    d["obs0"] = np.array(obs0, dtype=np.float64)
    d["H"], d["latency"], d["agg"] = np.int64(H), np.float64(latency), np.int64(agg or 1)
    d["max_steps"] = np.int64(limit)
    d["set_latency_at"], d["set_latency"] = np.int64(set_at), np.float64(set_latency if set_latency is not None else 0.0)
    return d, visible


def main():
    out = {}
    for i, (name, task, H, latency, agg, steps, set_latency, limit) in enumerate(CASES):
        d, visible = run(task, H, latency, agg, steps, seed=300 + i, set_latency=set_latency, limit=limit)
        for k, v in d.items():
            out[f"{name}_{k}"] = v
        ended = int(d["terminated"].sum() + d["truncated"].sum())
        B = int(d["buf_size"][0])
        print(f"{name}: obs dim {d['obs'].shape[1]}, buf_size {B}, episodes ended {ended}, steps with a visible rewrite {visible}"
              + (f", set_latency({set_latency}) in front of step {int(d['set_latency_at'])}" if set_latency is not None else ""))
        assert ended >= 2, name
        assert (visible == 0) == (B > H), (name, visible, B, H)
        assert set_latency is None or d["set_latency_at"] >= 0, name
    out["names"] = np.array([c[0] for c in CASES])
    out["tasks"] = np.array([c[1] for c in CASES])
    path = os.path.join(ROOT, "tests", "golden", "history_latency.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "kB")


if __name__ == "__main__":
    main()
