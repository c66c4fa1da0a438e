"""The sim-opt recipe (ObjectiveFunctionPyBullet.evaluate_once + loss_function, simopt/pybullet.py:127-227, on the SimplePhysics
env with the PT1 motor model) restated on the CPU oracle: reset, set, set_latency, step, euler_from_quat.  TEST INFRASTRUCTURE:
tests/test_simopt_cpu.py pins it against the reference's recorded values (tests/golden/simopt.npz), tests/test_gpu_simopt.py
takes its float32 run as the measure of what float32 arithmetic alone costs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

G = 9.81
GOLDEN = os.path.join(ROOT, "tests", "golden", "simopt.npz")
BLOCKS = ("a1", "a2", "p40")


def load_block(name, z=None):
    z = z if z is not None else np.load(GOLDEN)
    b = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}
    b.update(candidates=z["candidates"], sim_pairs=z["sim_pairs"], gamma=float(z["gamma"]), truth=z["truth"])
    return b


def make_env(precision, aggregate_phy_steps=1):
    return oracle.OracleEnv("hover", precision, use_motor_dynamics=1, observation_noise=-1, domain_randomization=-1.0,
                            motor_thrust_noise=0.0, enable_reset_distribution=0, aggregate_phy_steps=int(aggregate_phy_steps))


def set_parameters(env, params):
    """simopt/pybullet.py:233-248: clip at 0, update_motor_dynamics (envs/agents.py:208-224), set_latency (:388-404)."""
    p = np.clip(np.asarray(params, np.float64), 0, np.inf)
    Ts = float(env.cfg.time_step)
    T = max(p[1], Ts)
    env.set("T", [T] * 4)
    env.set("t2w", [p[0]] * 4)
    env.set("A", [1 - Ts / T] * 4)
    env.set("B", [Ts / T] * 4)
    env.set("K", [0.028 * G * p[0] / 4] * 4)
    env.set_latency(float(p[2]))


def loss_function(obs_sim, obs_real, precision):
    """simopt/pybullet.py:196-227 in the arithmetic of `precision`."""
    real = np.float64 if precision == "f64" else np.float32
    s, r = np.asarray(obs_sim, real), np.asarray(obs_real, real)
    rpy = np.asarray(oracle.euler_from_quat(s[3:7], precision), real)
    err = np.hstack((rpy - r[6:9], real(100) * (s[0:3] - r[0:3]), real(10) * (s[7:10] - r[3:6]), s[10:13] - r[9:12])).astype(real)
    return real(np.abs(err).sum(dtype=real) + np.sqrt((err * err).sum(dtype=real)))


def evaluate_once(env, obs, acs, pre_inputs, gamma, precision):
    """-> (loss, simulated observations [T - 1, 13]).  `env` carries the candidate's parameters (set_parameters)."""
    real = np.float64 if precision == "f64" else np.float32
    cfg = env.cfg
    # 1) pre-steps from a reset env (enable_reset_distribution off: motor state and delayed-action ring start at 0)
    for i in range(3):
        cfg.init_xyz[i], cfg.init_rpy[i], cfg.init_xyz_dot[i], cfg.init_rpy_dot[i] = (0.0, 0.0, 1.0)[i], 0.0, 0.0, 0.0
    env.reset()
    for u in pre_inputs:
        env.step(u)
    x, y = env.get("x").copy(), env.get("y").copy()
    # 2) the logged state becomes the env's init_*: quaternion from rpy, init_rpy_dot = R @ rpy_dot (:139-150)
    x0 = np.asarray(obs[0], np.float64)
    R = oracle.matrix_from_quat(oracle.quat_from_euler(x0[6:9]))
    w = R @ x0[9:12]
    for i in range(3):
        cfg.init_xyz[i], cfg.init_rpy[i], cfg.init_xyz_dot[i], cfg.init_rpy_dot[i] = x0[i], x0[6 + i], x0[3 + i], w[i]
    # 3) reset (its own R.T @, the pose read-back, ring zeroed again), motor state restored
    env.reset()
    env.set("x", x)
    env.set("y", y)
    # 4) replay
    T = len(obs)
    half = env.obs_dim // 2
    sims, acc, disc = [], real(0), 1.0
    for i in range(T - 1):
        o = env.step(acs[i])[0]
        sim = np.array(o[half:half + 13])
        sims.append(sim)
        acc = real(acc + real(disc) * loss_function(sim, obs[i + 1], precision))
        disc *= gamma
    return float(acc / real(T - 1)), np.array(sims)


def evaluate_block(block, precision, candidates=None, want_sims=False):
    """losses [P, M] (and the simulated observations [P, M, T - 1, 13]) of a fixture block on the oracle."""
    cands = block["candidates"] if candidates is None else candidates
    obs, acs, pre = block["observations"], block["actions"], block["pre_inputs"]
    env = make_env(precision, block["aggregate_phy_steps"])
    losses = np.zeros((len(cands), len(obs)))
    sims = np.zeros((len(cands), len(obs), obs.shape[1] - 1, 13))
    for p, params in enumerate(cands):
        set_parameters(env, params)
        for m in range(len(obs)):
            losses[p, m], sims[p, m] = evaluate_once(env, obs[m], acs[m], pre[m], block["gamma"], precision)
    return (losses, sims) if want_sims else losses
