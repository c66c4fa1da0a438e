#!/usr/bin/env python3
"""Times evaluate_population(fused=True) -- one launch -- against fused=False, the composed path out of entry points that were
there before the kernel (per step one pds_mlp_forward per policy + pds_step + five elementwise ops): the baseline.

Both paths run in ONE process and alternate; every shape is warmed up first; the host clock runs around work that ends in a
device synchronise (the results come back to the host); each path of each shape is timed for at least --seconds and the
spread over its repeats is printed.  Shapes, on Hover at its defaults: P x E = 1 x 8192, 64 x 128, 1024 x 64, each with
tests/golden/hip_policy_early.npz (episodes end by falling) and hip_policy_late.npz (episodes run to the TimeLimit).

  python profiles/tools/evaluate_bench.py > profiles/evaluate_timing.txt

--history H [H]: the history form instead (pds_evaluate_policies_history, csrc/pds_evaluate_hist.h) -- evaluate_population(fused=True,
history_fused=True) against fused=False on envs with observation_history_size = H: Hover at its defaults (first H) and lean Circle
(second H, or the first again), seeded random tanh actors (64, 64) with spread output biases, P x E = 8 x 128 and 64 x 1024; medians
of --reps alternating synchronised repeats.

  python profiles/tools/evaluate_bench.py --history 4 8 > profiles/evaluate_history_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population  # noqa: E402
from phoenix_drone_simulation_amd.ppo import ActorCritic  # noqa: E402

SHAPES = ((1, 8192), (64, 128), (1024, 64))


def population(name, P):
    sd = np.load(os.path.join(ROOT, "tests", "golden", f"hip_policy_{name}.npz"))
    one = PolicyPopulation.from_actor_critics([ActorCritic.from_reference_state_dict({k: sd[k] for k in sd.files})])
    return PolicyPopulation.from_flat(one.theta.expand(P, -1), one.d_in, one.hidden_sizes, one.activation,
                                      one.mean.expand(P, -1), one.std.expand(P, -1), one.eps)


def timed(env, pop, fused, history_fused=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate_population(env, pop, fused=fused, history_fused=history_fused)  # ends in the copies to the host: synchronised
    return time.perf_counter() - t0, out


HISTORY_SHAPES = ((8, 128), (64, 1024))
HISTORY_CASES = (("hover default", "DroneHoverSimpleEnv-v0", {}),
                 ("circle lean", "DroneCircleSimpleEnv-v0", dict(observation_noise=0, domain_randomization=0.0, motor_thrust_noise=0.0)))


def random_population(d_in, P, seed=0, hidden=(64, 64)):
    """seeded actors in torch's nn.Linear initialisation, tanh, output biases spread from "falls at once" to "climbs" """
    g = torch.Generator().manual_seed(seed)
    h1, h2 = hidden
    blocks = ((d_in, h1 * d_in), (d_in, h1), (h1, h2 * h1), (h1, h2), (h2, 4 * h2), (h2, 4))
    theta = torch.cat([(torch.rand(P, count, generator=g) * 2 - 1) / fan_in ** 0.5 for fan_in, count in blocks], dim=1)
    theta[:, -4:] += torch.linspace(-0.6, 0.6, P).unsqueeze(1) if P > 1 else -0.3
    return PolicyPopulation.from_flat(theta, d_in, hidden, "tanh")


def history_main(args):
    print(f"# evaluate_population(history_fused=True) on envs with an observation history, {torch.cuda.get_device_name(0)}; host clock "
          f"around a call that ends in the device-to-host copy of its results; paths alternate; median [min .. max] over {args.reps} reps")
    print("# env  H inputs  P x E | fused: ms, episodes/s | composed: ms, episodes/s | composed / fused | mean length | same bits")
    for j, (label, env_id, kw) in enumerate(HISTORY_CASES):
        H = args.history[min(j, len(args.history) - 1)]
        for P, E in HISTORY_SHAPES:
            env_f = pds.make(env_id, num_envs=P * E, seed=1, observation_history_size=H, **kw)
            env_c = pds.make(env_id, num_envs=P * E, seed=1, observation_history_size=H, **kw)
            pop = random_population(env_f.obs_dim, P).to("cuda:0")
            _, first_f = timed(env_f, pop, True, True)  # warm-up of both paths (and the bitwise comparison: same seed, first call)
            _, first_c = timed(env_c, pop, False)
            same = all(torch.equal(a, b) for a, b in zip(first_f, first_c))
            tf, tc = [], []
            for _ in range(args.reps):
                tf.append(timed(env_f, pop, True, True)[0])
                tc.append(timed(env_c, pop, False)[0])
            mf, mc = float(np.median(tf)), float(np.median(tc))
            n = P * E
            print(f"{label:13s} {H:2d} {env_f.obs_dim:4d} {P:5d} x {E:5d} | {1e3 * mf:9.2f} [{1e3 * min(tf):.2f} .. {1e3 * max(tf):.2f}] {n / mf:12.0f} | "
                  f"{1e3 * mc:10.2f} [{1e3 * min(tc):.2f} .. {1e3 * max(tc):.2f}] {n / mc:11.0f} | {mc / mf:7.1f}x | "
                  f"{float(first_f[1].mean()):6.1f} | {same}", flush=True)
            env_f.close(); env_c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="least timed duration per path and shape")
    ap.add_argument("--max-reps", type=int, default=50)
    ap.add_argument("--history", type=int, nargs="+", default=None, metavar="H",
                    help="time the history form: observation_history_size on Hover at its defaults [and on lean Circle]")
    ap.add_argument("--reps", type=int, default=5, help="--history: alternating repeats per path and shape")
    args = ap.parse_args()
    if args.history:
        return history_main(args)
    print(f"# evaluate_population on DroneHoverSimpleEnv-v0 (defaults), {torch.cuda.get_device_name(0)}; host clock around a call "
          "that ends in the device-to-host copy of its results; paths alternate; median [min .. max] over reps")
    print("# policy  P x E | fused: ms, reps, episodes/s | composed: ms, reps, episodes/s | composed / fused | mean length | same bits")
    for name in ("early", "late"):
        for P, E in SHAPES:
            pop = population(name, P).to("cuda:0")  # (on the device once: the call's own copy is then none)
            env_f = pds.make("DroneHoverSimpleEnv-v0", num_envs=P * E, seed=1)
            env_c = pds.make("DroneHoverSimpleEnv-v0", num_envs=P * E, seed=1)
            _, first_f = timed(env_f, pop, True)   # warm-up of both paths (and the bitwise comparison: same seed, first call)
            _, first_c = timed(env_c, pop, False)
            same = all(torch.equal(a, b) for a, b in zip(first_f, first_c))
            tf, tc = [], []
            while (sum(tf) < args.seconds or sum(tc) < args.seconds) and len(tc) < args.max_reps:
                tf.append(timed(env_f, pop, True)[0])
                if sum(tc) < args.seconds or len(tc) < 2:
                    tc.append(timed(env_c, pop, False)[0])
            while sum(tf) < args.seconds and len(tf) < 20 * args.max_reps:
                tf.append(timed(env_f, pop, True)[0])
            mf, mc = float(np.median(tf)), float(np.median(tc))
            n = P * E
            print(f"{name:5s} {P:5d} x {E:5d} | {1e3 * mf:9.2f} [{1e3 * min(tf):.2f} .. {1e3 * max(tf):.2f}] {len(tf):4d} {n / mf:12.0f} | "
                  f"{1e3 * mc:10.2f} [{1e3 * min(tc):.2f} .. {1e3 * max(tc):.2f}] {len(tc):3d} {n / mc:11.0f} | {mc / mf:7.1f}x | "
                  f"{float(first_f[1].mean()):6.1f} | {same}", flush=True)
            env_f.close(); env_c.close()


if __name__ == "__main__":
    main()
