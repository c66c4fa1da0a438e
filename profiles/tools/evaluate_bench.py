#!/usr/bin/env python3
"""Times evaluate_population(fused=True) -- one launch -- against fused=False, the composed path out of entry points that were
there before the kernel (per step one pds_mlp_forward per policy + pds_step + five elementwise ops): the baseline.

Both paths run in ONE process and alternate; every shape is warmed up first; the host clock runs around work that ends in a
device synchronise (the results come back to the host); each path of each shape is timed for at least --seconds and the
spread over its repeats is printed.  Shapes, on Hover at its defaults: P x E = 1 x 8192, 64 x 128, 1024 x 64, each with
tests/golden/hip_policy_early.npz (episodes end by falling) and hip_policy_late.npz (episodes run to the TimeLimit).

  python profiles/tools/evaluate_bench.py > profiles/evaluate_timing.txt
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


def timed(env, pop, fused):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate_population(env, pop, fused=fused)  # ends in the copies to the host: synchronised
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="least timed duration per path and shape")
    ap.add_argument("--max-reps", type=int, default=50)
    args = ap.parse_args()
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
