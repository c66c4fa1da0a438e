#!/usr/bin/env python3
"""What the flight-metric accumulators of the one-launch evaluation cost (evaluate_population(..., metrics=True),
pds_evaluate_policies_metrics): Hover at its defaults, tests/golden/hip_policy_early.npz replicated, the full 500-step limit,
P x E = 8 x 128, 64 x 1 024 and 64 x 16 384.  After a warm-up of each shape, --repeats (5) repeats of each of three paths,
alternating within one process, the host clock around a call that ends in a device synchronise:
  fused with metrics / fused without metrics / composed with metrics (what a user has to run without the kernel).

Pass condition (exit status 1 otherwise): at every size the median of "fused with metrics" is not above the median of "composed
with metrics".  Recorded, not a bar: the ratio with / without metrics next to the plain path's own min-max spread, and the team
count of each launch, read off the library's code objects by the launcher's rule (csrc/pds_rollout.h two_teams_fit).

  python profiles/tools/evaluate_metrics_bench.py > profiles/evaluate_metrics_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_names as en  # noqa: E402
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population  # noqa: E402
from phoenix_drone_simulation_amd.ppo import ActorCritic  # noqa: E402

SHAPES = ((8, 128), (64, 1024), (64, 16384))
TWO_TEAMS_ABOVE = 256  # tiles (kRolloutTwoTeamsAbove)


def population(P):
    sd = np.load(os.path.join(ROOT, "tests", "golden", "hip_policy_early.npz"))
    one = PolicyPopulation.from_actor_critics([ActorCritic.from_reference_state_dict({k: sd[k] for k in sd.files})])
    return PolicyPopulation.from_flat(one.theta.expand(P, -1), one.d_in, one.hidden_sizes, one.activation,
                                      one.mean.expand(P, -1), one.std.expand(P, -1), one.eps)


def scratch_of_forms():
    """{(metrics form?, teams): scratch bytes per lane} of Hover's default variant, from the code objects"""
    return en.hover_default_scratch("plain", "metrics")  # (the stats and record forms: profiles/tools/evaluate_{stats,record}_bench.py)


def teams_launched(scratch, metrics, tiles):
    return 2 if tiles > TWO_TEAMS_ABOVE and scratch[(metrics, 2)] <= scratch[(metrics, 1)] else 1


def timed(env, pop, fused, metrics):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate_population(env, pop, fused=fused, metrics=metrics)  # ends in the copies to the host
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{p}x{e}" for p, e in SHAPES))
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    scratch = scratch_of_forms()
    print(f"# evaluate_population(metrics=...) on DroneHoverSimpleEnv-v0 (defaults, 500 steps), hip_policy_early replicated, "
          f"{torch.cuda.get_device_name(0)}")
    print(f"# host clock around a call that ends in a device synchronise; one warm-up per path and shape, then {args.repeats} repeats "
          "of each path, alternating; ms: median [min .. max]")
    print(f"# scratch bytes per lane of Hover's default variant (metrics form, teams): {sorted(scratch.items())}")
    ok = True
    for P, E in shapes:
        pop = population(P).to("cuda:0")
        envs = [pds.make("DroneHoverSimpleEnv-v0", num_envs=P * E, seed=1) for _ in range(3)]
        paths = (("fused+metrics", envs[0], True, True), ("fused", envs[1], True, False), ("composed+metrics", envs[2], False, True))
        first = {name: timed(env, pop, f, m)[1] for name, env, f, m in paths}  # warm-up; same seed, first call: comparable
        same = all(torch.equal(a, b) for a, b in zip(first["fused+metrics"][:3], first["composed+metrics"][:3])) and \
            torch.equal(first["fused+metrics"][3].raw, first["composed+metrics"][3].raw) and \
            all(torch.equal(a, b) for a, b in zip(first["fused+metrics"][:3], first["fused"]))
        t = {name: [] for name, *_ in paths}
        for _ in range(args.repeats):
            for name, env, f, m in paths:
                t[name].append(timed(env, pop, f, m)[0])
        med = {k: float(np.median(v)) for k, v in t.items()}
        tiles = P * E // 64
        spread = (max(t["fused"]) - min(t["fused"])) / med["fused"]
        ratio = med["fused+metrics"] / med["fused"]
        passed = med["fused+metrics"] <= med["composed+metrics"]
        ok &= passed
        print(f"{P:3d} x {E:6d} ({tiles:6d} tiles) mean length {float(first['fused'][1].mean()):6.1f}  same bits {same}")
        for name in t:
            print(f"    {name:17s} {1e3 * med[name]:10.2f} [{1e3 * min(t[name]):.2f} .. {1e3 * max(t[name]):.2f}] ms")
        tm, tp = teams_launched(scratch, True, tiles), teams_launched(scratch, False, tiles)
        print(f"    teams per block: with metrics {tm}, without {tp}; with / without = {ratio:.3f}, the plain path's own (max - min) / median "
              f"= {spread:.3f}; composed / fused, both with metrics = {med['composed+metrics'] / med['fused+metrics']:.1f}x; "
              f"{'PASS' if passed else 'FAIL'}")
        if ratio - 1.0 > spread and tiles >= (1 << 20) // 64:
            print(f"    the ratio exceeds the spread at {P * E} envs; the variant "
                  f"{'FELL from two teams to one' if tm < tp else 'kept its team count'} with the metrics form")
        for env in envs:
            env.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
