#!/usr/bin/env python3
"""What the observation sums of the one-launch evaluation cost (evaluate_population(..., obs_stats=True),
pds_evaluate_policies_stats): the set-up of profiles/tools/evaluate_metrics_bench.py -- Hover at its defaults,
tests/golden/hip_policy_early.npz replicated, the full 500-step limit, P x E = 8 x 128, 64 x 1 024 and 64 x 16 384; after a warm-up
of each shape, --repeats (5) repeats of each of three paths, alternating within one process, the host clock around a call that
ends in a device synchronise:
  fused with metrics and stats / fused with metrics / composed with metrics and stats (the only way to the sums without the kernel).

Nothing here is a bar: the tool records the ratio stats / metrics next to the metrics path's own min-max spread, says where the
stats form is slower than the composed path (exit status 0 either way), and names the team count of each launch, read off the
library's code objects by the launcher's rule (csrc/pds_rollout.h two_teams_fit).

  python profiles/tools/evaluate_stats_bench.py > profiles/evaluate_stats_timing.txt
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_metrics_bench as mb  # noqa: E402  (population, shapes, the variant's name)
import evaluate_names as en  # noqa: E402
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.evaluation import evaluate_population  # noqa: E402


def scratch_of_forms():
    """{(stats form?, teams): scratch bytes per lane} of Hover's default variant in its metrics and its stats form"""
    return en.hover_default_scratch("metrics", "stats")


def timed(env, pop, fused, stats):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate_population(env, pop, fused=fused, metrics=True, obs_stats=stats)  # ends in the copies to the host
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{p}x{e}" for p, e in mb.SHAPES))
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    scratch = scratch_of_forms()
    print(f"# evaluate_population(metrics=True, obs_stats=...) on DroneHoverSimpleEnv-v0 (defaults, 500 steps), hip_policy_early replicated, "
          f"{torch.cuda.get_device_name(0)}")
    print(f"# host clock around a call that ends in a device synchronise; one warm-up per path and shape, then {args.repeats} repeats "
          "of each path, alternating; ms: median [min .. max]")
    print(f"# scratch bytes per lane of Hover's default variant (stats form, teams): {sorted(scratch.items())}")
    slower = []
    for P, E in shapes:
        pop = mb.population(P).to("cuda:0")
        envs = [pds.make("DroneHoverSimpleEnv-v0", num_envs=P * E, seed=1) for _ in range(3)]
        paths = (("fused+stats", envs[0], True, True), ("fused+metrics", envs[1], True, False), ("composed+stats", envs[2], False, True))
        first = {name: timed(env, pop, f, s)[1] for name, env, f, s in paths}  # warm-up; same seed, first call: comparable
        flat = lambda o: [o[0], o[1], o[2], o[3].raw]
        same = all(torch.equal(a, b) for a, b in zip(flat(first["fused+stats"]), flat(first["composed+stats"]))) and \
            torch.equal(first["fused+stats"][4].slab, first["composed+stats"][4].slab) and \
            all(torch.equal(a, b) for a, b in zip(flat(first["fused+stats"]), flat(first["fused+metrics"])))
        t = {name: [] for name, *_ in paths}
        for _ in range(args.repeats):
            for name, env, f, s in paths:
                t[name].append(timed(env, pop, f, s)[0])
        med = {k: float(np.median(v)) for k, v in t.items()}
        tiles = P * E // 64
        spread = (max(t["fused+metrics"]) - min(t["fused+metrics"])) / med["fused+metrics"]
        ratio = med["fused+stats"] / med["fused+metrics"]
        if med["fused+stats"] > med["composed+stats"]:
            slower.append((P, E))
        print(f"{P:3d} x {E:6d} ({tiles:6d} tiles) mean length {float(first['fused+metrics'][1].mean()):6.1f}  same bits {same}")
        for name in t:
            print(f"    {name:17s} {1e3 * med[name]:10.2f} [{1e3 * min(t[name]):.2f} .. {1e3 * max(t[name]):.2f}] ms")
        ts, tm = mb.teams_launched(scratch, True, tiles), mb.teams_launched(scratch, False, tiles)
        print(f"    teams per block: with stats {ts}, metrics only {tm}; stats / metrics = {ratio:.3f}, the metrics path's own (max - min) / "
              f"median = {spread:.3f}; composed / fused, both with stats = {med['composed+stats'] / med['fused+stats']:.1f}x")
        for env in envs:
            env.close()
    print("# the stats form is slower than the composed path at: " + (", ".join(f"{p} x {e}" for p, e in slower) if slower else "no size"))


if __name__ == "__main__":
    main()
