#!/usr/bin/env python3
"""What recording the flights costs the one-launch evaluation (evaluate_population(..., record=64),
pds_evaluate_policies_record): Hover at its defaults, tests/golden/hip_policy_early.npz replicated, the full 500-step limit,
P x E = 8 x 128, 64 x 1 024 and 64 x 16 384, R = 64 recorded episodes per policy.  After a warm-up of each shape, --repeats (5)
repeats of each of four paths, alternating within one process, the host clock around a call that ends in a device synchronise:
  fused record with observations / fused record without observations / fused metrics (the kernel without a record: the
  baseline) / composed record (what a user has to run without the kernel).

A call with record= also allocates and zero-fills the record, transposes it on the device and copies it to the host (200 B per
recorded env-step here), so next to the calls the tool times the LAUNCHES alone -- pds_evaluate_policies_record with and without
d_obs_rec and pds_evaluate_policies_metrics on buffers made beforehand, device events around the one entry point, the env reset in
front of each and outside the timing: that difference is what the stores cost the kernel.

Pass condition (exit status 1 otherwise): at every size the median of "fused record with observations" is not above the median
of "composed record".  Recorded, not a bar: the ratios record / metrics of the calls and of the launches alone, each next to
the metrics path's own min-max spread -- where a launch ratio exceeds it, the line says which store carries the excess, state
(the env wave's, in both record launches) or observation (the network waves', in the first only) -- and the team count of each
launch, read off the library's code objects by the launcher's rule (csrc/pds_rollout.h two_teams_fit).

  python profiles/tools/evaluate_record_bench.py > profiles/evaluate_record_timing.txt
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
from evaluate_metrics_bench import SHAPES, TWO_TEAMS_ABOVE, population  # noqa: E402
from phoenix_drone_simulation_amd import native  # noqa: E402
from phoenix_drone_simulation_amd.evaluation import evaluate_population  # noqa: E402

R = 64


def scratch_of_forms():
    """{(record form?, teams): scratch bytes per lane} of Hover's default variant, metrics and record form, from the code objects"""
    return en.hover_default_scratch("metrics", "record")


def teams_launched(scratch, record, tiles):
    return 2 if tiles > TWO_TEAMS_ABOVE and scratch[(record, 2)] <= scratch[(record, 1)] else 1


def timed(env, pop, fused, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate_population(env, pop, fused=fused, metrics=True, **kw)  # ends in the copies to the host
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def launch_ms(env, pop, P, E, T, bufs, form):
    """device time of ONE launch on buffers made beforehand: form "metrics", "record" (no observations) or "record+obs" """
    obs, _ = env.reset()
    ret, length, cost, raw, flight, obs_rec = bufs
    trail = (raw,) if form == "metrics" else (raw, R, flight, obs_rec if form == "record+obs" else None)
    name = "pds_evaluate_policies_metrics" if form == "metrics" else "pds_evaluate_policies_record"
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    native.call(name, env._handle, P, E, pop.mlp(0), pop.theta, pop.mean, pop.std, pop.eps, T, obs, ret, length, cost, *trail,
                on=env.device, handle=env._handle)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(f"{p}x{e}" for p, e in SHAPES))
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    scratch = scratch_of_forms()
    print(f"# evaluate_population(metrics=True, record={R}) on DroneHoverSimpleEnv-v0 (defaults, 500 steps), hip_policy_early replicated, "
          f"{torch.cuda.get_device_name(0)}")
    print(f"# host clock around a call that ends in a device synchronise; one warm-up per path and shape, then {args.repeats} repeats "
          "of each path, alternating; ms: median [min .. max]")
    print(f"# scratch bytes per lane of Hover's default variant (record form, teams): {sorted(scratch.items())}")
    ok = True
    for P, E in shapes:
        pop = population(P).to("cuda:0")
        envs = [pds.make("DroneHoverSimpleEnv-v0", num_envs=P * E, seed=1) for _ in range(4)]
        paths = (("fused record+obs", envs[0], True, dict(record=R)), ("fused record", envs[1], True, dict(record=R, record_observations=False)),
                 ("fused metrics", envs[2], True, {}), ("composed record+obs", envs[3], False, dict(record=R)))
        first = {name: timed(env, pop, f, kw)[1] for name, env, f, kw in paths}  # warm-up; same seed, first call: comparable
        a, b, m = first["fused record+obs"], first["composed record+obs"], first["fused metrics"]
        same = all(torch.equal(x, y) for x, y in zip(list(a[:3]) + [a[3].raw, a[4].state, a[4].action, a[4].observation],
                                                      list(b[:3]) + [b[3].raw, b[4].state, b[4].action, b[4].observation])) and \
            all(torch.equal(x, y) for x, y in zip(list(a[:3]) + [a[3].raw], list(m[:3]) + [m[3].raw]))
        t = {name: [] for name, *_ in paths}
        for _ in range(args.repeats):
            for name, env, f, kw in paths:
                t[name].append(timed(env, pop, f, kw)[0])
        med = {k: float(np.median(v)) for k, v in t.items()}
        tiles = P * E // 64
        spread = (max(t["fused metrics"]) - min(t["fused metrics"])) / med["fused metrics"]
        r_obs, r_state = med["fused record+obs"] / med["fused metrics"], med["fused record"] / med["fused metrics"]
        passed = med["fused record+obs"] <= med["composed record+obs"]
        ok &= passed
        print(f"{P:3d} x {E:6d} ({tiles:6d} tiles, {P * R} recorded envs) mean length {float(m[1].mean()):6.1f}  same bits {same}")
        for name in t:
            print(f"    {name:20s} {1e3 * med[name]:10.2f} [{1e3 * min(t[name]):.2f} .. {1e3 * max(t[name]):.2f}] ms")
        print(f"    teams per block: record form {teams_launched(scratch, True, tiles)}, metrics form {teams_launched(scratch, False, tiles)}; "
              f"record+obs / metrics = {r_obs:.3f}, record / metrics = {r_state:.3f}, the metrics path's own (max - min) / median = {spread:.3f}; "
              f"composed / fused, both recording = {med['composed record+obs'] / med['fused record+obs']:.1f}x; {'PASS' if passed else 'FAIL'}")
        n, T, dev = P * E, envs[0]._max_episode_steps, envs[0].device
        bufs = (torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, 8, device=dev),
                torch.zeros(T, 4, P * R, 4, device=dev), torch.zeros(T, P * R, envs[0].obs_dim, device=dev))
        forms = ("record+obs", "record", "metrics")
        k = {f: [] for f in forms}
        for rep_ in range(args.repeats + 1):  # (the first round warms up)
            for f in forms:
                ms = launch_ms(envs[2], pop, P, E, T, bufs, f)
                if rep_:
                    k[f].append(ms)
        kmed = {f: float(np.median(v)) for f, v in k.items()}
        kspread = (max(k["metrics"]) - min(k["metrics"])) / kmed["metrics"]
        k_obs, k_state = kmed["record+obs"] / kmed["metrics"], kmed["record"] / kmed["metrics"]
        print("    the launch alone: " + ", ".join(f"{f} {kmed[f]:.2f} [{min(k[f]):.2f} .. {max(k[f]):.2f}]" for f in forms) +
              f" ms; record+obs / metrics = {k_obs:.3f}, record / metrics = {k_state:.3f}, the metrics launch's own (max - min) / median = {kspread:.3f}")
        if k_obs - 1.0 > kspread:
            which = "the state stores (the env wave's) already exceed it" if k_state - 1.0 > kspread else \
                "the observation stores (the network waves') carry it: without them the ratio is inside the spread"
            print(f"    the launch's record+obs / metrics exceeds the spread at {P * E} envs, R = {R}: {which}")
        else:
            print(f"    the launch's record+obs / metrics is inside the spread at {P * E} envs, R = {R}")
        for env in envs:
            env.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
