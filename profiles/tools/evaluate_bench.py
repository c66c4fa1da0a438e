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

--history H [H] --record R: the record form of the history kernel (pds_evaluate_policies_history_record) on the same envs, actors
and shapes -- evaluate_population(fused=True, history_fused=True, metrics=True, record=R) with and without the observations against
fused=False with the same record (the composed record) and against the history kernel's metrics launch, the same alternating
repeats; then the launches alone, on buffers made beforehand.  Exit status 1 where the fused record is slower than the composed.

  python profiles/tools/evaluate_bench.py --history 4 8 --record 64 > profiles/evaluate_history_record_timing.txt

--history H [H] --obs-stats: the stats form of the history kernel (pds_evaluate_policies_history_stats) on the same envs, actors and
shapes -- evaluate_population(fused=True, history_fused=True, obs_stats=True, history_stats_fused=True, metrics=True) against
fused=False with obs_stats=True (the composed sums) and against the history kernel's metrics launch, the same alternating repeats;
then the two launches alone, on buffers made beforehand.  Exit status 1 where the fused sums are slower than the composed.

  python profiles/tools/evaluate_bench.py --history 4 8 --obs-stats > profiles/evaluate_history_stats_timing.txt

--latency S (with --history, in each of the three forms above): the same envs on the latency ring -- use_latency=True, latency=S,
history_latency=True -- and the launch of include/pds_history_latency_evaluate.h (history_latency_fused=True) against the composed
path, which is what such an env ran before that launch was there.  The metrics form also times the launch alone against the
non-latency history launch of the same shape on an env without the ring, each with its own spread.  Exit status 1 where the launch is
slower than the composed path.

  python profiles/tools/evaluate_bench.py --history 4 8 --latency 0.02 > profiles/evaluate_history_latency_timing.txt

--deep: populations of actors with three and four hidden layers -- seeded random (50, 30, 20) relu and (32, 32, 32, 32) tanh actors
on Hover at its defaults, 500 steps, P x E = 8 x 128 and 64 x 1024: the launch (pds_evaluate_policies_deep) against the composed path
of the same call, against one evaluation.evaluate call per policy on an E-env env (what such actors ran before), and against the
two-hidden-layer launch of a (64, 64) population; medians of --reps alternating synchronised repeats, with their spreads.

  python profiles/tools/evaluate_bench.py --deep > profiles/evaluate_deep_timing.txt

--deep-forms: the stats and the record form of that launch (pds_evaluate_policies_deep_stats / _deep_record,
evaluate_population(..., deep_forms_fused=True)) on the same actors, env and shapes: fused stats / fused metrics / composed stats;
fused record with and without observations / fused metrics / composed record (R = 64); and one learn_one_generation() of a deep
ESTrainer(obs_stats="online") with and without deep_forms_fused; the same alternating repeats.  Exit status 1 where a fused form is
slower than its composed path beyond both spreads.

  python profiles/tools/evaluate_bench.py --deep-forms > profiles/evaluate_deep_forms_timing.txt
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


LATENCY = None  # --latency S: the history forms fly the latency ring


def ring(kw):
    """the env keywords of a history case, on the latency ring where --latency asks for it"""
    return dict(kw, use_latency=True, latency=LATENCY, history_latency=True) if LATENCY is not None else kw


def entry(name):
    """the history entry point `name`, or its twin on the latency ring"""
    return name.replace("pds_evaluate_policies_history", "pds_evaluate_policies_history_latency") if LATENCY is not None else name


def timed(env, pop, fused, history_fused=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate_population(env, pop, fused=fused, history_fused=history_fused,
                              history_latency_fused=LATENCY is not None)  # ends in the copies to the host: synchronised
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
    ok = True
    for j, (label, env_id, kw) in enumerate(HISTORY_CASES):
        H = args.history[min(j, len(args.history) - 1)]
        for P, E in HISTORY_SHAPES:
            env_f = pds.make(env_id, num_envs=P * E, seed=1, observation_history_size=H, **ring(kw))
            env_c = pds.make(env_id, num_envs=P * E, seed=1, observation_history_size=H, **ring(kw))
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
            ok &= mf <= mc
            if LATENCY is not None:  # the launch alone, on the ring and on an env without it
                env_n = pds.make(env_id, num_envs=P * E, seed=1, observation_history_size=H, **kw)
                T, dev = env_f._max_episode_steps, env_f.device
                bufs = tuple(torch.zeros(n, device=dev) for _ in range(3)) + (torch.zeros(n, 8, device=dev), None)
                k = {"ring": [], "no ring": []}
                for rep_ in range(args.reps + 1):  # (the first round warms up)
                    for which, env, name in (("ring", env_f, entry("pds_evaluate_policies_history")), ("no ring", env_n, "pds_evaluate_policies_history")):
                        ms = history_stats_launch_ms(env, pop, H, P, E, T, bufs, "metrics", name)
                        if rep_:
                            k[which].append(ms)
                kmed = {w: float(np.median(v)) for w, v in k.items()}
                spread = {w: (max(v) - min(v)) / kmed[w] for w, v in k.items()}
                ratio = kmed["ring"] / kmed["no ring"]
                print("    the launch alone: " + ", ".join(f"{w} {kmed[w]:.3f} [{min(k[w]):.3f} .. {max(k[w]):.3f}] ms, (max - min) / median = {spread[w]:.3f}"
                                                           for w in k) + f"; ring / no ring = {ratio:.3f}: " +
                      ("outside both spreads" if abs(ratio - 1.0) > max(spread.values()) else "inside the spread") +
                      " (the flights differ: the ring delays the actions)", flush=True)
                env_n.close()
            env_f.close(); env_c.close()
    if LATENCY is not None:
        sys.exit(0 if ok else 1)


def timed_record(env, pop, fused, kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = evaluate_population(env, pop, fused=fused, history_fused=bool(fused), metrics=True, history_latency_fused=LATENCY is not None,
                              **kw)  # ends in the copies to the host
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def history_launch_ms(env, pop, H, P, E, T, R, bufs, form):
    """device time of ONE launch of the history kernel on buffers made beforehand: form "metrics", "record" (no observations),
    "record+obs", or "record+obs dword" -- the observations into a buffer 4 bytes off a 16-byte boundary, where the kernel copies
    them with dword stores whatever the history size"""
    from phoenix_drone_simulation_amd import native
    obs, _ = env.reset()
    obs = obs.contiguous()
    ret, length, cost, raw, flight, obs_rec = bufs
    where = {"record+obs": obs_rec[4:], "record+obs dword": obs_rec[1:-3], "record": None}
    trail = (raw,) if form == "metrics" else (raw, R, flight, where[form])
    name = entry("pds_evaluate_policies_history" if form == "metrics" else "pds_evaluate_policies_history_record")
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    native.call(name, env._handle, H, P, E, pop.mlp(0), pop.theta, pop.mean, pop.std, pop.eps, T, obs, ret, length, cost, *trail,
                on=env.device, handle=env._handle)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def history_record_main(args):
    """--history H [H] --record R: the record form of the history kernel (pds_evaluate_policies_history_record), with and without
    the observations, against the composed record and against the history kernel's metrics launch; the launches alone as well"""
    R = args.record
    print(f"# evaluate_population(history_fused=True, metrics=True, record={R}) on envs with an observation history, "
          f"{torch.cuda.get_device_name(0)}; seeded random tanh actors (64, 64)")
    print(f"# host clock around a call that ends in a device synchronise; one warm-up per path and shape, then {args.reps} repeats of each "
          "path, alternating; ms: median [min .. max]")
    ok = True
    for j, (label, env_id, kw) in enumerate(HISTORY_CASES):
        H = args.history[min(j, len(args.history) - 1)]
        for P, E in HISTORY_SHAPES:
            envs = [pds.make(env_id, num_envs=P * E, seed=1, observation_history_size=H, **ring(kw)) for _ in range(4)]
            pop = random_population(envs[0].obs_dim, P).to("cuda:0")
            big = dict(record=R, record_limit_bytes=1 << 32)  # (64 policies x 64 episodes x 500 steps x 160 inputs: 1.4 GB)
            paths = (("fused record+obs", envs[0], True, big), ("fused record", envs[1], True, dict(big, record_observations=False)),
                     ("fused metrics", envs[2], True, {}), ("composed record+obs", envs[3], False, big))
            first = {name: timed_record(env, pop, f, k)[1] for name, env, f, k in paths}  # warm-up; same seed, first call: comparable
            a, b, m = first["fused record+obs"], first["composed record+obs"], first["fused metrics"]
            same = all(torch.equal(x, y) for x, y in zip(list(a[:3]) + [a[3].raw, a[4].state, a[4].action, a[4].observation],
                                                          list(b[:3]) + [b[3].raw, b[4].state, b[4].action, b[4].observation])) and \
                all(torch.equal(x, y) for x, y in zip(list(a[:3]) + [a[3].raw], list(m[:3]) + [m[3].raw]))
            t = {name: [] for name, *_ in paths}
            for _ in range(args.reps):
                for name, env, f, k in paths:
                    t[name].append(timed_record(env, pop, f, k)[0])
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = (max(t["fused metrics"]) - min(t["fused metrics"])) / med["fused metrics"]
            passed = med["fused record+obs"] <= med["composed record+obs"]
            ok &= passed
            print(f"{label} H = {H} ({envs[0].obs_dim} inputs) {P:3d} x {E:5d} ({P * E // 64} tiles, {P * R} recorded envs) mean length "
                  f"{float(m[1].mean()):6.1f}  same bits {same}")
            for name in t:
                print(f"    {name:20s} {1e3 * med[name]:10.2f} [{1e3 * min(t[name]):.2f} .. {1e3 * max(t[name]):.2f}] ms")
            print(f"    record+obs / metrics = {med['fused record+obs'] / med['fused metrics']:.3f}, record / metrics = "
                  f"{med['fused record'] / med['fused metrics']:.3f}, the metrics path's own (max - min) / median = {spread:.3f}; "
                  f"composed / fused, both recording = {med['composed record+obs'] / med['fused record+obs']:.1f}x; {'PASS' if passed else 'FAIL'}")
            n, T, dev = P * E, envs[0]._max_episode_steps, envs[0].device
            bufs = (torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, 8, device=dev),
                    torch.zeros(T, 4, P * R, 4, device=dev), torch.zeros(T * P * R * envs[0].obs_dim + 4, device=dev))
            assert bufs[5].data_ptr() % 16 == 0
            del first, a, b, m
            forms = ("record+obs", "record+obs dword", "record", "metrics")
            k = {f: [] for f in forms}
            for rep_ in range(args.reps + 1):  # (the first round warms up)
                for f in forms:
                    ms = history_launch_ms(envs[2], pop, H, P, E, T, R, bufs, f)
                    if rep_:
                        k[f].append(ms)
            kmed = {f: float(np.median(v)) for f, v in k.items()}
            kspread = (max(k["metrics"]) - min(k["metrics"])) / kmed["metrics"]
            k_obs, k_state = kmed["record+obs"] / kmed["metrics"], kmed["record"] / kmed["metrics"]
            print("    the launch alone: " + ", ".join(f"{f} {kmed[f]:.3f} [{min(k[f]):.3f} .. {max(k[f]):.3f}]" for f in forms) +
                  f" ms; record+obs / metrics = {k_obs:.3f}, record+obs dword / metrics = {kmed['record+obs dword'] / kmed['metrics']:.3f}, "
                  f"record / metrics = {k_state:.3f}, the metrics launch's own (max - min) / median = {kspread:.3f}")
            if k_obs - 1.0 > kspread:
                which = "the state stores (the env wave's) already exceed it" if k_state - 1.0 > kspread else \
                    "the observation copy (the network waves') carries it: without it the ratio is inside the spread"
                print(f"    the launch's record+obs / metrics exceeds the spread: {which}")
            else:
                print("    the launch's record+obs / metrics is inside the spread")
            for env in envs:
                env.close()
    sys.exit(0 if ok else 1)


def history_stats_launch_ms(env, pop, H, P, E, T, bufs, form, name=None):
    """device time of ONE launch of the history kernel on buffers made beforehand: form "metrics" or "stats"; `name`: the entry
    point where it is not the form's own (on the ring with --latency)"""
    from phoenix_drone_simulation_amd import native
    obs, _ = env.reset()
    obs = obs.contiguous()
    ret, length, cost, raw, slab = bufs
    own, trail = ("pds_evaluate_policies_history", (raw,)) if form == "metrics" else ("pds_evaluate_policies_history_stats", (raw, slab))
    name = name or entry(own)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    native.call(name, env._handle, H, P, E, pop.mlp(0), pop.theta, pop.mean, pop.std, pop.eps, T, obs, ret, length, cost, *trail,
                on=env.device, handle=env._handle)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end)


def history_stats_main(args):
    """--history H [H] --obs-stats: the stats form of the history kernel against the composed sums and against the history
    kernel's metrics launch; the launches alone as well"""
    from phoenix_drone_simulation_amd.evaluation import fused_history_latency_stats_evaluation_built, fused_history_stats_evaluation_built, slab_features
    print(f"# evaluate_population(history_fused=True, obs_stats=True, history_stats_fused=True, metrics=True) on envs with an observation "
          f"history, {torch.cuda.get_device_name(0)}; seeded random tanh actors (64, 64)")
    print(f"# host clock around a call that ends in a device synchronise; one warm-up per path and shape, then {args.reps} repeats of each "
          "path, alternating; ms: median [min .. max]")
    ok = True
    for j, (label, env_id, kw) in enumerate(HISTORY_CASES):
        H = args.history[min(j, len(args.history) - 1)]
        for P, E in HISTORY_SHAPES:
            envs = [pds.make(env_id, num_envs=P * E, seed=1, observation_history_size=H, **ring(kw)) for _ in range(3)]
            if not (fused_history_latency_stats_evaluation_built if LATENCY is not None else fused_history_stats_evaluation_built)(envs[0]):
                print(f"{label} H = {H} ({envs[0].obs_dim} inputs): the stats form is not built for this width")
                continue
            pop = random_population(envs[0].obs_dim, P).to("cuda:0")
            stats = dict(obs_stats=True, history_stats_fused=True)
            paths = (("fused stats", envs[0], True, stats), ("fused metrics", envs[1], True, {}), ("composed stats", envs[2], False, stats))
            first = {name: timed_record(env, pop, f, k)[1] for name, env, f, k in paths}  # warm-up; same seed, first call: comparable
            a, b, m = first["fused stats"], first["composed stats"], first["fused metrics"]
            same = all(torch.equal(x, y) for x, y in zip(list(a[:3]) + [a[3].raw, a[4].slab], list(b[:3]) + [b[3].raw, b[4].slab])) and \
                all(torch.equal(x, y) for x, y in zip(list(a[:3]) + [a[3].raw], list(m[:3]) + [m[3].raw]))
            t = {name: [] for name, *_ in paths}
            for _ in range(args.reps):
                for name, env, f, k in paths:
                    t[name].append(timed_record(env, pop, f, k)[0])
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = (max(t["fused metrics"]) - min(t["fused metrics"])) / med["fused metrics"]
            passed = med["fused stats"] <= med["composed stats"]
            ok &= passed
            W = slab_features(envs[0].obs_dim)
            print(f"{label} H = {H} ({envs[0].obs_dim} inputs, slab width {W}) {P:3d} x {E:5d} ({P * E // 64} tiles) mean length "
                  f"{float(m[1].mean()):6.1f}  same bits {same}")
            for name in t:
                print(f"    {name:20s} {1e3 * med[name]:10.2f} [{1e3 * min(t[name]):.2f} .. {1e3 * max(t[name]):.2f}] ms")
            print(f"    stats / metrics = {med['fused stats'] / med['fused metrics']:.3f}, the metrics path's own (max - min) / median = {spread:.3f}; "
                  f"composed / fused, both summing = {med['composed stats'] / med['fused stats']:.1f}x; {'PASS' if passed else 'FAIL'}")
            n, T, dev = P * E, envs[0]._max_episode_steps, envs[0].device
            bufs = tuple(torch.zeros(n, device=dev) for _ in range(3)) + (torch.zeros(n, 8, device=dev), torch.zeros(n // 64, 4, 2, W, device=dev))
            del first, a, b, m
            forms = ("stats", "metrics")
            k = {f: [] for f in forms}
            for rep_ in range(args.reps + 1):  # (the first round warms up)
                for f in forms:
                    ms = history_stats_launch_ms(envs[1], pop, H, P, E, T, bufs, f)
                    if rep_:
                        k[f].append(ms)
            kmed = {f: float(np.median(v)) for f, v in k.items()}
            kspread = (max(k["metrics"]) - min(k["metrics"])) / kmed["metrics"]
            ratio = kmed["stats"] / kmed["metrics"]
            print("    the launch alone: " + ", ".join(f"{f} {kmed[f]:.3f} [{min(k[f]):.3f} .. {max(k[f]):.3f}]" for f in forms) +
                  f" ms; stats / metrics = {ratio:.3f}, the metrics launch's own (max - min) / median = {kspread:.3f}: "
                  + ("the sums exceed the spread" if ratio - 1.0 > kspread else "the sums are inside the spread"))
            for env in envs:
                env.close()
    sys.exit(0 if ok else 1)


DEEP_ACTORS = (((50, 30, 20), "relu"), ((32, 32, 32, 32), "tanh"))


def deep_population(d_in, P, hidden, activation, seed=0):
    """seeded actors with len(hidden) hidden layers in torch's nn.Linear initialisation, output biases spread as random_population's"""
    g = torch.Generator().manual_seed(seed)
    sizes = (d_in,) + tuple(hidden) + (4,)
    blocks = [(n_in, count) for n_in, n_out in zip(sizes[:-1], sizes[1:]) for count in (n_out * n_in, n_out)]
    theta = torch.cat([(torch.rand(P, count, generator=g) * 2 - 1) / fan_in ** 0.5 for fan_in, count in blocks], dim=1)
    theta[:, -4:] += torch.linspace(-0.6, 0.6, P).unsqueeze(1) if P > 1 else -0.3
    return PolicyPopulation.from_flat(theta, d_in, hidden, activation)


def deep_main(args):
    """--deep: pds_evaluate_policies_deep (evaluate_population(fused=True) on a population with three / four hidden layers) against
    the composed path of the same call (fused=False: pds_mlp_deep_forward per policy and step), against what such a population
    could run before either was there -- one evaluation.evaluate call per policy on an E-env env, the actor as PyTorch ops -- and,
    for scale, against the two-hidden-layer launch of a (64, 64) population.  Hover at its defaults, 500 steps."""
    from phoenix_drone_simulation_amd.evaluation import evaluate, fused_deep_evaluation_built
    env_id = "DroneHoverSimpleEnv-v0"
    print(f"# evaluate_population on a population of actors with three / four hidden layers, {env_id} at its defaults (500 steps), "
          f"{torch.cuda.get_device_name(0)}; seeded random actors")
    print(f"# host clock around work that ends in a device synchronise; one warm-up per side and shape, then {args.reps} repeats of each "
          "side, alternating; ms: median [min .. max]; spread = (max - min) / median")
    for hidden, activation in DEEP_ACTORS:
        for P, E in HISTORY_SHAPES:
            envs = [pds.make(env_id, num_envs=P * E, seed=1) for _ in range(3)]
            env_one = pds.make(env_id, num_envs=E, seed=1)
            pop = deep_population(envs[0].obs_dim, P, hidden, activation).to("cuda:0")
            two = random_population(envs[0].obs_dim, P).to("cuda:0")
            assert fused_deep_evaluation_built(envs[0], pop)
            actors = [pop.policy(p).to("cuda:0") for p in range(P)]

            def per_policy():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = [evaluate(env_one, a) for a in actors]  # (each ends in its copies to the host)
                return time.perf_counter() - t0, out

            sides = (("launch", lambda: timed(envs[0], pop, True)), ("composed", lambda: timed(envs[1], pop, False)),
                     ("per-policy evaluate", per_policy), ("two-hidden-layer launch (64, 64)", lambda: timed(envs[2], two, True)))
            first = {name: f()[1] for name, f in sides}  # warm-up; the first calls of same-seed envs: comparable
            same = all(torch.equal(x, y) for x, y in zip(first["launch"], first["composed"]))
            t = {name: [] for name, _ in sides}
            for _ in range(args.reps):
                for name, f in sides:
                    t[name].append(f()[0])
            med = {k: float(np.median(v)) for k, v in t.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
            print(f"{hidden} {activation} {P:3d} x {E:5d} ({P * E // 64} tiles) mean length {float(first['launch'][1].mean()):6.1f}  "
                  f"launch and composed: same bits {same}")
            for name in t:
                print(f"    {name:34s} {1e3 * med[name]:10.2f} [{1e3 * min(t[name]):.2f} .. {1e3 * max(t[name]):.2f}] ms  spread {spread[name]:.3f}  "
                      f"{P * E / med[name]:12.0f} episodes/s")
            r = med["composed"] / med["launch"]
            verdict = "the launch is faster beyond both spreads" if r - 1.0 > max(spread["launch"], spread["composed"]) else \
                ("the launch is SLOWER beyond both spreads" if 1.0 / r - 1.0 > max(spread["launch"], spread["composed"]) else "inside the spreads")
            print(f"    composed / launch = {r:.2f}x ({verdict}); per-policy evaluate / launch = {med['per-policy evaluate'] / med['launch']:.1f}x; "
                  f"launch / two-hidden-layer launch = {med['launch'] / med['two-hidden-layer launch (64, 64)']:.2f}x", flush=True)
            for env in envs + [env_one]:
                env.close()


def deep_forms_main(args):
    """--deep-forms: the stats and the record form of the deep launch against the composed path of the same call and against the
    deep metrics launch; one generation of a deep ESTrainer(obs_stats="online") with and without deep_forms_fused"""
    from phoenix_drone_simulation_amd.es import ESTrainer
    from phoenix_drone_simulation_amd.evaluation import fused_deep_forms_evaluation_built
    env_id, R = "DroneHoverSimpleEnv-v0", 64
    print(f"# evaluate_population(deep_forms_fused=True) on a population of actors with three / four hidden layers, {env_id} at its "
          f"defaults (500 steps), {torch.cuda.get_device_name(0)}; seeded random actors; record = {R}")
    print(f"# host clock around work that ends in a device synchronise; one warm-up per side and shape, then {args.reps} repeats of each "
          "side, alternating; ms: median [min .. max]; spread = (max - min) / median")
    ok = True

    def fly(env, pop, fused, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = evaluate_population(env, pop, fused=fused, metrics=True, deep_forms_fused=fused is True, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def rounds(sides):
        first = {name: f()[1] for name, f in sides}  # warm-up; the first calls of same-seed envs: comparable
        t = {name: [] for name, _ in sides}
        for _ in range(args.reps):
            for name, f in sides:
                t[name].append(f()[0])
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
        for name in t:
            print(f"    {name:34s} {1e3 * med[name]:10.2f} [{1e3 * min(t[name]):.2f} .. {1e3 * max(t[name]):.2f}] ms  spread {spread[name]:.3f}")
        return first, med, spread

    def verdict(med, spread, fused, composed):
        r, s = med[composed] / med[fused], max(spread[fused], spread[composed])
        return r, ("the launch is faster beyond both spreads" if r - 1.0 > s else
                   "the launch is SLOWER beyond both spreads" if 1.0 / r - 1.0 > s else "inside the spreads")

    for hidden, activation in DEEP_ACTORS:
        for P, E in HISTORY_SHAPES:
            envs = [pds.make(env_id, num_envs=P * E, seed=1) for _ in range(6)]
            pop = deep_population(envs[0].obs_dim, P, hidden, activation).to("cuda:0")
            assert fused_deep_forms_evaluation_built(envs[0], pop, "stats") and fused_deep_forms_evaluation_built(envs[0], pop, "record")
            big = dict(record=R, record_limit_bytes=1 << 32)
            print(f"{hidden} {activation} {P:3d} x {E:5d} ({P * E // 64} tiles, {P * R} recorded envs)")
            # (two groups of rounds: a side that follows a recording one pays for the return of its arrays to the allocators)
            first, med, spread = rounds((("fused stats", lambda: fly(envs[0], pop, True, obs_stats=True)),
                                         ("fused metrics", lambda: fly(envs[1], pop, True)),
                                         ("composed stats", lambda: fly(envs[2], pop, False, obs_stats=True))))
            for got, into in zip(rounds((("fused record+obs", lambda: fly(envs[3], pop, True, **big)),
                                         ("fused record", lambda: fly(envs[4], pop, True, record_observations=False, **big)),
                                         ("composed record+obs", lambda: fly(envs[5], pop, False, **big)))), (first, med, spread)):
                into.update(got)
            a, b, m, ra, rb = (first[k] for k in ("fused stats", "composed stats", "fused metrics", "fused record+obs", "composed record+obs"))
            base = lambda o: list(o[:3]) + [o[3].raw]
            same = all(torch.equal(x, y) for x, y in zip(base(a) + [a[4].slab], base(b) + [b[4].slab])) and \
                all(torch.equal(x, y) for x, y in zip(base(a), base(m))) and \
                all(torch.equal(x, y) for x, y in zip(base(ra) + [ra[4].state, ra[4].action, ra[4].observation],
                                                      base(rb) + [rb[4].state, rb[4].action, rb[4].observation]))
            rs, vs = verdict(med, spread, "fused stats", "composed stats")
            rr, vr = verdict(med, spread, "fused record+obs", "composed record+obs")
            ok &= "SLOWER" not in vs and "SLOWER" not in vr
            print(f"    mean length {float(m[1].mean()):6.1f}  same bits {same}; composed / fused: stats {rs:.1f}x ({vs}), record+obs {rr:.1f}x ({vr})")
            print(f"    over the metrics launch: stats {med['fused stats'] / med['fused metrics']:.3f}, record+obs "
                  f"{med['fused record+obs'] / med['fused metrics']:.3f}, record {med['fused record'] / med['fused metrics']:.3f}; the metrics "
                  f"launch's own spread {spread['fused metrics']:.3f}", flush=True)
            del first, a, b, m, ra, rb
            for env in envs[2:]:
                env.close()
            trainers = {name: ESTrainer(env, P, hidden_sizes=hidden, activation=activation, seed=3, obs_stats="online", eval_every=0,
                                        deep_forms_fused=dff) for name, env, dff in (("generation, deep_forms_fused", envs[0], True),
                                                                                     ("generation, composed sums", envs[1], False))}
            first, med, spread = rounds(tuple((name, (lambda tr: lambda: (tr.learn_one_generation()["t_evaluate"], None))(tr))
                                              for name, tr in trainers.items()))
            rg, vg = verdict(med, spread, "generation, deep_forms_fused", "generation, composed sums")
            ok &= "SLOWER" not in vg
            print(f"    (t_evaluate of learn_one_generation) composed / fused: {rg:.1f}x ({vg})", flush=True)
            for env in envs[:2]:
                env.close()
    sys.exit(0 if ok else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deep", action="store_true",
                    help="time the launch for actors with three / four hidden layers (pds_evaluate_policies_deep) against its composed "
                         "path, one evaluation.evaluate per policy and the two-hidden-layer launch")
    ap.add_argument("--deep-forms", action="store_true",
                    help="time the stats and the record form of that launch (pds_evaluate_policies_deep_stats / _deep_record) against "
                         "their composed paths and the metrics launch, and a generation of a deep ESTrainer(obs_stats='online')")
    ap.add_argument("--seconds", type=float, default=1.0, help="least timed duration per path and shape")
    ap.add_argument("--max-reps", type=int, default=50)
    ap.add_argument("--history", type=int, nargs="+", default=None, metavar="H",
                    help="time the history form: observation_history_size on Hover at its defaults [and on lean Circle]")
    ap.add_argument("--reps", type=int, default=5, help="--history: alternating repeats per path and shape")
    ap.add_argument("--record", type=int, default=None, metavar="R",
                    help="--history: time the record form (pds_evaluate_policies_history_record, R episodes per policy) instead")
    ap.add_argument("--obs-stats", action="store_true",
                    help="--history: time the stats form (pds_evaluate_policies_history_stats) instead")
    ap.add_argument("--latency", type=float, default=None, metavar="S",
                    help="--history: the envs on the latency ring (use_latency=True, latency=S, history_latency=True) and the launch of "
                         "include/pds_history_latency_evaluate.h against the composed path")
    args = ap.parse_args()
    if args.latency is not None:
        if not args.history:
            ap.error("--latency needs --history")
        global LATENCY
        LATENCY = args.latency
    if args.deep_forms:
        return deep_forms_main(args)
    if args.deep:
        return deep_main(args)
    if args.history and args.obs_stats:
        return history_stats_main(args)
    if args.history and args.record:
        return history_record_main(args)
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
