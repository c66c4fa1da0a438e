#!/usr/bin/env python3
"""Times one generation of ESTrainer (es.py) and records whether its centre learns.

Timing: Hover lean (no observation noise, domain randomisation or thrust noise) and Hover at the reference's defaults, both at
P = 4096 policies x E = 64 episodes (262 144 envs), split into perturb / evaluate / gradient + Adam with device events; one
warm-up generation first, then --reps generations, median [min .. max].  The evaluate span is the whole evaluate_population call
(reset, the one launch, the copies of its results to the host).  Below that the two kernels alone, back to back, with the bytes
pds_es_perturb writes over its time.

Learning: the centre's return (the centre alone on all envs) per generation for three seeds on Hover lean, defaults of ESTrainer
and a random-action warm-up of the observation statistics.  Recorded, not tuned.

  python profiles/tools/es_bench.py --timing-out profiles/es_timing.txt --learning-out profiles/es_learning.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.es import ESTrainer  # noqa: E402
from phoenix_drone_simulation_amd.evaluation import evaluate_population  # noqa: E402

LEAN = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0)
P, E = 4096, 64


def spans(fn_list):
    """run the callables in order, a device event between each two -> milliseconds per callable"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(fn_list) + 1)]
    out = []
    ev[0].record()
    for k, fn in enumerate(fn_list):
        out.append(fn())
        ev[k + 1].record()
    torch.cuda.synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(len(fn_list))], out


def fmt(xs):
    return f"{float(np.median(xs)):9.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


def time_generation(name, env_kw, reps, out):
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=P * E, seed=1, **env_kw)
    tr = ESTrainer(env, P, seed=0, obs_stats="warmup", eval_every=0)
    state = {}

    def ask():
        state["pop"] = tr.ask()

    def evaluate():
        ret, length, _ = evaluate_population(env, state["pop"], fused="auto")
        state["fitness"], state["len"] = ret.mean(dim=1), float(length.mean())

    def tell():
        tr.tell(state["fitness"])

    spans([ask, evaluate, tell])  # warm-up generation
    rows = [spans([ask, evaluate, tell])[0] for _ in range(reps)]
    a, e, t = (list(col) for col in zip(*rows))
    print(f"{name:18s} P {P} x E {E}, n {tr.n}, mean episode length {state['len']:6.1f} | perturb ms {fmt(a)} | evaluate ms {fmt(e)} | "
          f"gradient + Adam ms {fmt(t)} | {reps} generations", file=out, flush=True)
    env.close()


def time_kernels(pop, n, reps, out):
    lib, H, dev = pds.native.load(), pop // 2, "cuda:0"
    mu, theta = torch.randn(n, device=dev), torch.empty(pop, n, device=dev)
    w, grad = torch.randn(H, device=dev), torch.empty(n, device=dev)
    ws = torch.empty(lib.pds_es_workspace_floats(n, H), device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def perturb():
        assert lib.pds_es_perturb(p(mu), n, H, 0.02, 1, 0, 0, p(theta), st) == 0

    def gradient():
        assert lib.pds_es_gradient(p(w), p(mu), n, H, -1.0, 0.005, 1, 0, 0, p(grad), p(ws), st) == 0

    spans([perturb, gradient])
    rows = [spans([perturb, gradient])[0] for _ in range(reps)]
    a, g = (list(col) for col in zip(*rows))
    byts = 4.0 * pop * n
    print(f"kernels alone      P {pop:6d}, n {n} | pds_es_perturb ms {fmt(a)} = {byts / 1e6:.0f} MB written at "
          f"{byts / (1e-3 * float(np.median(a))) / 1e12:.2f} TB/s | pds_es_gradient (both launches) ms {fmt(g)} | {reps} calls",
          file=out, flush=True)


def learning(seeds, generations, out, obs_stats="warmup"):
    print(f"# centre return (the centre alone on {P * E} envs, mean over them) per generation; Hover lean, P {P} x E {E}, ESTrainer defaults "
          f"(sigma 0.02, lr 0.01, l2 0.005), obs_stats={obs_stats!r}; generation g = the centre before update g + 1", file=out)
    curves = []
    for seed in seeds:
        env = pds.make("DroneHoverSimpleEnv-v0", num_envs=P * E, seed=seed, **LEAN)
        tr = ESTrainer(env, P, seed=seed, obs_stats=obs_stats, eval_every=1)
        logs = [tr.learn_one_generation() for _ in range(generations)]
        curves.append(logs)
        env.close()
    print("# generation | " + " | ".join(f"seed {s}: centre return, population fitness mean, episode length" for s in seeds), file=out)
    for g in range(generations):
        print(f"{g:4d} | " + " | ".join(f"{c[g]['centre_return']:10.2f} {c[g]['fitness_mean']:10.2f} {c[g]['ep_len']:6.1f}" for c in curves),
              file=out)
    for s, c in zip(seeds, curves):
        first, last, best = c[0]["centre_return"], c[-1]["centre_return"], max(l["centre_return"] for l in c)
        print(f"# seed {s}: generation 0 {first:.2f}, last {last:.2f}, best {best:.2f}: "
              f"{'improved' if last > first else 'NOT improved'} over generation 0", file=out)
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--generations", type=int, default=30, help="generations per seed of the learning record (0: skip it)")
    ap.add_argument("--timing-out", default=None)
    ap.add_argument("--learning-out", default=None)
    ap.add_argument("--obs-stats", default="warmup", help="comma-separated obs_stats of the learning record, one block each: warmup,online")
    ap.add_argument("--no-timing", action="store_true", help="the learning record only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "es_bench.py needs a HIP device"
    t_out = open(args.timing_out, "w") if args.timing_out else sys.stdout
    print(f"# one generation of ESTrainer on DroneHoverSimpleEnv-v0, {torch.cuda.get_device_name(0)}; device events; one warm-up generation, "
          "then median [min .. max]", file=t_out)
    if not args.no_timing:
        time_generation("Hover lean", LEAN, args.reps, t_out)
        time_generation("Hover defaults", {}, args.reps, t_out)
        for pop in (4096, 16384):
            time_kernels(pop, 4504, 4 * args.reps, t_out)
    if args.generations > 0:
        l_out = open(args.learning_out, "w") if args.learning_out else sys.stdout
        for mode in args.obs_stats.split(","):
            learning((0, 1, 2), args.generations, l_out, mode)


if __name__ == "__main__":
    main()
