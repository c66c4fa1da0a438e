#!/usr/bin/env python3
"""Times the COLLECTION of the off-policy trainers alone -- no update -- on the per-step path (OffPolicyTrainer.step_env + the
episode bookkeeping of learn_one_epoch: about three dozen launches per vector step) against pds_collect (csrc/pds_collect.h: one
launch for K vector steps), in the same process: env-steps per second.

Hover at the reference defaults, default networks (64, 64) relu, DDPG and SAC, N = 1 024, 8 192 and 65 536 envs, K = 1 and 8
vector steps per launch.  Both sides run through the public path: learn_one_epoch on a trainer without warm-up whose epochs are
64 vector steps with an update point every K of them and updates_per_step = 0 -- the collection loop, its bookkeeping and the
epoch's log entry, no update -- with fused_collect off (64 step_env rounds) and on (64 / K launches and one reduction of their
statistics slabs).  `collect()` alone, the launch without any of that, is the third column.  Device events around --reps epochs
after --warmup; ms per K vector steps (epoch / 64 x K), median [min .. max].  Then one trainer epoch end to end (64 vector
steps, an update after each, the examples' settings) at N = 1 024 with the flag off and on, wall clock around a synchronised
epoch.  The one pass condition: the fused side is not slower than the per-step side at any row (the last line says so; exit
status 1 otherwise).

  python profiles/tools/collect_bench.py --out profiles/collect_timing.txt

--env / --control-mode / --use-latency / --motor-dynamics choose another env configuration; --control-fused puts pds_collect_control
(include/pds_collect_control.h) on the fused side, which is what flies a PID control mode or the latency ring.  The two sides of a
row are timed in alternating blocks (--rounds blocks of --reps epochs each per side), so a drift of the shared host falls on both;
the medians are over all of a side's epochs.  --append adds to --out instead of replacing it:

  python profiles/tools/collect_bench.py --control-mode Attitude --control-fused --out profiles/collect_control_timing.txt
  python profiles/tools/collect_bench.py --env DroneCircleSimpleEnv-v0 --control-mode AttitudeRate --use-latency --motor-dynamics \
      --control-fused --out profiles/collect_control_timing.txt --append
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
from phoenix_drone_simulation_amd.ddpg import DDPGTrainer  # noqa: E402
from phoenix_drone_simulation_amd.sac import SACTrainer  # noqa: E402

HOVER = "DroneHoverSimpleEnv-v0"
EPOCH = 64  # vector steps per measured epoch


def fmt(xs):
    return f"{float(np.median(xs)):8.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for k in range(reps):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    return [ev[k].elapsed_time(ev[k + 1]) for k in range(reps)]


def timed_alternating(fns, warmup, reps, rounds):
    """`rounds` blocks of `reps` timed calls per function, the functions taking turns block by block -> one list of ms per function"""
    out = [[] for _ in fns]
    for r in range(rounds):
        for j, fn in enumerate(fns):
            out[j] += timed(fn, warmup if r == 0 else 1, reps)
    return out


ENV_ID, ENV_KW, CONTROL_FUSED = HOVER, {}, False  # main() sets them from the command line


def collector(algo, N, K, flag):
    """a trainer whose epochs are EPOCH vector steps of collection, an update point with no update every K of them"""
    env = pds.make(ENV_ID, num_envs=N, seed=1, **ENV_KW)
    kw = dict(seed=0, buffer_size=16 * N, update_after=0, update_every=K * N, updates_per_step=0, steps_per_epoch=EPOCH,
              fused_collect=flag, control_fused=flag and CONTROL_FUSED)
    tr = DDPGTrainer(env, warmup_steps=0, **kw) if algo == "ddpg" else SACTrainer(env, start_steps=0, **kw)
    assert tr.fused and tr.collect_fused == flag
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternating blocks of --reps epochs per side")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out")
    ap.add_argument("--env", default=HOVER)
    ap.add_argument("--control-mode", default="PWM", choices=["PWM", "AttitudeRate", "Attitude"])
    ap.add_argument("--use-latency", action="store_true")
    ap.add_argument("--motor-dynamics", action="store_true")
    ap.add_argument("--control-fused", action="store_true", help="the fused side is pds_collect_control")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "collect_bench.py needs a HIP device"
    global ENV_ID, ENV_KW, CONTROL_FUSED
    ENV_ID, CONTROL_FUSED = args.env, args.control_fused
    ENV_KW = dict(control_mode=args.control_mode) if args.control_mode != "PWM" else {}
    if args.use_latency:
        ENV_KW["use_latency"] = True
    if args.motor_dynamics:
        ENV_KW["use_motor_dynamics"] = True
    entry = "pds_collect_control" if CONTROL_FUSED else "pds_collect"
    out = open(args.out, "a" if args.append else "w") if args.out else sys.stdout
    print(f"# collection alone, {ENV_ID} at the reference defaults {ENV_KW or ''}, nets (64, 64) relu, {torch.cuda.get_device_name(0)}; device "
          f"events, the two sides in {args.rounds} alternating blocks of {args.reps} epochs of {EPOCH} vector steps ({args.warmup} warm-up epochs "
          f"in front of the first block, 1 in front of the others): ms per K vector steps (epoch / {EPOCH} x K), median [min .. max] "
          f"over a side's {args.rounds * args.reps} epochs; M env-steps/s from the medians", file=out)
    ok = True
    for algo in ("ddpg", "sac"):
        for N in (1024, 8192, 65536):
            for K in (1, 8):
                off, on = collector(algo, N, K, False), collector(algo, N, K, True)
                per_k = lambda ts: [t * K / EPOCH for t in ts]
                t_off, t_on = (per_k(t) for t in timed_alternating((off.learn_one_epoch, on.learn_one_epoch), args.warmup, args.reps, args.rounds))
                epochs = args.warmup + args.rounds - 1 + args.rounds * args.reps
                assert on.collect_launches == EPOCH // K * epochs and off.collect_launches == 0
                t_k = timed(lambda: on.collect(K), args.warmup, args.reps)
                m_off, m_on, m_k = (float(np.median(t)) for t in (t_off, t_on, t_k))
                ratio = m_off / m_on
                ok = ok and ratio >= 1.0
                rate = lambda ms: K * N / ms / 1e3
                print(f"{algo:4s} N {N:6d} K {K} | per-step ms {fmt(t_off)} = {rate(m_off):8.2f} M/s | {entry} ms {fmt(t_on)} = "
                      f"{rate(m_on):8.2f} M/s | per-step / fused {ratio:6.2f} | collect() alone ms {fmt(t_k)} = {rate(m_k):8.2f} M/s",
                      file=out, flush=True)
                off.env.close(); on.env.close()
    print("# one epoch end to end: 64 vector steps at N = 1 024 with an update after each (update_every 50), after warm-up; wall "
          "clock around a synchronised epoch, ms, median [min .. max] of 5", file=out)
    for algo in ("ddpg", "sac"):
        ms = {}
        for flag in (False, True):
            env = pds.make(ENV_ID, num_envs=1024, seed=1, **ENV_KW)
            kw = dict(seed=0, buffer_size=1 << 18, update_after=1024, steps_per_epoch=64, fused_collect=flag, control_fused=flag and CONTROL_FUSED)
            tr = DDPGTrainer(env, warmup_steps=2048, **kw) if algo == "ddpg" else SACTrainer(env, start_steps=2048, **kw)
            tr.learn_one_epoch()  # warm-up and the first updates
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.learn_one_epoch()
                torch.cuda.synchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            ms[flag] = ts
            assert tr.collect_fused == flag and (tr.collect_launches == 62 + 5 * 64 if flag else tr.collect_launches == 0)
            env.close()
        ratio = float(np.median(ms[False])) / float(np.median(ms[True]))
        ok = ok and ratio >= 1.0
        print(f"{algo:4s} epoch | fused_collect=False ms {fmt(ms[False])} | fused_collect=True ms {fmt(ms[True])} | off / on {ratio:.2f}",
              file=out, flush=True)
    print(f"# fused collection not slower than the per-step path at every row: {'yes' if ok else 'NO'}", file=out, flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
