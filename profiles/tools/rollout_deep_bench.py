#!/usr/bin/env python3
"""Times the rollout of actors with three and four hidden layers: the one launch of csrc/pds_rollout_deep.h plus the two critic
passes behind it (PPOTrainer(deep_rollout=True)) against the per-step rollout, which is the parent commit's only path for such an
actor and what this commit runs without the keyword (seven launches per env step, replayed from a captured graph up to 262 144
envs, launched one by one above), in one process:

  rollout  one roll_out() on Hover at its defaults, actors (50, 30, 20) relu and (32, 32, 32, 32) tanh beside a (64, 64) tanh critic,
           at 8 192 x 64, 65 536 x 32 and 2^20 x 8 (the last two: more 64-env tiles than CUs with one team per block)
  epoch    one whole learn_one_epoch() of PPO and of TRPO (deep_fused=True) at 8 192 x 64, the keyword on and off

The two sides run in alternating blocks (--blocks of --reps calls each, device events around a block, synchronised); a row gives
ms per call, median [min .. max] over the blocks.  The first rollout of the two sides of a row is compared bit for bit at the timed
size.  No ratio is promised; this records what was measured.  Not measured: other tasks, other widths, more than one rank.

  python profiles/tools/rollout_deep_bench.py --out profiles/rollout_deep_timing.txt"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.npg import TRPOTrainer  # noqa: E402
from phoenix_drone_simulation_amd.ppo import PPOTrainer  # noqa: E402

HOVER = "DroneHoverSimpleEnv-v0"
ACTORS = [((50, 30, 20), "relu"), ((32, 32, 32, 32), "tanh")]
SIZES = [(8192, 64), (65536, 32), (1 << 20, 8)]
RATIOS = []


def fmt(xs):
    return f"{float(np.median(xs)):9.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


def block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, blocks, reps):
    for fn in fns:
        block(fn, 2)  # warm-up (the second call replays the captured graph)
    out = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            out[k].append(block(fn, reps))
    return out


def row(what, tl, tp, other, out):
    r = float(np.median(tp)) / float(np.median(tl))
    apart = min(tp) > max(tl) or min(tl) > max(tp)  # the two sides' ranges do not overlap
    RATIOS.append((what, r, apart))
    print(f"    {what:58s} | one launch ms {fmt(tl)} | {other} ms {fmt(tp)} | per step / one launch {r:6.2f}"
          f"{'' if apart else '  (ranges overlap)'}", file=out, flush=True)


def _kw(hidden, act):
    return {"pi": {"hidden_sizes": hidden, "activation": act}, "val": {"hidden_sizes": (64, 64), "activation": "tanh"}}


def rollout_rows(args, out):
    print("one roll_out(), Hover at its defaults, critic (64, 64) tanh", file=out)
    for N, T in SIZES:
        for hidden, act in ACTORS:
            pair = [PPOTrainer(pds.make(HOVER, num_envs=N, seed=1), rollout_len=T, epochs=100, seed=1, ac_kwargs=_kw(hidden, act),
                               deep_rollout=dr, fused_rollout=True if dr else None) for dr in (True, False)]
            a, b = pair
            a.roll_out(); b.roll_out()
            torch.cuda.synchronize()
            assert a.fused_rollout is True and b.fused_rollout is False
            same = all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf", "last_val"))
            assert same, "the two rollouts differ"
            tl, tp = alternate([a.roll_out, b.roll_out], args.blocks, args.reps)
            row(f"{N} x {T}, actor {hidden} {act}", tl, tp, "per step, graph replay" if b.graph_rollout else "per step, launch by launch", out)
            for t in pair:
                t.env.close()
            del a, b, pair
            torch.cuda.empty_cache()


def epoch_rows(args, out):
    print("one whole learn_one_epoch(), Hover, 8 192 envs x 64 steps, critic (64, 64) tanh (the per-step side: graph replay)", file=out)
    for cls, ckw in ((PPOTrainer, {}), (TRPOTrainer, dict(deep_fused=True))):
        for hidden, act in ACTORS:
            a, b = [cls(pds.make(HOVER, num_envs=8192, seed=1), rollout_len=64, epochs=10000, seed=1, ac_kwargs=_kw(hidden, act),
                        deep_rollout=dr, **ckw) for dr in (True, False)]
            tl, tp = alternate([a.learn_one_epoch, b.learn_one_epoch], args.blocks, args.reps)
            assert a.fused_rollout is True and b.fused_rollout is False
            row(f"{cls.__name__[:-7]}, actor {hidden} {act}", tl, tp, "deep_rollout=False", out)
            a.env.close(); b.env.close()
            del a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rollout_deep_bench.py needs a HIP device"
    out = open(args.out, "w") if args.out else sys.stdout
    print(f"# rollout of deep actors: the one launch of csrc/pds_rollout_deep.h + the critic passes (deep_rollout=True) against the per-step "
          f"rollout of the same commit (the parent commit's only path for these actors), {torch.cuda.get_device_name(0)}; alternating blocks, "
          f"{args.blocks} blocks per side of {args.reps} calls, device events, synchronised: ms per call, median [min .. max]", file=out)
    rollout_rows(args, out)
    epoch_rows(args, out)
    slower = [w for w, r, apart in RATIOS if r < 1.0 and apart]
    print(f"# per step / one launch over the {len(RATIOS)} rows: smallest {min(r for _, r, _ in RATIOS):.2f}, largest {max(r for _, r, _ in RATIOS):.2f}; "
          + ("no row is slower with the one launch beyond both sides' ranges" if not slower else "slower with the one launch, beyond both sides' ranges: "
             + "; ".join(slower)), file=out)
    print("# the keyword stays opt-in whatever these numbers are: the default is pinned by the existing tests", file=out)
    print("# not measured: other tasks, other widths, more than one rank", file=out)


if __name__ == "__main__":
    main()
