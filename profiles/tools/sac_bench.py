#!/usr/bin/env python3
"""Times one SAC update (sac.py SACTrainer.update: backup, two Q steps, actor step, polyak on the twin Qs) on the fused kernels
(csrc/pds_sac.hip) against the fused=False path -- the same recipe in torch autograd with torch.optim.Adam, its noise drawn by
the same kernel -- in the same process, at mini-batches 128, 4 096 and 65 536.

Hover (D = 34), default networks (64, 64) relu, a replay ring of 2^18 rows filled with random rows (the timing does not depend
on their values), distinct rows drawn once.  Device events around --reps updates after --warmup updates; median [min .. max] per
update.  The fused path is also split into its calls.  The one pass condition: the fused update is not slower than the autograd
one at each of the three sizes (the last line says so; exit status 1 otherwise).

  python profiles/tools/sac_bench.py --out profiles/sac_timing.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd import fused as F  # noqa: E402
from phoenix_drone_simulation_amd.sac import SACTrainer  # noqa: E402

ROWS = 1 << 18


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


def filled(env, fused):
    tr = SACTrainer(env, seed=0, fused=fused, buffer_size=ROWS)
    g = torch.Generator(device=env.device).manual_seed(1)
    b = tr.buffer
    b.oa.copy_(torch.randn(b.oa.shape, device=env.device, generator=g))
    b.oa[:, tr.D:].clamp_(-1.0, 1.0)
    b.obs2.copy_(torch.randn(b.obs2.shape, device=env.device, generator=g))
    b.rew.copy_(torch.randn(ROWS, device=env.device, generator=g))
    b.done.copy_((torch.rand(ROWS, device=env.device, generator=g) < 0.05).float())
    b.size = ROWS
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sac_bench.py needs a HIP device"
    out = open(args.out, "w") if args.out else sys.stdout
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=1024, seed=1)
    print(f"# one SAC update (backup, Q step x 2, actor step, polyak x 2), Hover D = {env.obs_dim}, nets (64, 64) relu, "
          f"{torch.cuda.get_device_name(0)}; device events, {args.warmup} warm-up updates, then {args.reps}: ms per update, "
          f"median [min .. max].  The gradient kernel runs three waves per block (csrc/pds_sac.hip, LDS budget); a four-wave "
          f"variant was not built and is not measured here.", file=out)
    trf, trp = filled(env, True), filled(env, False)
    assert trf.fused and not trp.fused
    ok = True
    for B in (128, 4096, 65536):
        index = trf.sample_rows(B)
        tf = timed(lambda: trf.update(index), args.warmup, args.reps)
        tp = timed(lambda: trp.update(index), args.warmup, args.reps)
        b = trf.buffer
        parts = [
            ("pds_sac_target", lambda: F.sac_target(trf.fm_pi, trf.fm_q1_targ, trf.fm_q2_targ, b.obs2, index, b.rew, b.done, trf.gamma,
                                                    trf.alpha, 1.0, trf.update_seed, 1, trf.target_rows)),
            ("pds_value_grad_step x 2", lambda: (trf.fm_q1.value_grad(b.oa, trf.target_rows, index=index, adam_lr=trf.lr),
                                                 trf.fm_q2.value_grad(b.oa, trf.target_rows, index=index, adam_lr=trf.lr))),
            ("pds_sac_policy_grad", lambda: trf.fm_pi.sac_policy_grad(trf.fm_q1, trf.fm_q2, b.oa, index, trf.alpha, 1.0,
                                                                      trf.update_seed, 2, adam_lr=trf.lr)),
            ("pds_polyak x 2", lambda: (F.polyak(trf.fm_q1_targ, trf.fm_q1, trf.polyak), F.polyak(trf.fm_q2_targ, trf.fm_q2, trf.polyak))),
        ]
        ratio = float(np.median(tp)) / float(np.median(tf))
        ok = ok and ratio >= 1.0
        print(f"mini-batch {B:6d} | fused ms {fmt(tf)} | autograd (fused=False) ms {fmt(tp)} | autograd / fused {ratio:.2f}",
              file=out, flush=True)
        for name, fn in parts:
            print(f"    {name:24s} ms {fmt(timed(fn, args.warmup, args.reps))}", file=out, flush=True)
    print(f"# fused not slower than autograd at each size: {'yes' if ok else 'NO'}", file=out, flush=True)
    env.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
