#!/usr/bin/env python3
"""Times one DDPG update (ddpg.py DDPGTrainer.update: target, Q step, actor step, polyak on both nets) on the fused kernels
(csrc/pds_ddpg.hip) against the fused=False path -- the same recipe in torch autograd with torch.optim.Adam -- in the same
process, at mini-batches 4 096 and 65 536 and at the trainer's default (128).

Hover (D = 34), default networks (64, 64) relu, a replay ring of 2^18 rows filled with random rows (the timing does not depend
on their values), indices drawn once.  Device events around --reps updates after --warmup updates; median [min .. max] per
update.  The fused path is also split into its four calls.  No ratio is promised; this records what was measured.

  python profiles/tools/ddpg_bench.py --out profiles/ddpg_timing.txt

--hidden H1 H2 sets both networks' hidden sizes.  With --broad-fused (hidden sizes above 64, the kernels of
include/pds_mlp_broad.h) the protocol is another: the fused trainer (broad_fused=True) against the fused=False trainer of the same
process in ALTERNATING blocks -- synchronise, --block calls, synchronise, host clock over the block -- for --rounds rounds after one
warm-up round, for one update() and for one policy_action() on the mini-batch's observations; ms per call, median [min .. max]
over the rounds.

  python profiles/tools/ddpg_bench.py --hidden 400 300 --broad-fused --batches 128 4096 8192 16384 32768 65536 \
      --out profiles/ddpg_broad_timing.txt
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
from phoenix_drone_simulation_amd import fused as F  # noqa: E402
from phoenix_drone_simulation_amd.ddpg import DDPGTrainer  # noqa: E402

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


def blocks(fns, block, rounds):
    """fns: the sides, timed in alternating synchronised blocks of `block` calls -> per side the ms per call of every round"""
    out = [[] for _ in fns]
    for r in range(rounds + 1):  # (round 0 warms up)
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(block):
                fn()
            torch.cuda.synchronize()
            if r > 0:
                out[k].append((time.perf_counter() - t0) * 1e3 / block)
    return out


def filled(env, fused, hidden=(64, 64), broad_fused=False):
    kw = {"pi": {"hidden_sizes": tuple(hidden)}, "q": {"hidden_sizes": tuple(hidden)}}
    tr = DDPGTrainer(env, seed=0, fused=fused, buffer_size=ROWS, ac_kwargs=kw, broad_fused=broad_fused)
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
    ap.add_argument("--hidden", type=int, nargs=2, default=[64, 64], metavar=("H1", "H2"))
    ap.add_argument("--broad-fused", action="store_true", help="the alternating-block protocol on the kernels of include/pds_mlp_broad.h")
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 4096, 65536], help="mini-batch sizes (--broad-fused)")
    ap.add_argument("--block", type=int, default=20, help="calls per synchronised block (--broad-fused)")
    ap.add_argument("--rounds", type=int, default=9, help="timed rounds of alternating blocks (--broad-fused)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ddpg_bench.py needs a HIP device"
    out = open(args.out, "w") if args.out else sys.stdout
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=1024, seed=1)
    hidden = tuple(args.hidden)
    if args.broad_fused:
        trf, trp = filled(env, True, hidden, True), filled(env, False, hidden)
        assert trf.fused and trf.broad and not trp.fused
        print(f"# DDPGTrainer.update() and .policy_action(), Hover D = {env.obs_dim}, nets {hidden} relu, {torch.cuda.get_device_name(0)}; fused = "
              f"broad_fused=True (include/pds_mlp_broad.h), autograd = fused=False of the same process; alternating synchronised blocks of "
              f"{args.block} calls, host clock, one warm-up round, then {args.rounds}: ms per call, median [min .. max] over the rounds", file=out)
        for B in args.batches:
            index = trf.buffer.sample_indices(B)
            obs = trf.buffer.oa[index][:, :trf.D].contiguous()
            tf, tp = blocks([lambda: trf.update(index), lambda: trp.update(index)], args.block, args.rounds)
            af, ap_ = blocks([lambda: trf.policy_action(obs), lambda: trp.policy_action(obs)], args.block, args.rounds)
            verdict = "fused faster beyond both ranges" if max(tf) < min(tp) else ("autograd faster beyond both ranges" if max(tp) < min(tf) else "ranges overlap")
            print(f"mini-batch {B:6d} | update: fused ms {fmt(tf)} | autograd ms {fmt(tp)} | autograd / fused "
                  f"{float(np.median(tp)) / float(np.median(tf)):.2f} ({verdict})", file=out, flush=True)
            verdict = "fused faster beyond both ranges" if max(af) < min(ap_) else ("autograd faster beyond both ranges" if max(ap_) < min(af) else "ranges overlap")
            print(f"           {B:6d} | policy_action: fused ms {fmt(af)} | autograd ms {fmt(ap_)} | autograd / fused "
                  f"{float(np.median(ap_)) / float(np.median(af)):.2f} ({verdict})", file=out, flush=True)
            b = trf.buffer
            parts = [
                ("pds_ddpg_broad_target", lambda: F.ddpg_target(trf.fm_pi_targ, trf.fm_q_targ, b.obs2, index, b.rew, b.done, trf.gamma, 1.0, trf.target_rows)),
                ("pds_mlp_broad_value_grad_step", lambda: trf.fm_q.value_grad(b.oa, trf.target_rows, index=index, adam_lr=trf.q_lr)),
                ("pds_ddpg_broad_policy_grad", lambda: trf.fm_pi.ddpg_policy_grad(trf.fm_q, b.oa, index, 1.0, adam_lr=trf.pi_lr)),
                ("pds_polyak_broad x 2", lambda: (F.polyak(trf.fm_pi_targ, trf.fm_pi, trf.polyak), F.polyak(trf.fm_q_targ, trf.fm_q, trf.polyak))),
            ]
            for name, fn in parts:
                print(f"    {name:30s} ms {fmt(blocks([fn], args.block, 3)[0])}", file=out, flush=True)
        env.close()
        return
    print(f"# one DDPG update (target, Q step, actor step, polyak x 2), Hover D = {env.obs_dim}, nets {hidden} relu, {torch.cuda.get_device_name(0)}; "
          f"device events, {args.warmup} warm-up updates, then {args.reps}: ms per update, median [min .. max]", file=out)
    trf, trp = filled(env, True, hidden), filled(env, False, hidden)
    assert trf.fused and not trp.fused
    for B in (128, 4096, 65536):
        index = trf.buffer.sample_indices(B)
        tf = timed(lambda: trf.update(index), args.warmup, args.reps)
        tp = timed(lambda: trp.update(index), args.warmup, args.reps)
        b = trf.buffer
        parts = [
            ("pds_ddpg_target", lambda: F.ddpg_target(trf.fm_pi_targ, trf.fm_q_targ, b.obs2, index, b.rew, b.done, trf.gamma, 1.0, trf.target_rows)),
            ("pds_value_grad_step", lambda: trf.fm_q.value_grad(b.oa, trf.target_rows, index=index, adam_lr=trf.q_lr)),
            ("pds_ddpg_policy_grad", lambda: trf.fm_pi.ddpg_policy_grad(trf.fm_q, b.oa, index, 1.0, adam_lr=trf.pi_lr)),
            ("pds_polyak x 2", lambda: (F.polyak(trf.fm_pi_targ, trf.fm_pi, trf.polyak), F.polyak(trf.fm_q_targ, trf.fm_q, trf.polyak))),
        ]
        print(f"mini-batch {B:6d} | fused ms {fmt(tf)} | autograd (fused=False) ms {fmt(tp)} | autograd / fused "
              f"{float(np.median(tp)) / float(np.median(tf)):.2f}", file=out, flush=True)
        for name, fn in parts:
            print(f"    {name:22s} ms {fmt(timed(fn, args.warmup, args.reps))}", file=out, flush=True)
    env.close()


if __name__ == "__main__":
    main()
