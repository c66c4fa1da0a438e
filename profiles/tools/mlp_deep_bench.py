#!/usr/bin/env python3
"""Times the kernels for networks with three and four hidden layers (csrc/pds_mlp_deep.hip, through fused.FusedMLP) against the
PyTorch path they replace (what PPOTrainer(fused=False) runs: autograd of the same loss + torch.optim.Adam; the forward under
no_grad) and beside the two-hidden-layer kernel of the nearest shape as a yardstick, in one process:

  policy  34 -> 50, 30, 20 -> 4 relu and 34 -> 32, 32, 32, 32 -> 4 tanh (yardstick 50, 50 relu):
          one policy gradient + Adam at B = 8 192 x 64 and 1 024 x 64; the forward at 8 192 and 2^20 rows
  critic  34 -> 64, 64, 64 -> 1 and 34 -> 64, 64, 64, 64 -> 1 tanh (yardstick 64, 64 tanh):
          one value mini-batch step (indexed, + Adam) at B / 16 = 32 768 and 4 096; the forward at 8 192 and 2^20 rows
  epoch   one whole PPOTrainer.learn_one_epoch at 8 192 envs x 64 steps (Hover) with the deep actor, fused against fused=False

The two sides run in alternating blocks (--blocks of --reps calls each, device events around a block, synchronised); a row
gives ms per call, median [min .. max] over the blocks.  No ratio is promised; this records what was measured.  Not measured:
other widths, d_out 8, more than one rank.

  python profiles/tools/mlp_deep_bench.py --out profiles/mlp_deep_timing.txt"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.fused import FusedMLP  # noqa: E402
from phoenix_drone_simulation_amd.ppo import PPOTrainer, _mlp  # noqa: E402

D, CLIP, LR = 34, 0.2, 3e-4
RATIOS = []  # PyTorch / fused of every row of the deep kernels


def fmt(xs):
    return f"{float(np.median(xs)):8.3f} [{min(xs):.3f} .. {max(xs):.3f}]"


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
        block(fn, 2)  # warm-up
    out = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            out[k].append(block(fn, reps))
    return out


def sides(hidden, d_out, act):
    """(fused call, torch call) factories over one network shape; the two sides own copies of the same parameters"""
    torch.manual_seed(0)
    net = _mlp([D] + list(hidden) + [d_out], act).cuda()
    ref = copy.deepcopy(net)
    return net, FusedMLP(net, act), ref, torch.optim.Adam(ref.parameters(), lr=LR)


def policy_rows(name, hidden, act, args, out):
    net, fm, ref, opt = sides(hidden, 4, act)
    g = torch.Generator(device="cuda").manual_seed(1)
    log_std = torch.full((4,), -0.7, device="cuda")
    res = {}
    for B in (8192 * 64, 1024 * 64):
        x = torch.randn(B, D, device="cuda", generator=g)
        a = torch.randn(B, 4, device="cuda", generator=g)
        adv, lp = torch.randn(B, device="cuda", generator=g), -4.0 + torch.randn(B, device="cuda", generator=g)

        def fused():
            fm.ppo_grad(x, a, adv, lp, log_std, CLIP, adam_lr=LR)

        def torch_side():
            opt.zero_grad()
            d = torch.distributions.Normal(ref(x), torch.exp(log_std))
            ratio = torch.exp(d.log_prob(a).sum(-1) - lp)
            (-torch.min(ratio * adv, adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP))).mean().backward()
            opt.step()

        tf, tp = alternate([fused, torch_side], args.blocks, args.reps)
        res[f"policy gradient + Adam, B = {B}"] = (tf, tp)
        del x, a, adv, lp
    forward_rows(net, fm, ref, g, res, args)
    report(name, res, out)


def critic_rows(name, hidden, args, out):
    net, fm, ref, opt = sides(hidden, 1, "tanh")
    g = torch.Generator(device="cuda").manual_seed(2)
    res = {}
    for B in (8192 * 64, 1024 * 64):
        x, target = torch.randn(B, D, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g)
        idx = torch.randperm(B, device="cuda", generator=g)[:B // 16]

        def fused():
            fm.value_grad(x, target, index=idx, adam_lr=LR)

        def torch_side():
            opt.zero_grad()
            ((ref(x[idx]).squeeze(-1) - target[idx]) ** 2).mean().backward()
            opt.step()

        tf, tp = alternate([fused, torch_side], args.blocks, args.reps)
        res[f"value mini-batch step + Adam, {B // 16} of {B} rows"] = (tf, tp)
        del x, target
    forward_rows(net, fm, ref, g, res, args)
    report(name, res, out)


def forward_rows(net, fm, ref, g, res, args):
    for rows in (8192, 1 << 20):
        x = torch.randn(rows, D, device="cuda", generator=g)
        y = torch.empty(rows, fm.d_out, device="cuda")

        def fused():
            fm.forward(x, out=y)

        def torch_side():
            with torch.no_grad():
                ref(x)

        tf, tp = alternate([fused, torch_side], args.blocks, args.reps)
        res[f"forward, {rows} rows"] = (tf, tp)


def report(name, res, out):
    print(name, file=out)
    for what, (tf, tp) in res.items():
        if "yardstick" not in name:
            RATIOS.append(float(np.median(tp)) / float(np.median(tf)))
        print(f"    {what:52s} | fused ms {fmt(tf)} | PyTorch ms {fmt(tp)} | PyTorch / fused {float(np.median(tp)) / float(np.median(tf)):6.2f}",
              file=out, flush=True)


def epoch_rows(args, out):
    kw = {"pi": {"hidden_sizes": (50, 30, 20), "activation": "relu"}, "val": {"hidden_sizes": (64, 64), "activation": "tanh"}}
    times = {True: [], False: []}
    trainers = {}
    for fused in (True, False):
        env = pds.make("DroneHoverSimpleEnv-v0", num_envs=8192, seed=1)
        trainers[fused] = PPOTrainer(env, rollout_len=64, epochs=100, seed=1, fused=fused, ac_kwargs=kw)
        trainers[fused].learn_one_epoch()  # warm-up (and the capture of the rollout graph)
    for _ in range(args.epochs):
        for fused in (True, False):
            times[fused].append(block(trainers[fused].learn_one_epoch, 1))
    print(f"learn_one_epoch, Hover, 8 192 envs x 64 steps, actor (50, 30, 20) relu, critic (64, 64) tanh: fused ms {fmt(times[True])} | "
          f"fused=False ms {fmt(times[False])} | fused=False / fused {float(np.median(times[False])) / float(np.median(times[True])):.2f}",
          file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_deep_bench.py needs a HIP device"
    out = open(args.out, "w") if args.out else sys.stdout
    print(f"# deep-MLP kernels (csrc/pds_mlp_deep.hip) against the PyTorch path of the same commit, d_in = {D}, {torch.cuda.get_device_name(0)}; "
          f"alternating blocks of {args.reps} calls, {args.blocks} blocks per side, device events, synchronised: ms per call, median [min .. max]",
          file=out)
    policy_rows("policy (50, 30, 20) relu -- deep kernels", (50, 30, 20), "relu", args, out)
    policy_rows("policy (32, 32, 32, 32) tanh -- deep kernels", (32, 32, 32, 32), "tanh", args, out)
    policy_rows("yardstick: policy (50, 50) relu -- two-hidden-layer kernels", (50, 50), "relu", args, out)
    critic_rows("critic (64, 64, 64) tanh -- deep kernels", (64, 64, 64), args, out)
    critic_rows("critic (64, 64, 64, 64) tanh -- deep kernels", (64, 64, 64, 64), args, out)
    critic_rows("yardstick: critic (64, 64) tanh -- two-hidden-layer kernels", (64, 64), args, out)
    epoch_rows(args, out)
    verdict = ("no row of the deep kernels is slower than the PyTorch path: fused=None selects them at both depths" if min(RATIOS) >= 1.0
               else "a row of the deep kernels is slower than the PyTorch path: fused=None must stay on PyTorch ops at that depth")
    print(f"# smallest PyTorch / fused over the {len(RATIOS)} rows of the deep kernels: {min(RATIOS):.2f} -- {verdict}", file=out)
    print("# not measured: other widths, d_out 8, more than one rank", file=out)


if __name__ == "__main__":
    main()
