#!/usr/bin/env python3
"""Times the natural-gradient policy step for actors with three and four hidden layers: the kernels of csrc/pds_npg_deep.hip
(NPGTrainer / TRPOTrainer(deep_fused=True)) against the PyTorch-op policy step, which is what the parent commit runs for such an
actor and what this commit runs without the keyword (fused=False here: the same update without the warning), in one process:

  update  one whole update() of TRPO and of NPG on Hover at 8 192 x 64 and 1 024 x 64, actors (50, 30, 20) relu and
          (32, 32, 32, 32) tanh, critic (64, 64) tanh; both trainers of a row own the same rollout and the same parameters, which
          are put back before every call, so that every call does the same work
  alone   one Fisher-vector product (every 4th row, as the trainer's) and one 16-candidate line search at 2 048 and 131 072 rows:
          FusedMLP(npg_deep=True) against the float32 double backward through autograd / 16 candidates one after the other

The two sides run in alternating blocks (--blocks of --reps calls each, device events around a block, synchronised); a row gives
ms per call, median [min .. max] over the blocks.  No ratio is promised; this records what was measured.  Not measured: other
widths, d_out 8, more than one rank.

  python profiles/tools/npg_deep_bench.py --out profiles/npg_deep_timing.txt"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd import npg  # noqa: E402
from phoenix_drone_simulation_amd.fused import FusedMLP  # noqa: E402
from phoenix_drone_simulation_amd.ppo import _mlp  # noqa: E402

D = 34
ACTORS = [((50, 30, 20), "relu"), ((32, 32, 32, 32), "tanh")]
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
        block(fn, 1)  # warm-up
    out = [[] for _ in fns]
    for _ in range(blocks):
        for k, fn in enumerate(fns):
            out[k].append(block(fn, reps))
    return out


def row(what, tf, tp, out):
    r = float(np.median(tp)) / float(np.median(tf))
    RATIOS.append((what, r))
    print(f"    {what:74s} | kernels ms {fmt(tf)} | PyTorch ops ms {fmt(tp)} | PyTorch / kernels {r:7.2f}", file=out, flush=True)


def update_rows(args, out):
    print("one whole update(), Hover, critic (64, 64) tanh", file=out)
    for N in (8192, 1024):
        for hidden, act in ACTORS:
            kw = {"pi": {"hidden_sizes": hidden, "activation": act}, "val": {"hidden_sizes": (64, 64), "activation": "tanh"}}
            for cls in (npg.TRPOTrainer, npg.NPGTrainer):
                env = pds.make("DroneHoverSimpleEnv-v0", num_envs=N, seed=1)
                a = cls(env, rollout_len=64, epochs=100, seed=1, fused=True, deep_fused=True, ac_kwargs=kw)
                a.roll_out()
                b = cls(env, rollout_len=64, epochs=100, seed=1, fused=False, graph_rollout=False, ac_kwargs=kw)
                b.ac.load_state_dict(a.ac.state_dict())
                for name in ("obs_buf", "act_buf", "rew_buf", "val_buf", "logp_buf", "term_buf", "trunc_buf", "fval_buf"):
                    getattr(b, name).copy_(getattr(a, name))
                b.last_val = a.last_val.clone()
                state = copy.deepcopy(a.ac.state_dict())

                def side(tr):
                    def fn():
                        tr.ac.load_state_dict(state)  # (in place: the kernels hold the parameters' addresses)
                        tr.update()
                    return fn

                reps = args.reps if N == 1024 else max(1, args.reps // 2)
                tf, tp = alternate([side(a), side(b)], args.blocks, reps)
                row(f"{cls.__name__[:-7]} {N} x 64, actor {hidden} {act}", tf, tp, out)
                env.close()
                del a, b


def alone_rows(args, out):
    print("one Fisher-vector product (rows / 4 samples) and one 16-candidate line search alone, d_in 34, d_out 4", file=out)
    for hidden, act in ACTORS:
        torch.manual_seed(0)
        net = _mlp([D] + list(hidden) + [4], act).cuda()
        fm = FusedMLP(net, act, npg_deep=True)
        params = list(net.parameters())
        g = torch.Generator(device="cuda").manual_seed(1)
        log_std = torch.full((4,), -0.7, device="cuda")
        std = torch.exp(log_std)
        P = fm.flat_grad.numel()
        for rows in (2048, 131072):
            x = torch.randn(rows, D, device="cuda", generator=g)
            v = torch.randn(P, device="cuda", generator=g)
            idx = torch.arange(0, rows, 4, device="cuda")
            xs = x[::4].contiguous()
            o = torch.empty(P, device="cuda")

            def fvp_kernel():
                fm.fisher_vector_product(x, v, log_std, 0.1, index=idx, out=o)

            def fvp_torch():  # NPGTrainer._policy_step_torch's Fvp
                q = torch.distributions.Normal(net(xs), std)
                with torch.no_grad():
                    p = torch.distributions.Normal(net(xs), std)
                kl = torch.distributions.kl.kl_divergence(p, q).mean()
                grads = torch.autograd.grad(kl, params, create_graph=True)
                kl_v = (torch.cat([t.view(-1) for t in grads]) * v).sum()
                gg = torch.cat([t.contiguous().view(-1) for t in torch.autograd.grad(kl_v, params)])
                return gg + v * 0.1

            tf, tp = alternate([fvp_kernel, fvp_torch], args.blocks, args.reps)
            row(f"Fisher product, {rows} rows, actor {hidden} {act}", tf, tp, out)

            with torch.no_grad():
                mu_old = net(x)
                a = mu_old + std * torch.randn(rows, 4, device="cuda", generator=g)
                adv = torch.randn(rows, device="cuda", generator=g)
                lp = torch.distributions.Normal(mu_old, std).log_prob(a).sum(-1)
            s = 0.01 * torch.randn(P, device="cuda", generator=g)
            fr = [0.0] + npg.step_fractions()[0]
            fracs = torch.tensor(fr, dtype=torch.float32, device="cuda")
            theta = npg._flat(params)

            def ls_kernel():
                return fm.surrogate_kl(s, fracs, x, a, adv, lp, mu_old, log_std).tolist()  # the trainer's one host read

            def ls_torch():  # the loop of NPGTrainer._policy_step_torch: every candidate with its own host read
                p_old = torch.distributions.Normal(mu_old, std)
                with torch.no_grad():
                    for f in fr:
                        npg._set_flat(params, theta + f * s)
                        d = torch.distributions.Normal(net(x), std)
                        loss = -(torch.exp(d.log_prob(a).sum(-1) - lp) * adv).mean()
                        kl = torch.distributions.kl.kl_divergence(p_old, d).mean()
                        float(loss), float(kl)
                    npg._set_flat(params, theta)

            tf, tp = alternate([ls_kernel, ls_torch], args.blocks, args.reps)
            row(f"line search, 16 candidates, {rows} rows, actor {hidden} {act}", tf, tp, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "npg_deep_bench.py needs a HIP device"
    out = open(args.out, "w") if args.out else sys.stdout
    print(f"# natural-gradient policy step for deep actors: the kernels of csrc/pds_npg_deep.hip (deep_fused=True) against the PyTorch-op "
          f"step of the same commit (the parent commit's only path for these actors), {torch.cuda.get_device_name(0)}; alternating blocks, "
          f"{args.blocks} blocks per side of up to {args.reps} calls, device events, synchronised: ms per call, median [min .. max]", file=out)
    update_rows(args, out)
    alone_rows(args, out)
    slower = [w for w, r in RATIOS if r < 1.0]
    print(f"# PyTorch / kernels over the {len(RATIOS)} rows: smallest {min(r for _, r in RATIOS):.2f}, largest {max(r for _, r in RATIOS):.2f}; "
          + ("no row is slower on the kernels" if not slower else "slower on the kernels: " + "; ".join(slower)), file=out)
    print("# the keyword stays opt-in whatever these numbers are: the default is pinned by the existing tests", file=out)
    print("# not measured: other widths, d_out 8, more than one rank", file=out)


if __name__ == "__main__":
    main()
