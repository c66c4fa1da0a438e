#!/usr/bin/env python3
"""Train a DDPG agent (the reference's algs/ddpg/ddpg.py) on a batched Simple env and leave a checkpoint behind.

One vector step stores num_envs transitions in the device replay ring; the update reads its mini-batch in place through the
fused kernels of csrc/pds_ddpg.hip (target, Q step, deterministic policy gradient through Q into the actor, polyak).  The
hyper-parameters carry the reference's names; their defaults are starting values, not tuned ones.

    python examples/train_ddpg.py --env DroneHoverSimpleEnv-v0 --num-envs 1024 --epochs 2 --log-dir /tmp/ddpg_run
"""
import argparse
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.ddpg import DDPGTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="DroneHoverSimpleEnv-v0")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--steps-per-epoch", type=int, default=64, help="vector steps per epoch")
    ap.add_argument("--updates-per-step", type=int, default=1, help="gradient updates after every vector step")
    ap.add_argument("--mini-batch-size", type=int, default=128)
    ap.add_argument("--buffer-size", type=int, default=int(1e6))
    ap.add_argument("--warmup-steps", type=int, default=10000, help="transitions with uniform random actions")
    ap.add_argument("--pi-lr", type=float, default=1e-4)
    ap.add_argument("--q-lr", type=float, default=1e-3)
    ap.add_argument("--act-noise", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-fused", action="store_true", help="the torch autograd path")
    ap.add_argument("--fused-collect", action="store_true",
                    help="after warm-up, collect the vector steps between updates in one pds_collect launch")
    ap.add_argument("--control-fused", action="store_true",
                    help="with --fused-collect: the launch is pds_collect_control, which also flies AttitudeRate / Attitude and "
                         "the latency ring on Hover and Circle")
    ap.add_argument("--pi-hidden", type=int, nargs=2, default=[64, 64], metavar=("H1", "H2"), help="the actor's hidden sizes")
    ap.add_argument("--q-hidden", type=int, nargs=2, default=[64, 64], metavar=("H1", "H2"), help="the Q network's hidden sizes")
    ap.add_argument("--broad-fused", action="store_true",
                    help="run hidden sizes above 64 (up to 512) on the fused kernels of include/pds_mlp_broad.h: with --pi-hidden 400 "
                         "300 --q-hidden 400 300 the reference's default configuration, fused")
    ap.add_argument("--control-mode", default="PWM", choices=["PWM", "AttitudeRate", "Attitude"], help="the env's control_mode")
    ap.add_argument("--use-latency", action="store_true", help="the env's delayed-action ring (the reference's 20 ms)")
    ap.add_argument("--log-dir", default=None, help="default: a fresh temporary directory")
    args = ap.parse_args()
    env_kw = dict(control_mode=args.control_mode) if args.control_mode != "PWM" else {}  # (TakeOff fixes PWM and takes no keyword)
    if args.use_latency:
        env_kw["use_latency"] = True
    env = pds.make(args.env, num_envs=args.num_envs, seed=args.seed, **env_kw)  # otherwise the reference's default config
    trainer = DDPGTrainer(env, epochs=args.epochs, steps_per_epoch=args.steps_per_epoch, updates_per_step=args.updates_per_step,
                          mini_batch_size=args.mini_batch_size, buffer_size=args.buffer_size, warmup_steps=args.warmup_steps,
                          pi_lr=args.pi_lr, q_lr=args.q_lr, act_noise=args.act_noise, seed=args.seed, fused=not args.no_fused,
                          fused_collect=args.fused_collect, control_fused=args.control_fused, broad_fused=args.broad_fused,
                          ac_kwargs={"pi": {"hidden_sizes": tuple(args.pi_hidden)}, "q": {"hidden_sizes": tuple(args.q_hidden)}})
    path = ("fused HIP kernels for widths above 64" if trainer.broad else "fused HIP kernels") if trainer.fused else "torch autograd"
    print(f"{args.env}: {env.num_envs} envs, obs_dim {env.obs_dim}, nets {tuple(args.pi_hidden)} / {tuple(args.q_hidden)}, update path: {path}, "
          f"collection: {('one pds_collect_control launch per stretch' if trainer.control_fused else 'one pds_collect launch per stretch') if trainer.collect_fused else 'per-step launches'}")
    t0 = time.time()
    for e in range(args.epochs):
        i = trainer.learn_one_epoch()
        if e % max(1, args.epochs // 20) == 0 or e == args.epochs - 1:
            print(f"epoch {i['epoch']:4d}  EpRet {i['ep_ret']:9.2f}  EpLen {i['ep_len']:6.1f}  QVals {i['q_mean']:9.3f}  LossQ {i['loss_q']:.4e}  "
                  f"LossPi {i['loss_pi']:9.3f}  warm-up {int(i['in_warm_up'])}  updates {i['updates']}  FPS {i['fps']:.0f}", flush=True)
    torch.cuda.synchronize()
    print(f"{trainer.total_steps} env-steps, {trainer.updates} updates in {time.time() - t0:.1f} s")
    log_dir = args.log_dir or tempfile.mkdtemp(prefix="ddpg_")
    path = trainer.save_checkpoint(log_dir)  # torch_save/model.pt, the reference module's keys
    trainer.write_progress_csv(os.path.join(log_dir, "progress.csv"))
    print("saved", path)
    env.close()


if __name__ == "__main__":
    main()
