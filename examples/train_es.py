#!/usr/bin/env python3
"""Train an actor with an evolution strategy (OpenAI-ES) on a batched Simple env and leave the reference's run artefacts behind.

A generation is P policies x E episodes in one launch (evaluation.evaluate_population); the population is written on the device
from the centre (pds_es_perturb) and the search gradient regenerates the noise from its counters (pds_es_gradient,
csrc/pds_es.hip).  The reference has no such trainer: this stands where it spreads independent evaluations over MPI cores.
The checkpoint is PPOTrainer's (`torch_save/model.pt` + `model.json`): examples/evaluate_policies.py reads it.

    python examples/train_es.py --env DroneHoverSimpleEnv-v0 --population 4096 --episodes 64 --generations 5 --log-dir /tmp/es_run

--penalise NAME=W (repeatable) trains on return - W x the raw flight metric NAME (es.penalised_return; the names are
evaluation.METRIC_NAMES), e.g. --penalise action_rate_sq=0.5 against chattering motor commands.

--hidden H1 H2 [H3 [H4]] sets the actor's hidden widths: two, or three or four of at most 64 each -- the small deep actors of the
reference's architecture search, e.g. --hidden 50 30 20 or --hidden 32 32 32 32 --activation tanh.  At three and four hidden
layers --obs-stats online takes its sums from the generation's launch with --deep-forms-fused (pds_evaluate_policies_deep_stats).
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.es import ESTrainer, penalised_return  # noqa: E402


def latency_kwargs(args):
    """the env keywords of --use-latency / --latency / --history-latency"""
    kw = {}
    if args.use_latency:
        kw["use_latency"] = True
        if args.latency is not None:
            kw["latency"] = args.latency
    if args.history_latency:
        kw["history_latency"] = True
    return kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="DroneHoverSimpleEnv-v0")
    ap.add_argument("--population", type=int, default=4096, help="policies per generation (even: antithetic pairs)")
    ap.add_argument("--episodes", type=int, default=64, help="episodes per policy, a multiple of 64")
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--hidden", type=int, nargs="+", default=[50, 50], metavar="H",
                    help="hidden widths of the actor: two, or three or four of at most 64 each")
    ap.add_argument("--activation", choices=("relu", "tanh"), default="relu", help="the actor's activation")
    ap.add_argument("--deep-forms-fused", action="store_true",
                    help="with three or four hidden widths and --obs-stats online: the generation's launch also sums the observations "
                         "(pds_evaluate_policies_deep_stats) where it is built, instead of the composed path")
    ap.add_argument("--sigma", type=float, default=0.02, help="standard deviation of the parameter noise")
    ap.add_argument("--lr", type=float, default=0.01, help="Adam's learning rate on the centre")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log-dir", default=None)
    ap.add_argument("--eval-every", type=int, default=10, help="every that many generations the centre alone flies all envs")
    ap.add_argument("--penalise", action="append", default=[], metavar="NAME=W",
                    help="subtract W x the raw flight metric NAME from every episode's return (repeatable)")
    ap.add_argument("--obs-stats", choices=("none", "warmup", "online"), default="warmup",
                    help="observation standardisation: none, frozen after a random-action warm-up, or kept running from what every "
                         "generation's policies saw")
    ap.add_argument("--shaping", choices=("ranks", "ars"), default="ranks", help="centred ranks, or the weights of Augmented Random Search")
    ap.add_argument("--top-b", type=int, default=None, help="--shaping ars: the best that many pairs enter the update (default: all)")
    ap.add_argument("--history", type=int, default=2, help="observation_history_size of the env (the reference's experiment 04: 1, 2, 4, 6, 8)")
    ap.add_argument("--history-fused", action="store_true",
                    help="with --history other than 2: evaluate every generation in one launch (pds_evaluate_policies_history) where "
                         "it is built, instead of the composed path; --obs-stats online stays composed there without --history-stats-fused")
    ap.add_argument("--history-stats-fused", action="store_true",
                    help="with --history-fused and --obs-stats online: the generation's launch also sums the observations "
                         "(pds_evaluate_policies_history_stats) where it is built, instead of the composed path")
    ap.add_argument("--use-latency", action="store_true", help="delay the actions through the env's latency ring (use_latency=True)")
    ap.add_argument("--latency", type=float, default=None, help="with --use-latency: the delay in seconds (default: the env's)")
    ap.add_argument("--history-latency", action="store_true",
                    help="with --use-latency and a history other than 2: build the env with history_latency=True, which resolves the "
                         "history's views of the ring's last row for any history size")
    ap.add_argument("--history-latency-fused", action="store_true",
                    help="with --history-latency: evaluate on the ring in one launch (pds_evaluate_policies_history_latency*) where it "
                         "is built, instead of the composed path")
    args = ap.parse_args()
    weights = {}
    for item in args.penalise:
        name, sep, w = item.partition("=")
        if not sep:
            ap.error(f"--penalise {item!r}: NAME=W")
        weights[name] = float(w)
    fitness = penalised_return(weights) if weights else None  # (ValueError names the metrics there are)
    env = pds.make(args.env, num_envs=args.population * args.episodes, seed=args.seed,
                   observation_history_size=args.history, **latency_kwargs(args))  # otherwise the reference's default config
    trainer = ESTrainer(env, args.population, hidden_sizes=tuple(args.hidden), activation=args.activation,
                        deep_forms_fused=args.deep_forms_fused, sigma=args.sigma, lr=args.lr, seed=args.seed,
                        obs_stats=None if args.obs_stats == "none" else args.obs_stats, eval_every=args.eval_every, fitness=fitness,
                        shaping=args.shaping, top_b=args.top_b, history_fused=args.history_fused,
                        history_stats_fused=args.history_stats_fused, history_latency_fused=args.history_latency_fused)
    t0 = time.time()
    steps = 0.0
    for g in range(args.generations):
        i = trainer.learn_one_generation()
        steps += i["env_steps"]
        if g % max(1, args.generations // 20) == 0 or g == args.generations - 1:
            print(f"generation {i['generation']:4d}  fitness {i['fitness_mean']:9.2f} [{i['fitness_min']:9.2f} .. {i['fitness_max']:9.2f}]  "
                  f"EpLen {i['ep_len']:6.1f}  centre {i['centre_return']:9.2f}  |g| {i['grad_norm']:.3e}  "
                  f"perturb {1e3 * i['t_perturb']:.2f} ms  evaluate {1e3 * i['t_evaluate']:.2f} ms  update {1e3 * i['t_update']:.2f} ms",
                  flush=True)
    torch.cuda.synchronize()
    print(f"{steps:.0f} env-steps in {time.time() - t0:.1f} s")
    ret, length, cost = trainer.evaluate_centre()
    print(f"centre: mean return {float(ret.mean()):.2f}  mean episode length {float(length.mean()):.1f}  mean cost {float(cost.mean()):.2f}")
    if args.log_dir:
        trainer.save_checkpoint(args.log_dir)          # torch_save/model.pt + model.json (firmware format)
        trainer.write_progress_csv(os.path.join(args.log_dir, "progress.csv"))
        print("saved to", args.log_dir)
    env.close()


if __name__ == "__main__":
    main()
