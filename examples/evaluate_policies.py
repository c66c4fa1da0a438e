#!/usr/bin/env python3
"""Score a set of trained checkpoints: every run directory's actor flies E episodes, all actors of one shape in ONE launch.

A run directory is what PPOTrainer.save_checkpoint and the reference's logger leave behind: `torch_save/model.pt` (the
ActorCritic state_dict) and, optionally, `config.json` (`ac_kwargs.pi.activation` / `hidden_sizes`, `env_id`).  The
directories are grouped by actor shape (inputs, hidden sizes, activation); each group is one PolicyPopulation and one call of
evaluate_population (the evaluation loop of the reference's utils/evaluation.py, for the whole group at once).

  python examples/evaluate_policies.py runs/*/seed_*              # prints mean return, length and cost per checkpoint
  python examples/evaluate_policies.py runs/ --episodes 256 --env DroneCircleSimpleEnv-v0 --log-dir eval_out
  python examples/evaluate_policies.py runs/ --metrics            # also the flight-quality table (evaluation.FlightMetrics.table)
  python examples/evaluate_policies.py runs_h4/ --history 4       # actors trained with observation_history_size = 4
  python examples/evaluate_policies.py runs/ --record 64 --record-dir flights   # the first 64 flights per checkpoint as CSV logs

A group whose actors read H x half inputs (half: one [o, u] half of the env's observation) was trained on an observation history
of H: its env is built with observation_history_size = H (inferred from the width, or --history) and flies in one launch too,
with --record as without it.

A group whose actors have three or four hidden layers -- the (50, 30, 20) and (32, 32, 32, 32) actors of train_ppo.py
--pi-hidden ... --deep-fused -- flies in one launch as well (pds_evaluate_policies_deep), with --metrics from the same launch;
--record flies such a group on the composed path and says so -- with --deep-forms-fused it takes the launch too
(pds_evaluate_policies_deep_record, where it is built) --, and an observation history is not evaluated at these depths.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population, fused_deep_forms_evaluation_built  # noqa: E402
from phoenix_drone_simulation_amd.ppo import ActorCritic  # noqa: E402


def find_run_dirs(paths):
    """every directory under `paths` that holds torch_save/model.pt, sorted"""
    found = []
    for path in paths:
        for root, _, _ in os.walk(path):
            if os.path.isfile(os.path.join(root, "torch_save", "model.pt")):
                found.append(root)
    return sorted(set(found))


def load_run(run_dir):
    """-> (ActorCritic, env id or None).  The activation is not in the state_dict: config.json names it (default relu)."""
    conf = {}
    conf_path = os.path.join(run_dir, "config.json")
    if os.path.isfile(conf_path):
        with open(conf_path) as f:
            conf = json.load(f)
    kw = conf.get("ac_kwargs", {})
    sd = torch.load(os.path.join(run_dir, "torch_save", "model.pt"), map_location="cpu")
    ac = ActorCritic.from_reference_state_dict(sd, pi_activation=kw.get("pi", {}).get("activation", "relu"),
                                               val_activation=kw.get("val", {}).get("activation", "tanh"))
    want = kw.get("pi", {}).get("hidden_sizes")
    have = tuple(l.out_features for l in ac.pi.net if isinstance(l, torch.nn.Linear))[:-1]
    if want is not None and tuple(want) != have:
        raise ValueError(f"{run_dir}: config.json says hidden_sizes {tuple(want)}, model.pt holds {have}")
    return ac, conf.get("env_id")


def group_by_shape(runs):
    """{(d_in, hidden sizes, activation, with standardisation): [(run_dir, ActorCritic), ...]}"""
    groups = {}
    for run_dir, ac in runs:
        lin = [l for l in ac.pi.net if isinstance(l, torch.nn.Linear)]
        act = type(ac.pi.net[1]).__name__.lower()
        key = (lin[0].in_features, tuple(l.out_features for l in lin[:-1]), act, ac.obs_oms is not None)
        groups.setdefault(key, []).append((run_dir, ac))
    return groups


def infer_history(d_in, half):
    """observation_history_size of an env whose observation is `d_in` wide: d_in / half, where half is one [o, u] half of the
    env's row; ValueError where d_in is no multiple of it"""
    if half < 1 or d_in < half or d_in % half != 0:
        raise ValueError(f"{d_in} inputs are not a whole number of {half}-wide observation halves")
    return d_in // half


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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("paths", nargs="+", help="run directories, or directories to search for them")
    ap.add_argument("--env", default=None, help="env id (default: config.json's env_id, else DroneHoverSimpleEnv-v0)")
    ap.add_argument("--episodes", type=int, default=128, help="episodes per checkpoint, a multiple of 64")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fused", default="auto", choices=["auto", "on", "off"])
    ap.add_argument("--log-dir", default=None, help="write returns.csv / costs.csv per checkpoint under <log-dir>/<group>/<p>/")
    ap.add_argument("--metrics", action="store_true",
                    help="also print flight time, mean squared roll / pitch, rate oscillation, action rate, saturation, maximum tilt")
    ap.add_argument("--history", type=int, default=None,
                    help="observation_history_size of the env (default: inferred per group, actor inputs / half the env's observation width)")
    ap.add_argument("--record", type=int, default=None, metavar="R",
                    help="record the first R episodes per checkpoint (a multiple of 64, at most --episodes): state, action and "
                         "observation of every step, from the same launch (evaluation.Flights); a group of history policies "
                         "records in its one launch too, the observation being the whole history its actors read")
    ap.add_argument("--record-dir", default=None, metavar="DIR",
                    help="with --record: one CSV log per recorded episode under <DIR>/<group>/<p>/ in the layout of the "
                         "simulation-optimisation logs (Flights.to_csv_dir; control_mode PWM)")
    ap.add_argument("--use-latency", action="store_true", help="delay the actions through the env's latency ring (use_latency=True)")
    ap.add_argument("--latency", type=float, default=None, help="with --use-latency: the delay in seconds (default: the env's)")
    ap.add_argument("--history-latency", action="store_true",
                    help="with --use-latency and a history other than 2: build the env with history_latency=True, which resolves the "
                         "history's views of the ring's last row for any history size")
    ap.add_argument("--history-latency-fused", action="store_true",
                    help="with --history-latency: evaluate on the ring in one launch (pds_evaluate_policies_history_latency*) where it "
                         "is built, instead of the composed path")
    ap.add_argument("--deep-forms-fused", action="store_true",
                    help="with --record and checkpoints of three or four hidden layers: record in the one launch "
                         "(pds_evaluate_policies_deep_record) where it is built, instead of the composed path")
    args = ap.parse_args()
    if args.record_dir and not args.record:
        ap.error("--record-dir needs --record R")
    fused = {"auto": "auto", "on": True, "off": False}[args.fused]
    lat_kw = latency_kwargs(args)

    loaded = [(d, *load_run(d)) for d in find_run_dirs(args.paths)]
    if not loaded:
        sys.exit("no run directory with torch_save/model.pt under " + ", ".join(args.paths))
    env_ids = {e for _, _, e in loaded if e}
    env_id = args.env or (env_ids.pop() if len(env_ids) == 1 else "DroneHoverSimpleEnv-v0")
    groups = group_by_shape([(d, ac) for d, ac, _ in loaded])
    print(f"{len(loaded)} checkpoints in {len(groups)} group(s) on {env_id}, {args.episodes} episodes each")
    for gi, (key, members) in enumerate(sorted(groups.items(), key=lambda kv: str(kv[0]))):
        d_in, hidden, act, _ = key
        pop = PolicyPopulation.from_actor_critics([ac for _, ac in members])
        env = pds.make(env_id, num_envs=pop.P * args.episodes, seed=args.seed, observation_history_size=args.history or 2, **lat_kw)
        if env.obs_dim != d_in and args.history is None:  # a history policy: the env again, with the history its width says
            half = env.obs_dim // 2
            env.close()
            try:
                history = infer_history(d_in, half)
            except ValueError as e:
                print(f"group {gi} {key}: {e} of {env_id}: skipped")
                continue
            env = pds.make(env_id, num_envs=pop.P * args.episodes, seed=args.seed, observation_history_size=history, **lat_kw)
        if env.obs_dim != d_in:
            print(f"group {gi} {key}: the actors read {d_in} inputs, {env_id} observes {env.obs_dim}: skipped")
            env.close()
            continue
        if pop.deep and getattr(env, "observation_history_size", 2) != 2:  # (pds_mlp_deep_forward reads up to 64 inputs: no path flies these)
            print(f"group {gi} {key}: actors with {len(hidden)} hidden layers on an observation history of "
                  f"{getattr(env, 'observation_history_size', 2)}: not evaluated at this depth, skipped")
            env.close()
            continue
        in_launch = args.deep_forms_fused and pop.deep and fused_deep_forms_evaluation_built(env, pop, "record")
        if pop.deep and args.record and fused is not True and not in_launch:
            print(f"group {gi}: {len(hidden)} hidden layers with --record: " +
                  ("the record form of the launch is not built for this env, " if args.deep_forms_fused else
                   "without --deep-forms-fused ") + "this group flies on the composed path (pds_mlp_deep_forward per checkpoint and step)")
        out = evaluate_population(env, pop, fused=fused, metrics=args.metrics, history_fused=True, record=args.record,
                                  history_latency_fused=args.history_latency_fused, deep_forms_fused=args.deep_forms_fused,
                                  log_dir=os.path.join(args.log_dir, str(gi)) if args.log_dir else None)
        ret, length, cost = out[:3]
        table = out[3].table() if args.metrics else {}
        env.close()
        if args.record:
            flights = out[-1]
            print(f"group {gi}: recorded {flights.R} flights per checkpoint, {int(flights.length.sum())} steps in all")
            if args.record_dir:
                for p in range(pop.P):
                    one = type(flights)(flights.state[p:p + 1], flights.action[p:p + 1], None, flights.length[p:p + 1], flights.step_seconds,
                                        flights.last_action0[p:p + 1], control_mode=flights.control_mode)
                    one.to_csv_dir(os.path.join(args.record_dir, str(gi), str(p)))
        print(f"group {gi}: {d_in} -> {hidden} -> 4, {act}; {pop.P} checkpoint(s)")
        for p, (run_dir, _) in enumerate(members):
            print(f"  {run_dir}: return {float(ret[p].mean()):9.3f} +- {float(ret[p].std()):7.3f}   "
                  f"length {float(length[p].mean()):6.1f}   cost {float(cost[p].mean()):7.2f}")
            if table:
                print("    " + "  ".join(f"{k} {float(v[p]):.4g}" for k, v in table.items()))


if __name__ == "__main__":
    main()
