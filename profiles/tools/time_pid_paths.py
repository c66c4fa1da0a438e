"""Time the one-launch paths of the PID control modes on one GPU (sibling of time_variants.py):

  python profiles/tools/time_pid_paths.py stepk [N] [K] [calls]    us per env-step of pds_step_k for the five configurations of
      tests/test_gpu_stepk_pid.py, three repeats each.  PDS_LIB selects another build of the library: with the parent commit's
      library the same call is the loop of K pds_step launches, i.e. the A/B is two runs of this command in one session.
  python profiles/tools/time_pid_paths.py rollout [N] [T] [calls]  env-steps/s of PPOTrainer.roll_out with the one-launch history
      rollout (fused_rollout=True) against the per-step rollout (fused_rollout=False), alternating, three repeats each.

Host clock around work that ends in a device synchronise; every shape is warmed up first."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import phoenix_drone_simulation_amd as pds

IDS = {"hover": "DroneHoverSimpleEnv-v0", "circle": "DroneCircleSimpleEnv-v0"}
OFF = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0.0)
STEPK_CASES = [
    ("circle AttitudeRate lean", "circle", dict(OFF, control_mode="AttitudeRate")),
    ("hover  Attitude on dr tn agg 4", "hover", dict(control_mode="Attitude", aggregate_phy_steps=4)),
    ("circle AttitudeRate pt1 dr", "circle", dict(OFF, control_mode="AttitudeRate", use_motor_dynamics=True, domain_randomization=0.1)),
    ("hover  AttitudeRate latency 0.02 on dr tn", "hover", dict(control_mode="AttitudeRate", use_latency=True, latency=0.02)),
    ("circle Attitude latency 0.03 pt1 lean", "circle", dict(OFF, control_mode="Attitude", use_latency=True, latency=0.03, use_motor_dynamics=True)),
]
ROLLOUT_CASES = [
    ("hover  AttitudeRate H=4", "hover", dict(control_mode="AttitudeRate", observation_history_size=4)),
    ("circle AttitudeRate H=8", "circle", dict(control_mode="AttitudeRate", observation_history_size=8)),
]


def stepk(N, K, calls):
    g = torch.Generator(device="cuda").manual_seed(0)
    acts = (-0.1 + 0.25 * torch.randn(K, N, 4, device="cuda", generator=g)).contiguous()
    print(f"library {os.environ.get('PDS_LIB', '(this tree)')}  N={N} K={K}  {calls} calls per repeat", flush=True)
    for name, task, kw in STEPK_CASES:
        env = pds.make(IDS[task], num_envs=N, seed=0, **kw)
        env.reset()
        for _ in range(5):
            env.step_k(acts)
        torch.cuda.synchronize()
        reps = []
        for rep in range(3):
            t0 = time.perf_counter()
            for _ in range(calls):
                env.step_k(acts)
            torch.cuda.synchronize()
            reps.append((time.perf_counter() - t0) / (calls * K) * 1e6)
        fused = env.lib.pds_step_k_fused(env._handle) if hasattr(env.lib, "pds_step_k_fused") else 0
        print(f"{name:44s} {'one launch' if fused else 'loop      '}  us/env-step " + "  ".join(f"{r:7.2f}" for r in reps) +
              f"   min {min(reps):7.2f}  spread {max(reps) - min(reps):5.2f}   {env.bytes_per_env_step_k(K):4d} B/env-step", flush=True)
        env.close()


def rollout(N, T, calls):
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    print(f"N={N} T={T}  {calls} rollouts per repeat", flush=True)
    for name, task, kw in ROLLOUT_CASES:
        tr = {f: PPOTrainer(pds.make(IDS[task], num_envs=N, seed=0, **kw), rollout_len=T, epochs=3, seed=1, fused=True,
                            graph_rollout=False, fused_rollout=f) for f in (True, False)}
        for t in tr.values():
            for _ in range(2):
                t.roll_out()
        torch.cuda.synchronize()
        reps = {True: [], False: []}
        for rep in range(3):
            for f in (True, False):  # alternating
                t0 = time.perf_counter()
                for _ in range(calls):
                    tr[f].roll_out()
                torch.cuda.synchronize()
                reps[f].append(calls * N * T / (time.perf_counter() - t0) / 1e6)
        assert tr[True].fused_rollout is True and tr[False].fused_rollout is False
        for f in (True, False):
            r = reps[f]
            print(f"{name:28s} {'one launch' if f else 'per step  '}  M env-steps/s " + "  ".join(f"{x:7.2f}" for x in r) +
                  f"   max {max(r):7.2f}  spread {max(r) - min(r):5.2f}", flush=True)
        for t in tr.values():
            t.env.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "stepk"
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    if mode == "stepk":
        stepk(arg(2, 1 << 20), arg(3, 8), arg(4, 20))
    else:
        rollout(arg(2, 8192), arg(3, 64), arg(4, 10))
