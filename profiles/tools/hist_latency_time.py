"""Observation histories on the latency ring (history_latency=True), timed on the device:
    python profiles/tools/hist_latency_time.py [path of another build of csrc/pds_history.hip as a shared library]
1. One rollout of 8 192 envs x 64 steps through PPOTrainer.roll_out(): the one-launch form (pds_rollout_history_latency) against
   the per-step rollout it replaces (per step: critic, actor, sample, pds_step, pds_history_advance_latency, V(final history),
   record).  Both sides in this process, in alternating blocks of three rollouts, host clock around a device synchronise; the
   median over the blocks and their range.
2. The per-step history launch at 2^20 envs, H = 4 (Hover, half = 21): pds_history_advance against pds_history_advance_latency
   with a ring of 2 rows and step counts 0 .. 7 (the rule fires in a quarter of the envs) and with lat_steps = 0, device events
   around 20 launches, alternating, the median over the blocks and their range.  With the optional argument the same
   pds_history_advance of another build (the parent commit's unit, `hipcc --offload-arch=gfx950 -shared -fPIC`) is timed beside them."""
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import phoenix_drone_simulation_amd as pds  # noqa: E402
from phoenix_drone_simulation_amd.ppo import PPOTrainer  # noqa: E402

HOVER, CIRCLE = "DroneHoverSimpleEnv-v0", "DroneCircleSimpleEnv-v0"


def spread(xs):
    return f"median {statistics.median(xs):9.3f}  range {min(xs):9.3f} .. {max(xs):9.3f}  ({len(xs)} blocks)"


def rollouts():
    for label, task, kw in (("Hover, reference defaults, H = 4, latency 0.02", HOVER, dict(observation_history_size=4)),
                            ("Circle AttitudeRate + motor dynamics, H = 8, latency 0.02", CIRCLE,
                             dict(observation_history_size=8, control_mode="AttitudeRate", use_motor_dynamics=True))):
        sides = {}
        for name, fr in (("one launch", True), ("per step", False)):
            env = pds.make(task, num_envs=8192, seed=0, use_latency=True, latency=0.02, history_latency=True, **kw)
            sides[name] = PPOTrainer(env, rollout_len=64, epochs=10, seed=1, fused=True, graph_rollout=False, fused_rollout=fr)
        times = {k: [] for k in sides}
        for blk in range(9):  # (block 0 warms up: code objects, buffers)
            for name, tr in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(3):
                    tr.roll_out()
                torch.cuda.synchronize()
                if blk:
                    times[name].append((time.perf_counter() - t0) / 3 * 1e3)
        assert sides["one launch"].fused_rollout is True and sides["per step"].fused_rollout is False
        print(label + "  [ms per rollout of 8192 x 64]")
        for name, xs in times.items():
            print(f"  {name:10s} {spread(xs)}")
        print(f"  per step / one launch = {statistics.median(times['per step']) / statistics.median(times['one launch']):.2f}")
        for tr in sides.values():
            tr.env.close()


def history_launch(other=None):
    n, H, half = 1 << 20, 4, 21
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = pds.native.load()
    g = torch.Generator(device="cpu").manual_seed(0)
    f = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    obs2, fin2, hist, act = f(n, 2 * half), f(n, 2 * half), f(n, H, half), f(n, 4)
    term = (torch.rand(n, generator=g) < 0.01).to(torch.uint8).to(dev)
    trunc = torch.zeros_like(term)
    steps = (torch.arange(n, dtype=torch.int32) % 8).to(dev)
    out, fin, steps_out = torch.empty_like(hist), torch.zeros_like(hist), torch.empty_like(steps)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    plain = lambda L: (lambda: L.pds_history_advance(n, half, H, p(obs2), p(term), p(trunc), p(fin2), 1, p(hist), p(out), p(fin), s))  # noqa: E731
    lat = lambda B: (lambda: lib.pds_history_advance_latency(n, half, H, p(obs2), p(term), p(trunc), p(fin2), 1, p(hist), p(out), p(fin),  # noqa: E731
                                                              p(act), p(steps), p(steps_out), B, 1, s))
    sides = {"pds_history_advance": plain(lib), "..._latency, ring of 2 rows": lat(2), "..._latency, lat_steps = 0": lat(0)}
    if other:
        L = C.CDLL(other)
        L.pds_history_advance.restype, L.pds_history_advance.argtypes = pds.native.SIGNATURES["pds_history_advance"]
        sides["pds_history_advance of " + os.path.basename(other)] = plain(L)
    times = {k: [] for k in sides}
    for blk in range(16):
        for name, fn in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                assert fn() == 0
            e1.record()
            e1.synchronize()
            if blk:
                times[name].append(e0.elapsed_time(e1) / 20 * 1e3)
    print(f"the per-step history launch, 2^20 envs, H = {H}, half = {half}  [us per launch]")
    for name, xs in times.items():
        print(f"  {name:48s} {spread(xs)}")


if __name__ == "__main__":
    rollouts()
    history_launch(sys.argv[1] if len(sys.argv) > 1 else None)
