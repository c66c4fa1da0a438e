"""Where the bars of tests/test_gpu_simopt.py come from, and how far the GPU is from them (profiles/simopt_parity_margins.txt):

  python profiles/tools/simopt_parity_margins.py oracle            CPU: float32 oracle vs the reference's float64 losses
  python profiles/tools/simopt_parity_margins.py identifiability [logs.npz]
                                                                   CPU: conditions (a) and (b) of the identifiability test with
                                                                   the oracle, on logs flown by the float32 oracle or on the
                                                                   HIP env's logs (`dump-logs`)
  python profiles/tools/simopt_parity_margins.py gpu               GPU: the kernel's losses vs the reference
  python profiles/tools/simopt_parity_margins.py dump-logs out.npz GPU: the logs the identifiability test flies
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simopt_oracle as so  # noqa: E402


def oracle_deviation():
    z = np.load(so.GOLDEN)
    worst = 0.0
    for name in so.BLOCKS:
        b = so.load_block(name, z)
        ref = b["evaluate_once"]
        d64 = np.abs(so.evaluate_block(b, "f64") - ref) / np.abs(ref)
        d32 = np.abs(so.evaluate_block(b, "f32") - ref) / np.abs(ref)
        worst = max(worst, d32.max())
        print(f"{name}: f64 oracle max rel {d64.max():.3e}   f32 oracle max rel {d32.max():.4e}  per candidate "
              f"{np.array2string(d32.max(1), precision=2)}")
    print(f"F32_ORACLE_MAX_REL = {worst:.4e}   GPU bar = 4 x = {4 * worst:.4e} relative + 1e-7 absolute")


def gpu_margins():
    import test_gpu_simopt as t
    from phoenix_drone_simulation_amd import simopt
    z = np.load(so.GOLDEN)
    for name in so.BLOCKS:
        b = so.load_block(name, z)
        obj = simopt.SimOptObjective(t.ENV_ID, t.block_data(b), aggregate_phy_steps=int(b["aggregate_phy_steps"]))
        got = obj.losses(b["candidates"]).double().cpu().numpy()
        rel = np.abs(got - b["evaluate_once"]) / np.abs(b["evaluate_once"])
        print(f"{name}: GPU max rel {rel.max():.4e} = {rel.max() / t.REFERENCE_RTOL:.3f} of the bar {t.REFERENCE_RTOL:.4e}; "
              f"per candidate {np.array2string(rel.max(1), precision=2)}")


def oracle_logs(steps=260):
    """The flight of the identifiability test on the float32 oracle (the HIP env's arithmetic up to rounding)."""
    import test_gpu_simopt as t
    env = so.make_env("f32")
    so.set_parameters(env, t.TRUTH)
    env.reset()
    env.set("x", [np.sqrt(1.0 / t.TRUTH[0])] * 4)
    acs = t.excitation(steps)
    rows = []
    for a in acs:
        rows.append(np.concatenate([env.get("xyz"), env.get("xyz_dot"), env.get("rpy"), env.get("rpy_dot")]).astype(np.float64))
        env.step(a)
    return np.array(rows), acs


def identifiability(path=None):
    import test_gpu_simopt as t
    from phoenix_drone_simulation_amd import simopt
    if path:
        z = np.load(path)
        log, acs = z["log"], z["acs"]
        print("logs of the HIP env:", path)
    else:
        log, acs = oracle_logs()
        print("logs of the float32 oracle")
    print(f"z in [{log[:, 2].min():.3f}, {log[:, 2].max():.3f}], max |roll, pitch| {np.abs(log[:, 6:8]).max():.3f}")
    for pre_steps in (40, 5):
        obs_s, acs_s, pre_s = simopt.MiniTrajectories.create_trajectory_slices(log, (acs + 1) * 30000.0, T=35, pre_steps=pre_steps)
        block = dict(observations=obs_s, actions=acs_s, pre_inputs=pre_s, aggregate_phy_steps=1, gamma=0.95)
        score = so.evaluate_block(block, "f64", candidates=t.grid_candidates()).mean(1).reshape(6, 9, 9)
        j, i = np.unravel_index(np.argmin(score[2]), (9, 9))
        k, jj, ii = np.unravel_index(np.argmin(score), score.shape)
        print(f"pre_steps {pre_steps}: M {len(obs_s)}  score at the truth {score[2, 2, 4]:.4f}  plane of the true latency: arg-min "
              f"(T index {j}, t2w index {i}) [truth (2, 4)]  global arg-min (latency index {k}, T index {jj}, t2w index {ii}) "
              f"[truth (2, 2, 4)]")
        print("   t2w axis", np.round(score[2, 2], 3), "\n   T axis", np.round(score[2, :, 4], 3), "\n   latency axis",
              np.round(score[:, 2, 4], 3))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "oracle"
    if what == "oracle":
        oracle_deviation()
    elif what == "gpu":
        gpu_margins()
    elif what == "identifiability":
        identifiability(sys.argv[2] if len(sys.argv) > 2 else None)
    elif what == "dump-logs":
        import test_gpu_simopt as t
        log, acs = t.fly_hip_env()
        np.savez(sys.argv[2], log=log, acs=acs)
        print("wrote", sys.argv[2])
    else:
        sys.exit(__doc__)
