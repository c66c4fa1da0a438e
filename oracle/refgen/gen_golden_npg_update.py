#!/usr/bin/env python3
"""Golden vectors for the reference's NPG and TRPO updates (algs/npg/npg.py, algs/trpo/trpo.py): tests/golden/npg_update.npz.

Follows gen_golden_update.py (PPO) next to it and uses the same stand-ins (oracle/refgen/standins).  Runs, in the build container only, the
reference's own `NaturalPolicyGradientAlgorithm` and `TRPOAlgorithm` on its `DroneHoverSimpleEnv-v0` at 1 000 steps per epoch
(2 value iterations x 4 mini-batches) and records everything a restatement needs to repeat the updates without randomness of
its own, under three prefixes:

  npg_   NPG, two consecutive epochs
  trpo_  TRPO, two consecutive epochs
  trpot_ TRPO with target_kl = 3 for one epoch: the search backtracks (asserted: AcceptanceStep >= 2).  On this rollout the
         reference accepts the full step for every target_kl from 1e-4 to 1 (the KL of the full step stays within 1.5 target_kl:
         e.g. 0.0108 at 0.01, 1.02 at 1); only a step so long that the KL grows faster than its quadratic model (8.7 at
         target_kl = 3) is cut back

Per record: the ActorCritic state_dict before epoch 0 and after each update; per epoch the rollout buffer, the path ends with
their bootstrap values, the terminated flags and the value net's shuffles (as update.npz); Loss/Pi before the update, x.Fx,
alpha, |x| (Misc/H_inv_g), |g| (Misc/gradient_norm), AcceptanceStep, and for TRPO every candidate's (loss_pi, KL).  The
generator asserts that no candidate lies within 1e-3 (relative) of either acceptance threshold, so that "the same accepted
step" is a fair demand of a float32 restatement.  Only data is written; running it twice gives the same bytes.

    python oracle/refgen/gen_golden_npg_update.py /path/to/the/reference/checkout
"""
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")  # oracle/refgen -> the repository
ENV_ID = "DroneHoverSimpleEnv-v0"
EPOCHS_TOTAL, STEPS, MINI, V_ITERS = 8, 1000, 4, 2
RECORDS = (("npg_", "npg", 0.01, 2), ("trpo_", "trpo", 0.01, 2), ("trpot_", "trpo", 3.0, 1))


def run(prefix, alg_name, target_kl, epochs, out):
    import phoenix_drone_simulation  # noqa: F401  (registers the env ids)
    from phoenix_drone_simulation.algs.npg import npg
    from phoenix_drone_simulation.algs.trpo import trpo
    from phoenix_drone_simulation.utils import utils
    torch.manual_seed(0)
    np.random.seed(20261016)  # the env draws from numpy's global generator in its constructor (see gen_golden_update.py)
    log_dir = tempfile.mkdtemp(prefix="ref_npg_")
    kw = utils.get_defaults_kwargs(alg=alg_name, env_id=ENV_ID)
    kw.update(epochs=EPOCHS_TOTAL, steps_per_epoch=STEPS, seed=5, verbose=False, save_freq=10 ** 9, num_mini_batches=MINI,
              train_v_iterations=V_ITERS, target_kl=target_kl,
              logger_kwargs=dict(log_dir=log_dir, exp_name="golden", level=0, use_tensor_board=False, verbose=False))
    cls = npg.NaturalPolicyGradientAlgorithm if alg_name == "npg" else trpo.TRPOAlgorithm
    alg = cls(env_id=ENV_ID, **kw)
    p = prefix
    out.update({p + "steps": np.int64(STEPS), p + "epochs_total": np.int64(EPOCHS_TOTAL), p + "epochs": np.int64(epochs),
                p + "num_mini_batches": np.int64(MINI), p + "train_v_iterations": np.int64(V_ITERS),
                p + "obs_dim": np.int64(alg.env.observation_space.shape[0]), p + "gamma": np.float64(alg.buf.gamma),
                p + "lam": np.float64(alg.buf.lam), p + "vf_lr": np.float64(alg.vf_lr), p + "target_kl": np.float64(target_kl),
                p + "cg_damping": np.float64(alg.cg_damping), p + "cg_iters": np.int64(alg.cg_iters)})
    for k, v in alg.ac.state_dict().items():
        out[p + "sd_init__" + k] = v.numpy().copy()

    rec = dict(paths=[], term=[], shuffles=[], stored={}, evals=[])
    finish = alg.buf.finish_path

    def finish_path(last_val=0):
        rec["paths"].append((alg.buf.ptr, float(np.asarray(last_val).reshape(-1)[0])))
        return finish(last_val)
    alg.buf.finish_path = finish_path
    step = alg.env.step

    def env_step(a):
        r = step(a)
        rec["term"].append(bool(r[2]))
        return r
    alg.env.step = env_step
    shuffle = np.random.shuffle

    def rec_shuffle(x):
        shuffle(x)
        rec["shuffles"].append(np.array(x, dtype=np.int64).copy())
    np.random.shuffle = rec_shuffle
    store = alg.logger.store

    def rec_store(**kwargs):
        rec["stored"].update(kwargs)
        return store(**kwargs)
    alg.logger.store = rec_store
    # the (loss_pi, KL) of every parameter set update_policy_net / adjust_step_direction evaluate without gradients: the line
    # search's candidates, then the final parameters
    loss_fn = alg.compute_loss_pi

    def rec_loss(data):
        loss, info = loss_fn(data=data)
        if not torch.is_grad_enabled():
            rec["evals"].append([float(loss.item()), None])
        return loss, info
    alg.compute_loss_pi = rec_loss
    kl_div = torch.distributions.kl.kl_divergence

    def rec_kl(a, b):
        kl = kl_div(a, b)
        if not torch.is_grad_enabled() and rec["evals"] and rec["evals"][-1][1] is None:
            rec["evals"][-1][1] = float(kl.mean().item())
        return kl
    torch.distributions.kl.kl_divergence = rec_kl
    try:
        for e in range(epochs):
            alg.epoch = e
            for k in ("paths", "term", "shuffles", "evals"):
                rec[k].clear()
            alg.ac.update(frac=e / alg.epochs)                       # learn_one_epoch: exploration-noise anneal
            out[f"{p}e{e}_log_std"] = alg.ac.pi.log_std.detach().numpy().copy()
            alg.roll_out()
            b = alg.buf
            for name in ("obs_buf", "act_buf", "rew_buf", "val_buf", "logp_buf", "adv_buf", "target_val_buf", "discounted_ret_buf"):
                out[f"{p}e{e}_{name}"] = getattr(b, name).copy()
            out[f"{p}e{e}_path_end"] = np.array([q for q, _ in rec["paths"]], dtype=np.int64)
            out[f"{p}e{e}_path_last_val"] = np.array([v for _, v in rec["paths"]], dtype=np.float32)
            out[f"{p}e{e}_terminated"] = np.array(rec["term"], dtype=np.uint8)
            assert len(rec["term"]) == STEPS and rec["paths"][-1][0] == STEPS
            alg.update()
            s = rec["stored"]
            out[f"{p}e{e}_shuffles"] = np.stack(rec["shuffles"])
            out[f"{p}e{e}_loss_pi"] = np.float64(alg.loss_pi_before)
            out[f"{p}e{e}_loss_v"] = np.float64(alg.loss_v_before)
            for k in ("Misc/xHx", "Misc/Alpha", "Misc/H_inv_g", "Misc/gradient_norm", "Misc/AcceptanceStep", "Misc/FinalStepNorm",
                      "KL", "Loss/DeltaPi"):
                out[f"{p}e{e}_{k.split('/')[-1]}"] = np.float64(s[k])
            cands = np.array(rec["evals"][:-1], dtype=np.float64).reshape(-1, 2)  # (the last evaluation: the final parameters)
            out[f"{p}e{e}_candidates"] = cands
            acc = int(s["Misc/AcceptanceStep"])
            if alg_name == "trpo":
                lb, lim = float(alg.loss_pi_before), 1.5 * target_kl
                for j, (loss_j, kl_j) in enumerate(cands):
                    # the decision margins: improvement against the candidate's own loss scale, KL against the bound
                    assert abs(lb - loss_j) > 1e-3 * max(abs(lb), abs(loss_j), 1e-3), (prefix, e, j, lb, loss_j)
                    assert abs(kl_j - lim) > 1e-3 * lim, (prefix, e, j, kl_j)
                assert len(cands) == (acc if acc else 15)
            else:
                assert acc == 1 and len(cands) == 0
            for k, v in alg.ac.state_dict().items():
                out[f"{p}e{e}_sd_after__" + k] = v.numpy().copy()
    finally:
        np.random.shuffle = shuffle
        torch.distributions.kl.kl_divergence = kl_div
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PDS_REFERENCE", "")
    if not ref or not os.path.isdir(os.path.join(ref, "phoenix_drone_simulation")):
        raise SystemExit("usage: oracle/refgen/gen_golden_npg_update.py REFERENCE_CHECKOUT")
    sys.path.insert(0, os.path.join(HERE, "standins"))
    sys.path.insert(0, ref)
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = object
    sys.modules["torch.utils.tensorboard"] = tb
    torch.set_num_threads(1)
    out = {}
    for prefix, alg_name, target_kl, epochs in RECORDS:
        run(prefix, alg_name, target_kl, epochs, out)
    assert int(out["trpot_e0_AcceptanceStep"]) >= 2, out["trpot_e0_AcceptanceStep"]
    # np.savez_compressed stamps the zip entries with the current time: write them with a fixed one (same bytes every run)
    path = os.path.join(ROOT, "tests", "golden", "npg_update.npz")
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            a = io.BytesIO()
            np.lib.format.write_array(a, np.asarray(out[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, a.getvalue())
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    print("wrote", path, os.path.getsize(path) // 1024, "kB;", len(out), "arrays; accepted steps",
          {p: [int(out[f"{p}e{e}_AcceptanceStep"]) for e in range(n)] for p, _, _, n in RECORDS})


if __name__ == "__main__":
    main()
