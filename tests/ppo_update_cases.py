"""The option tests of PPOTrainer.update() (tests/test_ppo_update_options_cpu.py, tests/test_gpu_ppo_update_options.py): how a
recorded update of tests/golden/update.npz is put into a PPOTrainer (tests/test_trainer.py replays two of them at the
reference's defaults), the rows of constructor switches, and the comparison of a trainer's update with the float64 oracle of
tests/ppo_update_oracle.py."""
import os

import numpy as np
import torch

import golden_util as gu
from ppo_update_oracle import UpdateOracle, adam_state, initial_actor_critic, sd_margin  # noqa: F401  (the tests' one import)

UPDATE_NPZ = os.path.join(gu.GOLDEN, "update.npz")


# ---- the recorded batch into a trainer -----------------------------------------------------------------------------------------
def make_replay_trainer(g, env, fused, **kw):
    """A PPOTrainer with the recorded run's hyper-parameters (anything in `kw` overrides) and its initial state_dict; entries
    of networks the switches leave out (obs_oms / ret_oms) are not loaded."""
    import phoenix_drone_simulation_amd.ppo as ppo
    args = dict(rollout_len=int(g["steps"]), epochs=int(g["epochs_total"]), gamma=float(g["gamma"]), lam=float(g["lam"]),
                clip_ratio=float(g["clip_ratio"]), pi_lr=float(g["pi_lr"]), vf_lr=float(g["vf_lr"]),
                train_pi_iterations=int(g["train_pi_iterations"]), train_v_iterations=int(g["train_v_iterations"]),
                num_mini_batches=int(g["num_mini_batches"]), seed=0, fused=fused, graph_rollout=False)
    args.update(kw)
    tr = ppo.PPOTrainer(env, **args)
    with torch.no_grad():
        for k, p_ in tr.ac.state_dict().items():
            p_.copy_(torch.as_tensor(g["sd_init__" + k], device=env.device))
    return tr


def load_replay_epoch(tr, g, e, d):
    """Epoch `e` of the recording (d = golden_util.load_update_epoch) into the trainer's rollout buffers, after the
    exploration-noise anneal of learn_one_epoch; the recorded shuffles replace the value net's own.  -> the shuffle iterator"""
    tr.ac.update(frac=e / tr.epochs)
    assert torch.allclose(tr.ac.pi.log_std.cpu(), torch.as_tensor(g[f"e{e}_log_std"], dtype=torch.float32), rtol=0, atol=1e-7)
    tr.obs_buf.copy_(d["obs"]); tr.act_buf.copy_(d["act"]); tr.rew_buf.copy_(d["rew"]); tr.val_buf.copy_(d["val"])
    tr.logp_buf.copy_(d["logp"]); tr.term_buf.copy_(d["term"]); tr.trunc_buf.copy_(d["trunc"]); tr.fval_buf.copy_(d["fval"])
    tr.last_val = d["last_val"]
    shuffles = iter(d["shuffles"])
    tr.perm_fn = lambda B: next(shuffles)
    return shuffles


class ReplayEnv:
    """Stands in for a DroneVecEnv where only the trainer's update is exercised (CPU tests): one env, no stepping."""

    def __init__(self, obs_dim, device):
        self.num_envs, self.obs_dim, self.act_dim, self.device = 1, int(obs_dim), 4, torch.device(device)
        self.env_id_base = 0

    def reset(self):
        return torch.zeros(1, self.obs_dim, device=self.device), {}


# ---- the rows of the option tests (CPU: the PyTorch path; GPU: the fused and the PyTorch path) ------------------------------------
SD_RTOL, SD_ATOL = 2e-4, 2e-6   # the project's bar for this update on the device (test_two_reference_updates_replayed_on_the_gpu)
LOSS_TOL = 1e-4                 # x max(1, |loss|), that test's
REL_TOL = 1e-5                  # entropy, ratio
GAP = 1.15                      # a target_kl sits at least this factor away from the KL on either side of it
ROW_IDS = ["defaults", "early-stop-mid", "early-stop-first", "early-stop-never", "grad-norm-2.85", "grad-norm-0.5",
           "grad-norm-2.85-early-stop", "entropy", "no-reward-scaling", "no-obs-standardisation", "neither"]
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        _CACHE["g"] = np.load(UPDATE_NPZ)
    return _CACHE["g"]


def oracle_run(**kw):
    """one float64 update of epoch 0 under PPOTrainer's switches `kw`; computed once per set of switches, read-only"""
    key = tuple(sorted(kw.items()))
    if key not in _CACHE:
        g = golden()
        ac = initial_actor_critic(g, kw.get("use_standardized_obs", True), kw.get("use_reward_scaling", True))
        _CACHE[key] = UpdateOracle(ac, g, **kw).update(gu.load_update_epoch(g, 0, "cpu"))
    return _CACHE[key]


def target_between(kl, i=4):
    """-> (target_kl, stop_iter): the geometric mean of kl[i] and kl[i + 1] of a sequence that rises up to there, at least GAP
    away from both (i = 4 unless that gap fails: then the widest of the others) -- the rule stops after iteration i + 2"""
    ok = lambda j: all(a < b for a, b in zip(kl[:j + 1], kl[1:j + 2])) and kl[j + 1] / kl[j] > GAP * GAP  # noqa: E731
    if not ok(i):
        i = max((j for j in range(len(kl) - 1) if ok(j)), key=lambda j: kl[j + 1] / kl[j])
    t = float(np.sqrt(kl[i] * kl[i + 1]))
    assert kl[i] * GAP < t < kl[i + 1] / GAP
    return t, i + 2


def row_kwargs(rid):
    """-> (PPOTrainer / UpdateOracle switches of the row, the stop_iter the row is there for or None)"""
    clip = dict(use_max_grad_norm=True, max_grad_norm=2.85)
    if rid == "early-stop-mid":       # between the KL after iterations 5 and 6: the reference's rule stops at 6, 4 x the KL at 3
        t, stop = target_between(oracle_run()["kl"])
        assert stop == 6
        return dict(use_kl_early_stopping=True, target_kl=t), stop
    if rid == "early-stop-first":
        return dict(use_kl_early_stopping=True, target_kl=0.5 * oracle_run()["kl"][0]), 1
    if rid == "early-stop-never":
        return dict(use_kl_early_stopping=True, target_kl=1.0), int(golden()["train_pi_iterations"])
    if rid == "grad-norm-2.85":
        return clip, None
    if rid == "grad-norm-0.5":        # the reference's default: binds on all ten
        return dict(use_max_grad_norm=True, max_grad_norm=0.5), None
    if rid == "grad-norm-2.85-early-stop":
        t, stop = target_between(oracle_run(**clip)["kl"])
        return dict(clip, use_kl_early_stopping=True, target_kl=t), stop
    return {"defaults": {}, "entropy": dict(use_entropy=True), "no-reward-scaling": dict(use_reward_scaling=False),
            "no-obs-standardisation": dict(use_standardized_obs=False),
            "neither": dict(use_reward_scaling=False, use_standardized_obs=False)}[rid], None


def check_row(rid, kw, stop, want):
    """what a row asserts on the oracle's own run `want`, before any trainer is compared with it"""
    n = int(golden()["train_pi_iterations"])
    if stop is not None:
        assert want["stop_iter"] == stop and len(want["kl"]) == stop
    else:
        assert want["stop_iter"] == n and len(want["kl"]) == n
    if kw.get("use_kl_early_stopping"):
        if stop < n:      # the KL that stopped it is GAP above the target, the one before it (if any) GAP below
            assert want["kl"][-1] > kw["target_kl"] * GAP and all(k * GAP < kw["target_kl"] for k in want["kl"][:-1])
        else:
            assert all(k * GAP < kw["target_kl"] for k in want["kl"])
    if kw.get("use_max_grad_norm"):
        c, norms = kw["max_grad_norm"], want["grad_norm"]
        assert all(abs(x / c - 1) >= 0.03 for x in norms), norms   # no norm within 3 % of the threshold
        binds = [x > c for x in norms]
        if c == 2.85 and not kw.get("use_kl_early_stopping"):
            assert any(binds) and not all(binds), norms            # the clip binds on some iterations and not on others
        if c == 0.5:
            assert all(binds), norms
    if not kw.get("use_reward_scaling", True) or not kw.get("use_standardized_obs", True):
        keys = set(want["sd"])
        assert any(k.startswith("ret_oms.") for k in keys) == kw.get("use_reward_scaling", True)
        assert any(k.startswith("obs_oms.") for k in keys) == kw.get("use_standardized_obs", True)


def run_trainer(env, fused, kw, epochs=1):
    """`epochs` recorded updates through a PPOTrainer with switches `kw` -> (trainer, list of update() infos); between two
    updates the bookkeeping of learn_one_epoch (the LambdaLR step if there is a scheduler, the epoch counter)"""
    g = golden()
    tr = make_replay_trainer(g, env, fused, **kw)
    assert tr.fused is fused
    infos = []
    for e in range(epochs):
        shuffles = load_replay_epoch(tr, g, e, gu.load_update_epoch(g, e, env.device))
        infos.append(tr.update())
        assert next(shuffles, None) is None  # every recorded shuffle was consumed
        if tr.scheduler is not None:
            tr.scheduler.step()
        tr.epoch += 1
    return tr, infos


def compare(info, sd, want, rtol=SD_RTOL, atol=SD_ATOL):
    """one update() of a trainer (its info, its state_dict afterwards) against the oracle's -> dict of err / bar, all <= 1.
    loss_pi and loss_v are those of before the update; entropy and ratio are pi_info of the LAST iteration's loss, as the
    reference logs Entropy and PolicyRatio (algs/iwpg/iwpg.py:426, 445-453; tests/golden/learning_curve.json holds 0.989,
    0.981, ...) -- a ratio of before the update is exp(0) = 1 whatever the trainer does, and would check nothing."""
    assert info["stop_iter"] == want["stop_iter"], (info["stop_iter"], want["stop_iter"])
    worst, where = sd_margin(sd, want["sd"], rtol, atol)
    m = dict(sd=worst,
             loss_pi=abs(info["loss_pi"] - want["loss_pi"]) / (LOSS_TOL * max(1.0, abs(want["loss_pi"]))),
             loss_v=abs(info["loss_v"] - want["loss_v"]) / (LOSS_TOL * max(1.0, abs(want["loss_v"]))),
             entropy=abs(info["entropy"] - want["entropy"]) / (REL_TOL * abs(want["entropy"])),
             ratio=abs(info["ratio"] - want["ratio_last"]) / (REL_TOL * abs(want["ratio_last"])))
    assert all(v <= 1.0 for v in m.values()), (m, where)
    return m, where


def check_reported_kl(info, kw, want):
    """info["kl"], the last KL the trainer's stopping rule evaluated: on the same side of target_kl as the oracle's, and closer
    to the oracle's than the gap the target was placed in -> its relative deviation"""
    ref = want["kl"][-1]
    assert (info["kl"] > kw["target_kl"]) == (ref > kw["target_kl"])
    assert ref / GAP < info["kl"] < ref * GAP, (info["kl"], ref)
    return abs(info["kl"] / ref - 1)


def oracle_two_updates():
    """epochs 0 and 1 of the recording as two consecutive updates at a constant pi_lr (use_linear_lr_decay=False)
    -> ([result 0, result 1], the UpdateOracle with its optimisers)"""
    if "two" not in _CACHE:
        g = golden()
        o = UpdateOracle(initial_actor_critic(g), g)
        _CACHE["two"] = ([o.update(gu.load_update_epoch(g, e, "cpu"), frac=e / int(g["epochs_total"])) for e in range(2)], o)
    return _CACHE["two"]


def adam_margins(got, oracle):
    """A trainer's exp_avg / exp_avg_sq of the policy net (adam_state) against the oracle's optimiser -> err / bar per moment,
    with bar = 2e-4 ||exp_avg||_2 and 4e-4 ||exp_avg_sq||_2: the rtol of this update's state-dict bar (SD_RTOL), on the moment
    vector as a whole, doubled for the squares (d(g^2) = 2 g dg).
    Why not element by element: one entry of a gradient is a cancelling sum over the 1000 samples.  It answers the drift the
    state-dict bar allows in the parameters, and a sample within rounding of a relu or clip kink moves it by 1 / B of that
    sample's term (mlp_cases.grad_atol), so a single entry has no scale of its own to be relative to; the vector has.
    What the bar has to tell apart: an optimiser that starts the second update from zero drops the first update's terms,
    weights 0.9^10 .. 0.9^19 of exp_avg (asserted on the CPU: over a hundred bars away); a step count that does not carry over changes the
    bias correction and with it every parameter, which the state-dict bar sees."""
    ref = adam_state(oracle.pi_opt)
    assert got["step"] == ref["step"] == oracle.pi_steps
    out = {}
    for k, rtol in (("exp_avg", SD_RTOL), ("exp_avg_sq", 2 * SD_RTOL)):
        out[k] = float(torch.norm(got[k].double() - ref[k]) / (rtol * torch.norm(ref[k])))
    return out, ref
