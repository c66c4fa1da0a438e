"""tests/ppo_update_oracle.py and the rows of tests/ppo_update_cases.py on the CPU: the float64 restatement of
IWPGAlgorithm.update lands on the reference's recorded parameters at the defaults, stops where the reference's own
early-stopping rule stopped (tests/golden/update_options.npz), and the trainer's PyTorch path (CPU tensors) follows it under
every constructor switch."""
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import ppo_update_cases as uo

CPU_RTOL, CPU_ATOL = 1e-5, 1e-6  # the bar of the CPU replay (test_two_reference_updates_replayed_through_the_torch_path_on_cpu)


@pytest.fixture(scope="module")
def opts():
    return np.load(os.path.join(gu.GOLDEN, "update_options.npz"))


@pytest.fixture()
def torch_gae(monkeypatch):
    import phoenix_drone_simulation_amd.ppo as ppo
    monkeypatch.setattr(ppo, "gae", gu.gae_torch)  # (the HIP kernel restated with torch ops: no device here)


def _reference_sd(g, prefix):
    return {k[len(prefix):]: torch.as_tensor(g[k]) for k in g.files if k.startswith(prefix)}


def test_oracle_lands_on_the_references_recorded_update_at_the_defaults(torch_gae):
    """the oracle and the float32 PyTorch path are both within the CPU replay's 1e-5 / 1e-6 of e0_sd_after__* (both
    distances are printed)"""
    g, want = uo.golden(), uo.oracle_run()
    ref = _reference_sd(g, "e0_sd_after__")
    m_oracle, where = uo.sd_margin(ref, want["sd"], CPU_RTOL, CPU_ATOL)
    tr, _ = uo.run_trainer(uo.ReplayEnv(int(g["obs_dim"]), "cpu"), False, {})
    m_f32, where32 = uo.sd_margin(tr.ac.state_dict(), {k: v.double() for k, v in ref.items()}, CPU_RTOL, CPU_ATOL)
    print("update oracle vs reference e0: err / bar %.3f (%s); float32 PyTorch path vs reference: %.3f (%s)"
          % (m_oracle, where, m_f32, where32))
    assert m_oracle <= 1.0 and m_f32 <= 1.0
    assert abs(want["loss_pi"] - float(g["e0_loss_pi"])) < 1e-5 * max(1.0, abs(float(g["e0_loss_pi"])))
    assert abs(want["loss_v"] - float(g["e0_loss_v"])) < 1e-5 * max(1.0, abs(float(g["e0_loss_v"])))


def test_oracle_stops_where_the_references_own_rule_stopped(opts):
    """the reference's update() with use_kl_early_stopping=True on the same batch (oracle/refgen/gen_golden_update.py): its KL
    sequence, the iteration of its `Reached ES criterion` line and its parameters afterwards"""
    free = uo.oracle_run()
    assert np.allclose(free["kl"], opts["kl_free"], rtol=1e-4, atol=0)  # (the reference evaluates it in float32)
    kw, stop = uo.row_kwargs("early-stop-mid")
    assert abs(kw["target_kl"] / float(opts["target_kl"]) - 1) < 1e-4
    assert stop == int(opts["stop_iter"]) == 6
    want = uo.oracle_run(use_kl_early_stopping=True, target_kl=float(opts["target_kl"]))
    assert want["stop_iter"] == int(opts["stop_iter"])
    assert np.allclose(want["kl"], opts["kl_stopped"], rtol=1e-4, atol=0)
    m, where = uo.sd_margin(_reference_sd(opts, "sd_after__"), want["sd"], CPU_RTOL, CPU_ATOL)
    assert m <= 1.0, (m, where)


def test_the_stopping_row_tells_the_mean_over_both_axes_from_the_sum_over_actions():
    """kl_divergence(p, q).mean() is a quarter of .sum(-1).mean() with four action dimensions: at the row's target_kl the
    reference's rule stops at 6, a rule on the sum at 3 -- so a trainer that stops on the sum fails the row on stop_iter"""
    kw, stop = uo.row_kwargs("early-stop-mid")
    kl = uo.oracle_run()["kl"]
    assert all(a < b for a, b in zip(kl[:5], kl[1:6]))                       # rises over iterations 1 .. 6
    assert kl[4] * uo.GAP < kw["target_kl"] < kl[5] / uo.GAP
    first = lambda seq: next(i + 1 for i, k in enumerate(seq) if k > kw["target_kl"])  # noqa: E731
    assert first(kl) == stop == 6 and first([4 * k for k in kl]) == 3


@pytest.mark.parametrize("rid", uo.ROW_IDS)
def test_torch_path_follows_the_oracle_under_every_switch(rid, torch_gae):
    kw, stop = uo.row_kwargs(rid)
    want = uo.oracle_run(**kw)
    uo.check_row(rid, kw, stop, want)
    tr, (info,) = uo.run_trainer(uo.ReplayEnv(int(uo.golden()["obs_dim"]), "cpu"), False, kw)
    m, where = uo.compare(info, tr.ac.state_dict(), want, CPU_RTOL, CPU_ATOL)
    print("ppo-update cpu", rid, "stop", info["stop_iter"], " ".join(f"{k} {v:.3f}" for k, v in m.items()), "worst", where)
    if kw.get("use_kl_early_stopping"):
        uo.check_reported_kl(info, kw, want)
    else:
        assert "kl" not in info
    if rid == "entropy":
        base = uo.oracle_run()
        assert abs((want["loss_pi"] - base["loss_pi"]) + 0.01 * want["entropy"]) < 1e-12
        assert all(torch.equal(want["sd"][k], base["sd"][k]) for k in base["sd"])  # log_std is not trained


def test_adam_state_carries_over_two_updates_without_lr_decay(torch_gae):
    """use_linear_lr_decay=False: no scheduler, the same pi_lr in both updates, Adam's moments and step count carried from the
    first update into the second (epochs 0 and 1 of the recording as two consecutive batches)"""
    want, oracle = uo.oracle_two_updates()
    tr, infos = uo.run_trainer(uo.ReplayEnv(int(uo.golden()["obs_dim"]), "cpu"), False, dict(use_linear_lr_decay=False), epochs=2)
    assert tr.scheduler is None and tr.pi_opt.param_groups[0]["lr"] == float(uo.golden()["pi_lr"])
    m, where = uo.compare(infos[1], tr.ac.state_dict(), want[1], CPU_RTOL, CPU_ATOL)
    print("ppo-update cpu no-lr-decay second update", " ".join(f"{k} {v:.3f}" for k, v in m.items()), "worst", where)
    m, ref = uo.adam_margins(uo.adam_state(tr.pi_opt), oracle)
    assert ref["step"] == 2 * int(uo.golden()["train_pi_iterations"])
    print("ppo-update cpu no-lr-decay moments err / bar:", " ".join(f"{k} {v:.3f}" for k, v in m.items()))
    assert max(m.values()) <= 1.0, m
    # what the bar has to tell apart: the moments of an optimiser that starts the second update from zero
    fresh = uo.UpdateOracle(tr.ac, uo.golden())  # (any ActorCritic: only the optimiser's start matters here)
    fresh.ac.load_state_dict(want[0]["sd"])
    fresh.update(gu.load_update_epoch(uo.golden(), 1, "cpu"), frac=1 / int(uo.golden()["epochs_total"]))
    lost = uo.adam_state(fresh.pi_opt)
    lost["step"] = ref["step"]
    assert min(uo.adam_margins(lost, oracle)[0].values()) > 100
