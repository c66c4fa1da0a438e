"""PPOTrainer.update() on the device under every constructor switch, fused (the MFMA gradient kernels, pds_adam_step, the value
steps on a second stream) and not (PyTorch ops), each held to the float64 restatement of IWPGAlgorithm.update in
tests/ppo_update_oracle.py on epoch 0 of tests/golden/update.npz (1000 samples: 62 x 16 + 8, 10 policy iterations, 2 x 4 value
mini-batches on the recorded shuffles): stop_iter equal, every state_dict entry within rtol 2e-4 / atol 2e-6, the losses within
1e-4, entropy and ratio within 1e-5 relative.  Behind the switches the fused path has code of its own -- the gradient / clip /
pds_adam_step branch, a hand-written KL, feed(v_total) after an early stop, NULL statistics pointers.
Measured margins: profiles/ppo_update_option_margins.txt."""
import pytest
import torch

import ppo_update_cases as uo

pytestmark = pytest.mark.gpu
_RUNS = {}


def _run(fused, kw, overlap=True, epochs=1):
    """one trainer run per (path, switches), shared between the tests: (state_dict after, infos, Adam state of the policy)"""
    import phoenix_drone_simulation_amd as pds
    key = (fused, overlap, epochs, tuple(sorted(kw.items())))
    if key not in _RUNS:
        env = pds.make("DroneHoverSimpleEnv-v0", num_envs=1, seed=0)
        tr, infos = uo.run_trainer(env, fused, dict(kw, overlap_value_update=overlap), epochs=epochs)
        torch.cuda.synchronize()
        adam = uo.adam_state(fm=tr.fm_pi) if fused else uo.adam_state(tr.pi_opt)
        _RUNS[key] = ({k: v.detach().cpu().clone() for k, v in tr.ac.state_dict().items()}, infos, adam,
                      tr.pi_opt.param_groups[0]["lr"], tr.scheduler)
        env.close()
    return _RUNS[key]


def _same_bits(a, b, prefix=""):
    keys = [k for k in a if k.startswith(prefix)]
    assert keys and set(a) == set(b)
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
@pytest.mark.parametrize("rid", uo.ROW_IDS)
def test_update_follows_the_float64_oracle_under_every_switch(rid, fused, record_property):
    kw, stop = uo.row_kwargs(rid)
    want = uo.oracle_run(**kw)
    uo.check_row(rid, kw, stop, want)
    sd, (info,), _, _, _ = _run(fused, kw)
    print("ppo-update", rid, "fused" if fused else "torch", "stop_iter", info["stop_iter"], "oracle", want["stop_iter"],
          "kl", info.get("kl"), "oracle", want["kl"][-1])
    m, where = uo.compare(info, sd, want)
    print("ppo-update", rid, "fused" if fused else "torch", "err / bar:", " ".join(f"{k} {v:.3f}" for k, v in m.items()),
          "worst entry", where)
    record_property("margin", max(m.values()))
    if kw.get("use_kl_early_stopping"):
        dev = uo.check_reported_kl(info, kw, want)
        print("ppo-update", rid, "fused" if fused else "torch", "kl %.6e oracle %.6e relative deviation %.2e"
              % (info["kl"], want["kl"][-1], dev))
    else:
        assert "kl" not in info
    base_sd, (base,), _, _, _ = _run(fused, {})
    if rid == "entropy":
        # loss_pi moves by -0.01 x entropy (1e-6: float32 rounding of a loss of order 1 on the PyTorch path, exact on the fused
        # one); log_std is not trained, so the fused path's parameters are those of the defaults row on the bits
        assert abs((info["loss_pi"] - base["loss_pi"]) + 0.01 * info["entropy"]) < 1e-6
        assert not fused or _same_bits(sd, base_sd)
    if rid == "early-stop-never" and fused:  # the KL evaluation only reads
        assert _same_bits(sd, base_sd)


@pytest.mark.parametrize("overlap", [True, False], ids=["second-stream", "sequential"])
@pytest.mark.parametrize("rid", ["early-stop-mid", "early-stop-first", "early-stop-never", "grad-norm-2.85-early-stop"])
def test_value_net_gets_every_step_when_the_policy_loop_stops_early(rid, overlap):
    """the two nets share nothing: whatever the policy loop does, the value net after the update is the one of the run
    without early stopping, on the bits -- on the second stream feed(v_total) delivers what the stop left over"""
    kw, stop = uo.row_kwargs(rid)
    sd, (info,), _, _, _ = _run(True, kw, overlap=overlap)
    assert info["stop_iter"] == stop
    base_sd, _, _, _, _ = _run(True, {k: v for k, v in kw.items() if k not in ("use_kl_early_stopping", "target_kl")}, overlap=overlap)
    assert _same_bits(sd, base_sd, "v.")
    assert _same_bits(sd, _run(True, kw, overlap=not overlap)[0])  # (and the schedule of the value steps changes no bit)
    worst, where = uo.sd_margin({k: v for k, v in sd.items() if k.startswith("v.")},
                                {k: v for k, v in uo.oracle_run(**kw)["sd"].items() if k.startswith("v.")}, uo.SD_RTOL, uo.SD_ATOL)
    assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
def test_adam_state_carries_over_two_updates_without_lr_decay(fused, record_property):
    """use_linear_lr_decay=False: no scheduler, the same pi_lr in both updates; the second update starts from the first one's
    Adam moments and step count (pds_adam_step's flat buffers on the fused path) -- against the oracle's optimiser, within
    the bars of ppo_update_cases.adam_margins (the update's rtol on each moment vector as a whole)."""
    want, oracle = uo.oracle_two_updates()
    sd, infos, adam, lr, scheduler = _run(fused, dict(use_linear_lr_decay=False), epochs=2)
    assert scheduler is None and lr == float(uo.golden()["pi_lr"])
    for e in range(2):
        assert infos[e]["stop_iter"] == want[e]["stop_iter"]
    m, where = uo.compare(infos[1], sd, want[1])
    print("ppo-update no-lr-decay", "fused" if fused else "torch", "second update err / bar:",
          " ".join(f"{k} {v:.3f}" for k, v in m.items()), "worst entry", where)
    record_property("margin", max(m.values()))
    am, ref = uo.adam_margins(adam, oracle)
    assert ref["step"] == 2 * int(uo.golden()["train_pi_iterations"])
    print("ppo-update no-lr-decay", "fused" if fused else "torch", "moments err / bar:", " ".join(f"{k} {v:.3f}" for k, v in am.items()),
          "largest element error", " ".join("%s %.2e of %.2e" % (k, float((adam[k].double() - ref[k]).abs().max()),
                                                                 float(ref[k].abs().max())) for k in am))
    assert max(am.values()) <= 1.0, am
    # with the decay the second update would have run at 7/8 of the learning rate: the rows differ
    decayed, _, _, lr2, _ = _run(fused, {}, epochs=2)
    assert lr2 < lr and not _same_bits(sd, decayed, "pi.net.")
