"""SACTrainer on the device: the fused update against the autograd one, what the replay ring holds after real vector steps,
a short training run with its checkpoint, and the fall-back to autograd for observation histories the kernels do not cover."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOVER = "DroneHoverSimpleEnv-v0"
KEYS = ([f"pi.net.{i}.{t}" for i in (0, 2) for t in ("weight", "bias")] +
        [f"pi.{n}.{t}" for n in ("mu_layer", "log_std_layer") for t in ("weight", "bias")] +
        [f"{q}.q.{i}.{t}" for q in ("q1", "q2") for i in (0, 2, 4) for t in ("weight", "bias")])


def _params(tr):
    """every parameter the update moves: pi, q1, q2 and the target Qs (the target actor is never read or moved)"""
    out = [(f"ac.{k}", v) for k, v in tr.ac.state_dict().items()]
    return out + [(f"targ.{k}", v) for k, v in tr.ac_targ.state_dict().items() if not k.startswith("pi.")]


def test_three_fused_updates_match_three_autograd_updates():
    """The same state, buffer, indices and noise through both paths; every parameter of pi, q1, q2, q1_targ, q2_targ at the bar
    of the DDPG twin of this test: rtol 1e-3, atol 1e-6 of the largest entry; the losses at 1e-4 relative."""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.sac import SACTrainer
    env = pds.make(HOVER, num_envs=256, device=DEV, seed=4)
    kw = dict(seed=5, buffer_size=256 * 8, start_steps=256 * 8, mini_batch_size=128)
    fused, plain = SACTrainer(env, fused=True, **kw), SACTrainer(env, fused=False, **kw)
    assert fused.fused is True and plain.fused is False
    for (k, a), (_, b) in zip(_params(fused), _params(plain)):
        assert torch.equal(a, b), k  # the same initial state
    for _ in range(8):
        fused.step_env()  # warm-up: uniform actions
    for name in ("oa", "obs2", "rew", "done"):
        getattr(plain.buffer, name).copy_(getattr(fused.buffer, name))
    plain.buffer.size, plain.buffer.ptr = fused.buffer.size, fused.buffer.ptr
    assert len(fused.buffer) == 256 * 8 and float(fused.buffer.oa[:, env.obs_dim:].abs().max()) <= 1.0
    for k in range(3):
        index = fused.sample_rows(128)
        assert index.dtype == torch.int64 and index.unique().numel() == 128 and int(index.max()) < 256 * 8  # distinct rows
        assert torch.equal(index, plain.sample_rows(128))  # (the two trainers draw the same rows, and the same noise)
        assert torch.equal(fused.update_noise(128, 2 * k + 1), plain.update_noise(128, 2 * k + 1))
        fused.update(index)
        plain.update(index)
        lq_f, lp_f, lg_f, _ = fused._last
        lq_p, lp_p, lg_p, _ = plain._last
        print(f"update {k}: loss_q {float(lq_f):.6e} / {float(lq_p):.6e}  loss_pi {float(lp_f):.6e} / {float(lp_p):.6e}  "
              f"logp {float(lg_f):.6e} / {float(lg_p):.6e}")
        assert abs(float(lq_f) - float(lq_p)) <= 1e-4 * abs(float(lq_p)) + 1e-6
        assert abs(float(lp_f) - float(lp_p)) <= 1e-4 * abs(float(lp_p)) + 1e-6
        assert abs(float(lg_f) - float(lg_p)) <= 1e-4 * abs(float(lg_p)) + 1e-6
    worst = 0.0
    for (k, got), (_, want) in zip(_params(fused), _params(plain)):
        atol = 1e-6 * max(1.0, float(want.abs().max()))
        worst = max(worst, float(((got - want).abs() / (atol + 1e-3 * want.abs())).max()))
    print(f"largest error / bar over all parameters after three updates: {worst:.3f}")
    for (k, got), (_, want) in zip(_params(fused), _params(plain)):
        assert torch.allclose(got, want, rtol=1e-3, atol=1e-6 * max(1.0, float(want.abs().max()))), k
    init = SACTrainer(env, fused=False, **kw)
    assert float((init.ac.pi.net[0].weight - fused.ac.pi.net[0].weight).detach().abs().max()) > 1e-5  # the actor moved,
    assert float((init.ac.pi.head.weight[4:] - fused.ac.pi.head.weight[4:]).detach().abs().max()) > 1e-5  # its log_std head too,
    assert float((init.ac_targ.q2.q[0].weight - fused.ac_targ.q2.q[0].weight).abs().max()) > 0  # and so did the targets
    env.close()


def test_buffer_holds_what_the_env_returned():
    """128 Hover envs with a TimeLimit of 5 steps and large random actions, a ring of 4 vector steps, 7 steps: against a twin
    env on the same seed and actions (the DDPG twin-env test, through SACTrainer)."""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.sac import SACTrainer
    N = 128
    mk = lambda: pds.make(HOVER, num_envs=N, device=DEV, seed=9, max_episode_steps=5)
    env, twin = mk(), mk()
    D = env.obs_dim
    tr = SACTrainer(env, buffer_size=4 * N + 17, seed=1)  # rounded down to a multiple of N
    assert tr.buffer.capacity == 4 * N
    o, _ = twin.reset()
    o = o.clone()
    g = torch.Generator(device=DEV).manual_seed(2)
    want, n_term, n_trunc, n_reset = [], 0, 0, 0
    for t in range(7):
        a = torch.clamp(3.0 * torch.randn(N, 4, device=DEV, generator=g), -1.0, 1.0)
        tr.step_env(act=a)
        o2, r, te, trn, info = twin.step(a)
        fin = te | trn
        nxt = torch.where(fin.unsqueeze(-1), info["final_obs"], o2)
        want.append((o, a, r.clone(), nxt.clone(), (te & ~trn).float()))
        n_term += int((te & ~trn).sum()); n_trunc += int(trn.sum())
        n_reset += int((fin & (info["final_obs"] != o2).any(-1)).sum())
        o = o2.clone()
        assert torch.equal(tr.obs, o2) and len(tr.buffer) == min((t + 1) * N, 4 * N) and tr.buffer.ptr == ((t + 1) * N) % (4 * N)
    assert n_term > 0 and n_trunc > 0 and n_reset > 0, (n_term, n_trunc, n_reset)
    buf = tr.buffer
    for t, slot in ((4, 0), (5, 1), (6, 2), (3, 3)):  # the ring wrapped: steps 4 .. 6 overwrote steps 0 .. 2
        s = slice(slot * N, (slot + 1) * N)
        ob, a, r, nxt, term = want[t]
        assert torch.equal(buf.oa[s, :D], ob), t     # the observation that was acted on
        assert torch.equal(buf.oa[s, D:], a), t
        assert torch.equal(buf.rew[s], r), t
        assert torch.equal(buf.obs2[s], nxt), t      # final_obs where the env finished, not the reset observation
        assert torch.equal(buf.done[s], term), t     # false where the TimeLimit cut the episode
    assert tr.total_steps == 7 * N
    env.close(); twin.close()


def test_two_epochs_leave_finite_parameters_and_a_checkpoint(tmp_path):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.sac import SACActorCritic, SACTrainer
    env = pds.make(HOVER, num_envs=256, device=DEV, seed=3)
    tr = SACTrainer(env, seed=3, steps_per_epoch=8, start_steps=256 * 4, update_after=256, buffer_size=256 * 16,
                    updates_per_step=2, epochs=2)
    assert tr.fused is True
    tr.learn()
    assert tr.epoch == 2 and len(tr.log) == 2 and tr.total_steps == 2 * 8 * 256
    assert tr.log[0]["in_warm_up"] == 0.0 and tr.updates == 2 * 12  # steps 5 .. 16 update
    assert tr.log[1]["loss_q"] > 0 and all(k in tr.log[1] for k in ("ep_ret", "ep_len", "q1_mean", "q2_max", "log_pi", "loss_pi", "fps"))
    acted = tr.buffer.oa[256 * 4:256 * 16, env.obs_dim:]  # the policy's actions: inside the limit, and not the same twice
    assert float(acted.abs().max()) <= tr.act_limit and not torch.equal(acted[:256], acted[256:512])
    for k, v in _params(tr):
        assert bool(torch.isfinite(v).all()), k
    path = tr.save_checkpoint(str(tmp_path))
    assert path == str(tmp_path / "torch_save" / "model.pt")
    sd = torch.load(path)
    assert list(sd.keys()) == KEYS and all(torch.equal(sd[k], v.cpu()) for k, v in tr.ac.state_dict().items())
    back = SACActorCritic(env.obs_dim)
    back.load_state_dict(sd)  # the reference's layout loads into the stacked head
    assert torch.equal(back.pi.head.weight, tr.ac.pi.head.weight.detach().cpu())
    tr.write_progress_csv(str(tmp_path / "progress.csv"))
    head = (tmp_path / "progress.csv").read_text().splitlines()
    assert head[0].startswith("Epoch,EpRet/Mean,EpRet/Min,EpRet/Max,EpRet/Std,EpLen/Mean") and len(head) == 3
    assert all(c in head[0].split(",") for c in ("Q1Vals/Mean", "Q2Vals/Max", "LogPi", "LossPi", "LossQ", "InWarmUp", "TotalEnvSteps", "FPS"))
    a = tr.policy_action(tr.obs)
    assert a.shape == (256, 4) and torch.equal(a, tr.policy_action(tr.obs)) and float(a.abs().max()) <= tr.act_limit
    env.close()


def test_a_history_of_four_runs_on_the_autograd_path():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.sac import SACTrainer
    env = pds.make(HOVER, num_envs=128, device=DEV, seed=6, observation_history_size=4)
    assert env.obs_dim + 4 > 64
    tr = SACTrainer(env, seed=6, fused=True, start_steps=128 * 2, buffer_size=128 * 8)
    assert tr.fused is False
    for _ in range(4):
        tr.step_env()
    assert tr.in_warm_up is False  # the last two steps acted with the policy and its noise
    before = [p.detach().clone() for p in tr.ac.parameters()]
    tr.update()
    assert all(bool(torch.isfinite(p).all()) for p in tr.ac.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.ac.parameters()))
    env.close()
