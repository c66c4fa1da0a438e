"""IWPGAlgorithm.update (algs/iwpg/iwpg.py:398-522) with the PPO-clip loss (algs/ppo/ppo.py:22-40) restated in float64 on a deep
copy of an ActorCritic: torch autograd, torch.optim.Adam and clip_grad_norm_ on the CPU.  The value net is trained first on the
shuffles it is handed, then the policy loop with KL = kl_divergence(p_old, q).mean() (the mean over batch AND action
dimensions, iwpg.py:436-437) compared with target_kl after every step, then the running statistics from the raw data.
The networks, the running statistics and the noise anneal are the ActorCritic's own (anchored to the reference's recorded
state dicts by tests/test_ppo_update_options_cpu.py); the update logic is restated here.
How the recorded batch gets into a trainer, the rows and the comparisons: tests/ppo_update_cases.py."""
import copy

import numpy as np
import torch

import gae_oracle as go


# ---- the float64 update ---------------------------------------------------------------------------------------------------------
class UpdateOracle:
    """One ActorCritic in float64 with its two Adam optimisers; update() is one IWPGAlgorithm.update on a recorded rollout.
    The switches are PPOTrainer's; obs_oms / ret_oms exist on the ActorCritic it is given, or not, accordingly."""

    def __init__(self, ac, g, entropy_coef=0.01, use_entropy=False, target_kl=0.01, use_kl_early_stopping=False,
                 use_max_grad_norm=False, max_grad_norm=0.5, use_reward_scaling=True, use_standardized_obs=True):
        self.ac = copy.deepcopy(ac).cpu().double()
        assert (self.ac.obs_oms is not None) == use_standardized_obs and (self.ac.ret_oms is not None) == use_reward_scaling
        self.gamma, self.lam, self.clip_ratio = float(g["gamma"]), float(g["lam"]), float(g["clip_ratio"])
        self.pi_iters, self.mini = int(g["train_pi_iterations"]), int(g["num_mini_batches"])
        self.entropy_coef = entropy_coef if use_entropy else 0.0
        self.target_kl, self.early = target_kl, use_kl_early_stopping
        self.clip_norm = max_grad_norm if use_max_grad_norm else None
        self.pi_opt = torch.optim.Adam(self.ac.pi.net.parameters(), lr=float(g["pi_lr"]))
        self.vf_opt = torch.optim.Adam(self.ac.v.parameters(), lr=float(g["vf_lr"]))
        self.pi_steps = 0  # Adam steps of the policy net so far

    def _loss_pi(self, obs, act, adv, logp_old):
        dist = self.ac.pi.dist(obs)
        ratio = torch.exp(dist.log_prob(act).sum(-1) - logp_old)
        clip_adv = adv * torch.clamp(ratio, 1 - self.clip_ratio, 1 + self.clip_ratio)
        loss = -(torch.min(ratio * adv, clip_adv)).mean() - self.entropy_coef * dist.entropy().mean()
        return loss, float(dist.entropy().mean().detach()), float(ratio.mean().detach())

    def update(self, d, frac=0.0, pi_lr=None):
        """d: golden_util.load_update_epoch(g, e, "cpu").  frac = epoch / epochs: the exploration-noise anneal of learn_one_epoch
        before the rollout.  pi_lr: this epoch's policy learning rate (None: as it stands)."""
        ac = self.ac
        ac.update(frac=frac)
        f64 = lambda x: x.detach().cpu().double()  # noqa: E731
        n = lambda x: x.detach().cpu().numpy()     # noqa: E731
        scale, bound = 0.0, 10.0
        if ac.ret_oms is not None:  # Buffer.finish_path: rews / (std + eps), clipped to the bound
            scale, bound = 1.0 / (float(ac.ret_oms.std) + ac.ret_oms.eps), float(ac.ret_oms.bound)
        (adv, target_v, disc_ret), _ = go.gae_oracle(n(d["rew"]), n(d["val"]), n(d["term"]), n(d["trunc"]), n(d["fval"]),
                                                     n(d["last_val"]), self.gamma, self.lam, scale, bound)
        adv, target_v, disc_ret = (torch.from_numpy(x).reshape(-1) for x in (adv, target_v, disc_ret))
        raw_obs = f64(d["obs"]).reshape(adv.numel(), -1)
        obs = ac.obs_oms(raw_obs) if ac.obs_oms is not None else raw_obs  # pre_process_data
        act, logp_old = f64(d["act"]).reshape(adv.numel(), -1), f64(d["logp"]).reshape(-1)
        B = adv.numel()
        mbs = B // self.mini
        # ---- update_value_net
        with torch.no_grad():
            loss_v = float(((ac.v(obs) - target_v) ** 2).mean())
        for perm in d["shuffles"]:
            perm = perm.cpu()
            for s in range(0, mbs * self.mini, mbs):
                idx = perm[s:s + mbs]
                self.vf_opt.zero_grad()
                ((ac.v(obs[idx]) - target_v[idx]) ** 2).mean().backward()
                self.vf_opt.step()
        # ---- update_policy_net
        if pi_lr is not None:
            self.pi_opt.param_groups[0]["lr"] = pi_lr
        with torch.no_grad():
            loss_pi, entropy, ratio = self._loss_pi(obs, act, adv, logp_old)
            p_old = ac.pi.dist(obs)
        kls, norms, stop_iter = [], [], self.pi_iters
        for i in range(self.pi_iters):
            self.pi_opt.zero_grad()
            loss_i, _, ratio_last = self._loss_pi(obs, act, adv, logp_old)  # (pi_info of this iteration: what the reference logs)
            loss_i.backward()
            grads = [p.grad for p in ac.pi.parameters() if p.grad is not None]
            norms.append(float(torch.sqrt(sum((g_ ** 2).sum() for g_ in grads))))  # before the clip
            if self.clip_norm is not None:
                torch.nn.utils.clip_grad_norm_(ac.pi.parameters(), self.clip_norm)
            self.pi_steps += 1
            self.pi_opt.step()
            with torch.no_grad():
                kls.append(float(torch.distributions.kl.kl_divergence(p_old, ac.pi.dist(obs)).mean()))
            if self.early and kls[-1] > self.target_kl:
                stop_iter = i + 1
                break
        # ---- update_running_statistics: from the raw data
        if ac.obs_oms is not None:
            ac.obs_oms.update(raw_obs)
        if ac.ret_oms is not None:
            ac.ret_oms.update(disc_ret)
        return dict(sd={k: v.detach().clone() for k, v in ac.state_dict().items()}, stop_iter=stop_iter, kl=kls, grad_norm=norms,
                    loss_pi=float(loss_pi), loss_v=loss_v, entropy=entropy, ratio=ratio, ratio_last=ratio_last)


def initial_actor_critic(g, use_standardized_obs=True, use_reward_scaling=True):
    from phoenix_drone_simulation_amd.ppo import ActorCritic
    ac = ActorCritic(int(g["obs_dim"]), 4, None, use_standardized_obs, use_reward_scaling)
    ac.load_state_dict({k: torch.as_tensor(g["sd_init__" + k]) for k in ac.state_dict()})
    return ac


def sd_margin(got_sd, want_sd, rtol, atol):
    """largest |got - want| / (atol + rtol |want|) over every entry of the state dict, the keys equal"""
    assert set(got_sd) == set(want_sd), (sorted(got_sd), sorted(want_sd))
    worst, where = 0.0, None
    for k, w in want_sd.items():
        x = got_sd[k].detach().cpu().double()
        m = float(((x - w).abs() / (atol + rtol * w.abs())).max())
        m = m if np.isfinite(m) else float("inf")
        if m > worst:
            worst, where = m, k
    return worst, where


def adam_state(opt=None, fm=None):
    """exp_avg / exp_avg_sq flattened in parameter order and the step count, of a torch.optim.Adam or of a FusedMLP"""
    if fm is not None:
        return dict(exp_avg=fm.exp_avg.detach().cpu(), exp_avg_sq=fm.exp_avg_sq.detach().cpu(), step=int(fm.adam_steps))
    st = [opt.state[p] for p in opt.param_groups[0]["params"]]
    steps = {int(s["step"]) for s in st}
    assert len(steps) == 1
    return dict(exp_avg=torch.cat([s["exp_avg"].detach().cpu().reshape(-1) for s in st]),
                exp_avg_sq=torch.cat([s["exp_avg_sq"].detach().cpu().reshape(-1) for s in st]), step=steps.pop())
