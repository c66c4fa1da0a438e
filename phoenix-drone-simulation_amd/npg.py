"""On-device NPG and TRPO for the batched envs: the reference's two other on-policy trainers on the IWPGAlgorithm base.

  NaturalPolicyGradientAlgorithm.update / update_policy_net / Fvp     algs/npg/npg.py:52-160
  TRPOAlgorithm.adjust_step_direction (backtracking line search)       algs/trpo/trpo.py:16-66
  conjugate_gradients                                                  algs/utils.py:5-38
  IWPGAlgorithm.compute_loss_pi (importance-weighted, unclipped)       algs/iwpg/iwpg.py:239-251

Rollout, GAE, observation / return normalisation, the value net's mini-batch update, checkpoints and the non-finite guard
are PPOTrainer's (ppo.py).  What differs is the policy step, taken once per epoch BEFORE the value update (the reference's
order): g = -d loss_pi / d theta, x = F^-1 g by 10 conjugate-gradient iterations, alpha = sqrt(2 target_kl / x.F x),
theta = theta_old + alpha x (NPG) or the first of theta_old + 0.8^j alpha x, j = 0 .. 14, whose loss did not rise and whose
KL stays within 1.5 target_kl (TRPO).  The Fisher-vector products run over every 4th row of the batch.

fused=True: the policy gradient is pds_ppo_policy_grad with an infinite clip ratio (min(r A, clip(r) A) = r A), the Fisher
products, the CG iterations and the line-search candidates are the kernels of csrc/pds_npg.hip -- the step up to alpha with
one host read.  fused=False: the PyTorch-op restatement of the reference (double backward through autograd), the yardstick
of the fused path and the fallback for networks the kernels do not cover.

An actor with 3 or 4 hidden layers (the reference's architecture search trains (50, 30, 20) and (32, 32, 32, 32) with --alg trpo)
takes the PyTorch-op step with a warning unless the trainer is built with deep_fused=True: then the same fused step runs on the
kernels of csrc/pds_npg_deep.hip (include/pds_npg_deep.h), for d_in <= 64."""
import math

import torch
import torch.distributed as dist

from .ppo import PPOTrainer, _avg, _collectives

TOTAL_STEPS, DECAY = 15, 0.8  # algs/trpo/trpo.py:20-21


def iw_loss(ac, data, entropy_coef=0.0):
    """IWPGAlgorithm.compute_loss_pi (algs/iwpg/iwpg.py:239-251): -(ratio adv).mean() - entropy_coef entropy."""
    d, logp = ac.pi(data["obs"], data["act"])
    ratio = torch.exp(logp - data["log_p"])
    loss = -(ratio * data["adv"]).mean()
    loss = loss - entropy_coef * d.entropy().mean()
    return loss, dict(ent=d.entropy().mean(), ratio=ratio.mean())


def conjugate_gradients(Avp, b, nsteps, residual_tol=1e-10, eps=1e-6):
    """algs/utils.py:5-38, statement for statement (the dtype is b's)."""
    x = torch.zeros_like(b)
    r = b - Avp(x)
    p = r.clone()
    rdotr = torch.dot(r, r)
    for _ in range(nsteps):
        z = Avp(p)
        alpha = rdotr / (torch.dot(p, z) + eps)
        x += alpha * p
        r -= alpha * z
        new_rdotr = torch.dot(r, r)
        if torch.sqrt(new_rdotr) < residual_tol:
            break
        mu = new_rdotr / (rdotr + eps)
        p = r + mu * p
        rdotr = new_rdotr
    return x


def step_fractions(total_steps=TOTAL_STEPS, decay=DECAY):
    """step_frac of TRPO's loop: 1, decay, decay^2, ... by repeated multiplication in double, as the reference"""
    out, f = [], 1.0
    for _ in range(total_steps):
        out.append(f)
        f *= decay
    return out, f


def _flat(params):
    return torch.cat([p.data.reshape(-1) for p in params])


def _set_flat(params, flat):
    """in place: the fused kernels (and a captured rollout graph) hold the parameters' addresses"""
    off = 0
    for p in params:
        p.data.copy_(flat[off:off + p.numel()].view_as(p))
        off += p.numel()


class NPGTrainer(PPOTrainer):
    """NaturalPolicyGradientAlgorithm on a DroneVecEnv (algs/npg/defaults.py: target_kl 0.01, cg_damping 0.1, cg_iters 10;
    no learning-rate schedule for the policy).  deep_fused=True: an actor with 3 or 4 hidden layers and d_in <= 64 runs the fused
    policy step on the kernels of include/pds_npg_deep.h (opt-in: without it such an actor warns and runs as PyTorch ops; with
    two hidden layers the keyword changes nothing).  Other arguments as PPOTrainer."""
    line_search = False
    _deep_actor = False  # the Fisher-vector product and the line search take struct pds_mlp: a deeper actor runs as PyTorch ops

    def __init__(self, env, cg_damping=0.1, cg_iters=10, target_kl=0.01, total_steps=TOTAL_STEPS, decay=DECAY, deep_fused=False,
                 **kwargs):
        self.deep_fused = bool(deep_fused)
        if self.deep_fused:  # (before PPOTrainer builds the actor's FusedMLP)
            self._deep_actor, self._pi_fm_kwargs = True, {"npg_deep": True}
        super().__init__(env, target_kl=target_kl, **kwargs)
        self.cg_damping, self.cg_iters = float(cg_damping), int(cg_iters)
        self.total_steps, self.decay = int(total_steps), float(decay)  # TRPO's line search
        self.scheduler = None  # algs/npg/npg.py:30
        self._fvp_index = None

    # ---- update: policy, then value, then running statistics (algs/npg/npg.py:79-96) -----------------------------------
    def update(self):
        ac = self.ac
        data, raw_obs, disc_ret, B, mbs = self._prepare_batch()
        data = {k: v.contiguous() for k, v in data.items()}
        with torch.no_grad():
            v = self.fm_v.forward(data["obs"]).view(-1) if self.fused else ac.v(data["obs"])
            loss_v_before = _avg(((v - data["target_v"]) ** 2).mean())  # (read after the policy step: no sync in front of it)
        vgen = self._value_steps(data["obs"], data["target_v"], B, mbs)
        v_total = self.train_v_iterations * self.num_mini_batches
        with self._value_stream(vgen, data["obs"]) as (_, feed):
            # with the overlap: a chunk of value steps after each Fisher product, the rest behind the policy step
            chunk = -(-v_total // (self.cg_iters + 2))
            info = self._policy_step_fused(data, feed, chunk) if self.fused else self._policy_step_torch(data)
            feed(v_total)
        for _ in vgen:  # without the overlap: every value step, after the policy step
            pass
        self._update_running_statistics(raw_obs, disc_ret)
        info.update(loss_v=float(loss_v_before), stop_iter=1)
        return info

    # ---- the policy step through autograd (the reference's statements) ------------------------------------------------
    def _policy_step_torch(self, data):
        ac = self.ac
        params = list(ac.pi.net.parameters())
        theta_old = _flat(params)
        loss_pi, _ = iw_loss(ac, data, self.entropy_coef)
        loss_pi_before = float(_avg(loss_pi.detach().clone()))
        with torch.no_grad():
            mu_old = ac.pi.net(data["obs"])
        g = torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss_pi, params)])
        g = -_avg(g)
        fvp_obs = data["obs"][::4]
        std = torch.exp(ac.pi.log_std)

        def Fvp(v):
            q = torch.distributions.Normal(ac.pi.net(fvp_obs), std)
            with torch.no_grad():
                p = torch.distributions.Normal(ac.pi.net(fvp_obs), std)
            kl = torch.distributions.kl.kl_divergence(p, q).mean()
            grads = torch.autograd.grad(kl, params, create_graph=True)
            kl_v = (torch.cat([t.view(-1) for t in grads]) * v).sum()
            gg = torch.cat([t.contiguous().view(-1) for t in torch.autograd.grad(kl_v, params)])
            return _avg(gg) + v * self.cg_damping

        x = conjugate_gradients(Fvp, g, self.cg_iters)
        if not bool(torch.isfinite(x).all()):
            raise FloatingPointError("NPG: the conjugate-gradient solution is not finite")
        xHx = torch.dot(x, Fvp(x)).detach()
        if float(xHx) < 0:
            raise FloatingPointError(f"NPG: x.Fx = {float(xHx)} < 0")
        alpha = torch.sqrt(2 * self.target_kl / (xHx + 1e-8))
        step_dir = (alpha * x).detach()
        p_old = torch.distributions.Normal(mu_old, std)
        cands = []
        if self.line_search:
            fracs, f_end = step_fractions(self.total_steps, self.decay)
            accept = 0
            for j, f in enumerate(fracs):
                with torch.no_grad():
                    _set_flat(params, theta_old + f * step_dir)
                    loss_j, _ = iw_loss(ac, data, self.entropy_coef)
                    kl_j = torch.distributions.kl.kl_divergence(p_old, ac.pi.dist(data["obs"])).mean()
                    lk = _avg(torch.stack([loss_j, kl_j]))
                loss_j, kl_j = float(lk[0]), float(lk[1])
                cands.append((loss_j, kl_j))
                if not math.isfinite(loss_j) or loss_pi_before - loss_j < 0 or kl_j > self.target_kl * 1.5:
                    continue
                accept = j + 1
                break
            final = f * step_dir if accept else torch.zeros_like(step_dir) * f_end
        else:
            accept, final = 1, step_dir
        with torch.no_grad():
            _set_flat(params, theta_old + final)
            loss_after, pi_info = iw_loss(ac, data, self.entropy_coef)
            kl = torch.distributions.kl.kl_divergence(p_old, ac.pi.dist(data["obs"])).mean()
        return dict(loss_pi=loss_pi_before, delta_pi=float(loss_after) - loss_pi_before, kl=float(kl),
                    entropy=float(pi_info["ent"]), ratio=float(pi_info["ratio"]), acceptance_step=accept,
                    alpha=float(alpha), final_step_norm=float(torch.norm(final)), gradient_norm=float(torch.norm(g)),
                    xHx=float(xHx), h_inv_g=float(x.norm()), candidates=cands)

    # ---- the policy step on the kernels of csrc/pds_npg.hip (deep_fused: csrc/pds_npg_deep.hip) -----------------------
    def _policy_step_fused(self, data, feed=lambda steps: None, chunk=0):
        from .fused import conjugate_gradients as cg_fused
        ac, fm = self.ac, self.fm_pi
        obs, act, adv, logp_old = data["obs"], data["act"], data["adv"], data["log_p"]
        B, A = obs.shape[0], act.shape[1]
        log_std = ac.pi.log_std
        params = list(ac.pi.net.parameters())
        world = dist.get_world_size() if _collectives() else 1
        with torch.no_grad():
            ent = (0.5 + 0.5 * math.log(2 * math.pi) + log_std).mean()  # Normal(., sigma).entropy().mean(): no network in it
            theta_old = _flat(params)
            mu_old = fm.forward(obs)
            fm.ppo_grad(obs, act, adv, logp_old, log_std, math.inf)  # clip = inf: d(-(r A).mean()) / d theta
            g = _avg(-fm.flat_grad)
            if self._fvp_index is None or self._fvp_index.shape[0] != (B + 3) // 4 or self._fvp_index.device != obs.device:
                self._fvp_index = torch.arange(0, B, 4, device=obs.device)

            def avp(v, out):
                fm.fisher_vector_product(obs, v, log_std, 0.0 if world > 1 else self.cg_damping, index=self._fvp_index, out=out)
                if world > 1:  # mpi_avg_torch_tensor(F v), then + damping v
                    _avg(out)
                    out.add_(v * self.cg_damping)
                feed(chunk)
                return out

            x, _ = cg_fused(avp, g, self.cg_iters)
            fx = avp(x, torch.empty_like(x))
            xHx = torch.dot(x, fx)
            alpha = torch.sqrt(2 * self.target_kl / (xHx + 1e-8))
            step_dir = alpha * x
            fracs = step_fractions(self.total_steps, self.decay)[0] if self.line_search else [1.0]
            # candidate 0 is theta_old itself (0 * s adds zeros): Loss/Pi before the step comes out of the same kernel and the
            # same summation as the candidates' losses it is compared with
            fr = torch.tensor([0.0] + fracs, dtype=torch.float32, device=obs.device)
            cand = fm.surrogate_kl(step_dir, fr, obs, act, adv, logp_old, mu_old, log_std)
            sums = _avg(cand[:, [0, 1, 3]].contiguous())
            loss_c = -sums[:, 0] / B - self.entropy_coef * ent
            kl_c = sums[:, 1] / (B * A)
            ratio_c = sums[:, 2] / B
            bad = _avg(cand[:, 2].contiguous())
            step_norm = torch.norm(fr[:, None] * step_dir[None, :], dim=1)  # |f * s| as torch forms the step (f rounded to f32)
            # the one host read of the step
            vals = torch.cat([torch.stack([xHx, alpha, torch.norm(g), torch.norm(x), ent]), loss_c, kl_c, ratio_c, bad,
                              step_norm]).tolist()
        xhx, alpha_f, g_norm, x_norm, ent = vals[:5]
        J = len(fracs) + 1
        loss_c, kl_c, ratio_c, bad, step_norm = (vals[5 + k * J:5 + (k + 1) * J] for k in range(5))
        lb = loss_c[0]
        if not (math.isfinite(xhx) and math.isfinite(x_norm)):
            if not math.isfinite(lb):
                # a poisoned batch: the parameters stay, learn_one_epoch's guard reports it
                return dict(loss_pi=lb, delta_pi=float("nan"), kl=float("nan"), entropy=ent, ratio=ratio_c[0], acceptance_step=0,
                            alpha=alpha_f, final_step_norm=0.0, gradient_norm=g_norm, xHx=xhx, h_inv_g=x_norm, candidates=[])
            raise FloatingPointError("NPG: the conjugate-gradient solution is not finite")
        if xhx < 0:
            raise FloatingPointError(f"NPG: x.Fx = {xhx} < 0")
        accept = 1
        if self.line_search:
            accept = 0
            for j in range(1, J):
                if bad[j] != 0 or not math.isfinite(loss_c[j]) or lb - loss_c[j] < 0 or kl_c[j] > self.target_kl * 1.5:
                    continue
                accept = j
                break
        with torch.no_grad():
            if accept:
                # the same expression (and bits) as the candidate the kernel evaluated: theta_old + f * s
                _set_flat(params, theta_old + fracs[accept - 1] * step_dir)
        return dict(loss_pi=lb, delta_pi=loss_c[accept] - lb, kl=kl_c[accept], entropy=ent, ratio=ratio_c[accept],
                    acceptance_step=accept, alpha=alpha_f, final_step_norm=step_norm[accept], gradient_norm=g_norm, xHx=xhx,
                    h_inv_g=x_norm, candidates=list(zip(loss_c[1:], kl_c[1:])) if self.line_search else [])

    def _progress_columns(self):
        cols = super()._progress_columns()
        i = [c for c, _ in cols].index("Misc/StopIter")
        return cols[:i] + [("KL", "kl"), ("Loss/DeltaPi", "delta_pi"), ("Misc/AcceptanceStep", "acceptance_step"),
                           ("Misc/Alpha", "alpha"), ("Misc/FinalStepNorm", "final_step_norm"),
                           ("Misc/gradient_norm", "gradient_norm"), ("Misc/xHx", "xHx"), ("Misc/H_inv_g", "h_inv_g")] + cols[i:]


class TRPOTrainer(NPGTrainer):
    """TRPOAlgorithm (algs/trpo/trpo.py): NPG with the backtracking line search -- total_steps (15) candidates
    theta_old + decay^j alpha x, decay 0.8 (trainer arguments, as adjust_step_direction's); the first one whose loss did not rise and whose KL(p_old || q) stays within
    1.5 target_kl is taken, none: no step (AcceptanceStep 0)."""
    line_search = True
