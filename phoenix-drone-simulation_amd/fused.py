"""Host side of csrc/pds_mlp.hip: the trainer's dense work as fused HIP kernels
on the f32 matrix cores -- MLP forward for the rollout, PPO-clip policy gradient and value-regression
gradient for the update.  Each call replaces an autograd op chain of the reference trainer:

    FusedMLP.forward      ActorCritic.step / MLPGaussianActor.net / MLPCritic.net  algs/core.py:228-311,370-393
    FusedMLP.ppo_grad     compute_loss_pi + backward                                algs/ppo/ppo.py:22-40
    FusedMLP.value_grad   compute_loss_v + backward                                 algs/iwpg/iwpg.py:272-275
    FusedMLP.fisher_vector_product  NaturalPolicyGradientAlgorithm.Fvp              algs/npg/npg.py:52-77
    conjugate_gradients   conjugate_gradients                                       algs/utils.py:5-38
    FusedMLP.surrogate_kl the candidates of TRPO's line search                      algs/trpo/trpo.py:16-66
    FusedMLP.ddpg_policy_grad  compute_loss_pi + backward (through Q into the actor) algs/ddpg/ddpg.py:336-340
    ddpg_target           the Bellman backup of compute_loss_q                      algs/ddpg/ddpg.py:323-326
    polyak                the target networks' polyak step                          algs/ddpg/ddpg.py:459-464
    sac_sample            SquashedGaussianMLPActor.forward after its two heads      algs/sac/sac.py:47-76
    sac_target            the entropy-regularised backup of compute_loss_q          algs/sac/sac.py:303-311
    FusedMLP.sac_policy_grad  compute_loss_pi + backward (through min(Q1, Q2))      algs/sac/sac.py:324-337
    ddpg_explore          get_action's clip(pi(o) + noise) behind the actor         algs/ddpg/ddpg.py:342-345
    fused_collect         roll_out: K vector steps into the replay ring, one launch algs/ddpg/ddpg.py:393-429, algs/sac/sac.py:402-437

Networks with three or four hidden layers (csrc/pds_mlp_deep.hip, include/pds_mlp_deep.h) take the first three rows and
adam_step on kernels of their own (FusedMLP.deep); every other row takes two hidden layers and refuses them -- but for
fisher_vector_product and surrogate_kl of a FusedMLP built with npg_deep=True (csrc/pds_npg_deep.hip, include/pds_npg_deep.h);
fused_rollout_deep is the one-launch rollout under such an actor (csrc/pds_rollout_deep.h, include/pds_rollout_deep.h).
Two hidden layers with a width above 64, up to 512 -- the reference's (400, 300) for DDPG -- are FusedMLP(..., broad=True)
(csrc/pds_mlp_broad.hip, csrc/pds_ddpg_broad.hip, include/pds_mlp_broad.h): forward, value_grad, adam_step, ddpg_policy_grad,
ddpg_target and polyak run on kernels that keep the weights in L2; every other row refuses such a network.

The gradients are written straight into the `.grad` storage of the torch parameters (one flat
buffer, torch parameter order), so the optimiser step stays torch.optim.Adam like the reference's."""
import ctypes as C

import torch
import torch.nn as nn

from . import native

_ptr, _on = native._ptr, native.on_device  # (for direct calls; every launch below enters the library through native.call)
# the entry points behind FusedMLP.forward / ppo_grad / value_grad / adam_step: include/pds.h, include/pds_mlp_deep.h
_SHALLOW_CALLS = ("pds_mlp_forward", "pds_ppo_policy_grad_step", "pds_value_grad_step", "pds_adam_step")
_BROAD_CALLS = ("pds_mlp_broad_forward", None, "pds_mlp_broad_value_grad_step", "pds_mlp_broad_adam_step")  # include/pds_mlp_broad.h
_DEEP_CALLS = ("pds_mlp_deep_forward", "pds_mlp_deep_ppo_policy_grad_step", "pds_mlp_deep_value_grad_step", "pds_mlp_deep_adam_step")
# the entry points behind FusedMLP._npg_workspace / fisher_vector_product / surrogate_kl: include/pds.h, include/pds_npg_deep.h
_NPG_CALLS = ("pds_npg_workspace_floats", "pds_npg_fisher_vector_product", "pds_npg_surrogate_kl")
_NPG_DEEP_CALLS = ("pds_npg_deep_workspace_floats", "pds_npg_deep_fisher_vector_product", "pds_npg_deep_surrogate_kl")


def _refuse_deep(what, *fms):
    """NotImplementedError where a network with 3 or 4 hidden layers meets a kernel that takes struct pds_mlp (before any native call)"""
    for fm in fms:
        if getattr(fm, "deep", False):
            raise NotImplementedError(f"{what} takes networks with 2 hidden layers; this one has {fm.n_hidden} (the deep kernels of "
                                      "include/pds_mlp_deep.h cover forward, ppo_grad, value_grad and adam_step)")


class FusedMLP:
    """View of `nn.Sequential(Linear, act, Linear, act, Linear[, Identity])` as a struct pds_mlp (`m`; native.call re-binds its
    pointers wherever a FusedMLP is an argument) -- or, with 4 or 5 Linear layers (`deep` is True), as a struct pds_mlp_deep
    (include/pds_mlp_deep.h): forward, ppo_grad, value_grad, adam_step, flat_grad, stats and workspace are the same calls on the
    deep kernels, everything else that takes a struct pds_mlp raises NotImplementedError, and there is no `m`.
    npg_deep=True: on a deep network _npg_workspace, fisher_vector_product and surrogate_kl are the same calls too, on the kernels
    of include/pds_npg_deep.h (so conjugate_gradients works over them); on two hidden layers the keyword changes nothing.
    broad=True: a network with two hidden layers of which one is wider than 64 (up to 512; d_in <= 64) is accepted (`broad` is
    True): forward, value_grad, adam_step and ddpg_policy_grad are the same calls on the kernels of include/pds_mlp_broad.h,
    ppo_grad and everything else raise NotImplementedError.  On widths up to 64 the keyword changes nothing; without it such a
    network is refused as before."""

    def __init__(self, net, activation, npg_deep=False, broad=False):
        lin = [l for l in net if isinstance(l, nn.Linear)]
        if len(lin) not in (3, 4, 5) or activation not in native.ACTIVATIONS:
            raise NotImplementedError("fused kernels cover 2, 3 or 4 hidden layers with relu or tanh")
        self.lin = lin
        self.deep = len(lin) > 3
        self.n_hidden = len(lin) - 1
        self.params = [p for l in lin for p in (l.weight, l.bias)]
        for p in self.params:
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise ValueError("fused kernels need contiguous float32 parameters on the HIP device")
        self.lib = native.load()
        self.broad = bool(broad) and not self.deep and max(lin[0].out_features, lin[1].out_features) > 64
        if self.deep:
            self.md = m = native.mlp_deep(lin[0].in_features, [l.out_features for l in lin[:-1]], lin[-1].out_features, activation,
                                          tensors=self.params)
            n = self.lib.pds_mlp_deep_param_count(C.byref(m))
        else:
            self.m = m = native.mlp(lin[0].in_features, lin[0].out_features, lin[1].out_features, lin[2].out_features, activation,
                                    tensors=self.params)
            n = (self.lib.pds_mlp_broad_param_count if self.broad else self.lib.pds_mlp_param_count)(C.byref(m))
        if n < 0 and self.broad:
            raise ValueError("layer sizes outside the broad kernels' range (2 hidden layers: d_in <= 64, h1, h2 <= 512 with one of "
                             "them above 64, d_out <= 8)")
        if n < 0:
            raise ValueError("layer sizes outside the fused kernels' range (2 hidden layers: d_in <= 192, h1, h2 <= 64, d_out <= 8; "
                             "3 or 4 hidden layers: d_in <= 64, every hidden width <= 64, d_out <= 8)")
        if self.deep and self.lib.pds_mlp_deep_supported(C.byref(m)) != 1:
            raise NotImplementedError(f"the fused kernels for {self.n_hidden} hidden layers take d_in <= 64, not {m.d_in}")
        if self.broad and self.lib.pds_mlp_broad_supported(C.byref(m)) != 1:
            raise NotImplementedError(f"the fused kernels for hidden widths above 64 take d_in <= 64, not {m.d_in}")
        self._names = _DEEP_CALLS if self.deep else (_BROAD_CALLS if self.broad else _SHALLOW_CALLS)
        self.npg_deep = bool(npg_deep) and self.deep
        self._npg_names = _NPG_DEEP_CALLS if self.npg_deep else _NPG_CALLS
        dev = self.params[0].device
        self.flat_grad = torch.zeros(n, device=dev)
        off = 0
        for p in self.params:  # .grad of every parameter is a view into the flat buffer the kernel fills
            p.grad = self.flat_grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.stats = torch.zeros(4, device=dev)
        if self.broad:  # the activations of a whole batch, hundreds of MB: allocated by the first gradient call (_broad_workspace)
            self.workspace = None
            return
        ws = self.lib.pds_mlp_deep_workspace_floats(C.byref(m)) if self.deep else self.lib.pds_mlp_workspace_floats(C.byref(m))
        self.workspace = torch.empty(ws, device=dev)

    def _broad_workspace(self, attr, q_fm=None):
        """The workspace of a broad gradient call (pds_mlp_broad_workspace_floats; with `q_fm` pds_ddpg_broad_workspace_floats),
        kept in self.<attr>: a forward-only network (a target network) never allocates one."""
        ws = getattr(self, attr, None)
        if ws is None:
            n = (self.lib.pds_mlp_broad_workspace_floats(C.byref(self.m)) if q_fm is None else
                 self.lib.pds_ddpg_broad_workspace_floats(C.byref(self.m), C.byref(q_fm.m)))
            if n < 0:
                raise (NotImplementedError if n == native.EUNSUPPORTED else ValueError)(f"pds_*_broad_workspace_floats -> {n}")
            ws = torch.empty(n, device=self.flat_grad.device)
            setattr(self, attr, ws)
        return ws

    @property
    def d_out(self):
        return self.lin[-1].out_features

    def _bind(self):
        if self.deep:
            native.bind_mlp_deep(self.md, self.params)
        else:
            l = self.lin
            native.bind_mlp(self.m, (l[0].weight, l[0].bias, l[1].weight, l[1].bias, l[2].weight, l[2].bias))

    @staticmethod
    def _stream(t=None):
        """The caller's current stream ON THE TENSOR'S DEVICE, for a direct call (native.call appends it by itself)."""
        return C.c_void_p(torch.cuda.current_stream(t.device if t is not None else None).cuda_stream)

    def forward(self, x, index=None, mean=None, std=None, eps=1e-5, out=None):
        """y[B, d_out] = net(standardise(x[index]))."""
        B = x.shape[0] if index is None else index.shape[0]
        y = out if out is not None else torch.empty(B, self.d_out, device=x.device)
        native.call(self._names[0], self, x, index, B, mean, std, float(eps), y, on=x)
        return y

    def _adam_state(self):
        if not hasattr(self, "exp_avg"):
            self.exp_avg = torch.zeros_like(self.flat_grad)
            self.exp_avg_sq = torch.zeros_like(self.flat_grad)
            self.adam_steps = 0

    def _adam_arg(self, adam_lr, betas, eps):
        """pds_adam for a gradient call that also steps (None: gradient only)"""
        if adam_lr is None:
            return None
        self._adam_state()
        self.adam_steps += 1
        return C.byref(native.Adam(_ptr(self.exp_avg), _ptr(self.exp_avg_sq), self.adam_steps, float(adam_lr),
                                   float(betas[0]), float(betas[1]), float(eps)))

    def ppo_grad(self, x, act, adv, logp_old, log_std, clip_ratio, adam_lr=None, betas=(0.9, 0.999), eps=1e-8):
        """Fills the parameters' .grad with d loss_pi / d theta; returns the stats tensor
        [sum(-min(..)), sum(ratio), sum(0.5 z^2), B] (device, no sync).  adam_lr: also take the torch.optim.Adam step
        with this learning rate, in the same two launches (same bits as ppo_grad + adam_step)."""
        if self.broad:
            raise NotImplementedError("ppo_grad takes hidden widths up to 64 (include/pds_mlp_broad.h has forward, value_grad, "
                                      "adam_step and DDPG's update)")
        opt = self._adam_arg(adam_lr, betas, eps)
        native.call(self._names[1], self, x, act, adv, logp_old, log_std, x.shape[0], float(clip_ratio), self.flat_grad,
                    self.stats, self.workspace, opt, on=x)
        return self.stats

    def adam_step(self, lr, betas=(0.9, 0.999), eps=1e-8):
        """torch.optim.Adam.step for this network's parameters from the flat gradient, in one launch."""
        self._adam_state()
        self.adam_steps += 1
        native.call(self._names[3], self, self.flat_grad, self.exp_avg, self.exp_avg_sq, self.adam_steps, float(lr), float(betas[0]),
                    float(betas[1]), float(eps), on=self.flat_grad)

    def value_grad(self, x, target, index=None, adam_lr=None, betas=(0.9, 0.999), eps=1e-8):
        """Fills .grad with d mse(net(x[index]), target[index]) / d theta; stats[0] = sum of squared errors.
        adam_lr: as in ppo_grad."""
        B = x.shape[0] if index is None else index.shape[0]
        ws = self._broad_workspace("workspace") if self.broad else self.workspace
        opt = self._adam_arg(adam_lr, betas, eps)
        native.call(self._names[2], self, x, index, target, B, self.flat_grad, self.stats, ws, opt, on=x)
        return self.stats

    def _npg_workspace(self, candidates):
        if not self.npg_deep:
            _refuse_deep("the natural-gradient workspace (pds_npg_workspace_floats)", self)
        n = getattr(self.lib, self._npg_names[0])(C.byref(self.md if self.npg_deep else self.m), int(candidates))
        if n < 0:
            raise (NotImplementedError if n == native.EUNSUPPORTED else ValueError)(f"{self._npg_names[0]} -> {n}")
        ws = getattr(self, "npg_workspace", None)
        if ws is None or ws.numel() < n:
            self.npg_workspace = ws = torch.empty(n, device=self.flat_grad.device)
        return ws

    def fisher_vector_product(self, x, v, log_std, damping, index=None, out=None):
        """F v + damping v (flat, param_count) over the standardised rows x[index] (csrc/pds_npg.hip): the Fisher matrix of
        the Gaussian policy with the fixed log_std at the current parameters, mean over samples x action dims.  A network with 3
        or 4 hidden layers needs npg_deep=True at construction (csrc/pds_npg_deep.hip)."""
        if not self.npg_deep:
            _refuse_deep("fisher_vector_product (pds_npg_fisher_vector_product)", self)
        B = x.shape[0] if index is None else index.shape[0]
        out = out if out is not None else torch.empty_like(self.flat_grad)
        native.call(self._npg_names[1], self, x, index, B, log_std, v, float(damping), out, self._npg_workspace(0), on=x)
        return out

    def surrogate_kl(self, step, fracs, x, act, adv, logp_old, mu_old, log_std, theta_out=None):
        """[J, 4] device tensor: per candidate theta + fracs[j] * step (fracs: float32 device tensor [J]) the sum of ratio * adv
        over the batch, the sum of KL(Normal(mu_old, sigma) || Normal(mu_j, sigma)) over samples x action dims, a non-finite
        flag and the sum of ratio (csrc/pds_npg.hip).  theta_out [J, param_count]: also the candidates' parameters."""
        if not self.npg_deep:
            _refuse_deep("surrogate_kl (pds_npg_surrogate_kl)", self)
        J = int(fracs.shape[0])
        out = torch.empty(J, 4, device=x.device)
        native.call(self._npg_names[2], self, step, fracs, J, x, act, adv, logp_old, mu_old, log_std, x.shape[0], out, theta_out,
                    self._npg_workspace(J), on=x)
        return out

    def ddpg_policy_grad(self, q_fm, oa, index, act_limit, adam_lr=None, betas=(0.9, 0.999), eps=1e-8):
        """This network as the DDPG actor (output act_limit * tanh): fills .grad with the gradient of
        -Q(o, pi(o)).mean() over the rows oa[index] = [obs | act] (index None: every row), Q = `q_fm` (read only);
        stats[0] = sum of Q(o, pi(o)), stats[3] = B (csrc/pds_ddpg.hip).  adam_lr: as in ppo_grad.
        NotImplementedError for shapes the kernel is not built for (ddpg_supported says so beforehand).  A broad actor takes a
        broad Q (csrc/pds_ddpg_broad.hip)."""
        _refuse_deep("ddpg_policy_grad (pds_ddpg_policy_grad)", self, q_fm)
        B = oa.shape[0] if index is None else index.shape[0]
        if self.broad:
            ws = self._broad_workspace("ddpg_workspace", q_fm)
            opt = self._adam_arg(adam_lr, betas, eps)
            native.call("pds_ddpg_broad_policy_grad", self, q_fm, oa, index, B, float(act_limit), self.flat_grad, self.stats, ws, opt,
                        on=oa)
            return self.stats
        ws = getattr(self, "ddpg_workspace", None)
        if ws is None:
            n = self.lib.pds_ddpg_workspace_floats(C.byref(self.m), C.byref(q_fm.m))
            if n < 0:
                raise (NotImplementedError if n == native.EUNSUPPORTED else ValueError)(f"pds_ddpg_workspace_floats -> {n}")
            self.ddpg_workspace = ws = torch.empty(n, device=self.flat_grad.device)
        opt = self._adam_arg(adam_lr, betas, eps)
        native.call("pds_ddpg_policy_grad", self, q_fm, oa, index, B, float(act_limit), self.flat_grad, self.stats, ws, opt, on=oa)
        return self.stats

    def sac_policy_grad(self, q1_fm, q2_fm, oa, index, alpha, act_limit, seed, call, adam_lr=None, betas=(0.9, 0.999), eps=1e-8):
        """This network as the SAC actor (d_out = 8: [mu | log_std]): fills .grad with the gradient of
        (alpha logp - min(Q1, Q2)(o, a)).mean() over the rows oa[index] = [obs | act] (index None: every row), a and logp the
        squashed-Gaussian sample under the noise of (seed, call); Q1, Q2 = `q1_fm`, `q2_fm` (read only).  stats = [sum min Q,
        sum logp, 0, B] (csrc/pds_sac.hip).  adam_lr: as in ppo_grad.  NotImplementedError for shapes the kernel is not built
        for (sac_supported says so beforehand)."""
        _refuse_deep("sac_policy_grad (pds_sac_policy_grad)", self, q1_fm, q2_fm)
        B = oa.shape[0] if index is None else index.shape[0]
        ws = getattr(self, "sac_workspace", None)
        if ws is None:
            n = self.lib.pds_sac_workspace_floats(C.byref(self.m), C.byref(q1_fm.m), C.byref(q2_fm.m))
            if n < 0:
                raise (NotImplementedError if n == native.EUNSUPPORTED else ValueError)(f"pds_sac_workspace_floats -> {n}")
            self.sac_workspace = ws = torch.empty(n, device=self.flat_grad.device)
        opt = self._adam_arg(adam_lr, betas, eps)
        native.call("pds_sac_policy_grad", self, q1_fm, q2_fm, oa, index, B, float(alpha), float(act_limit),
                    int(seed) & (2 ** 64 - 1), int(call), self.flat_grad, self.stats, ws, opt, on=oa)
        return self.stats


def ddpg_supported(pi_fm, q_fm):
    """True when the fused DDPG kernels cover this actor / Q pair (D + 4 <= 64, hidden <= 64, d_out 4 / 1)."""
    _refuse_deep("ddpg_supported (pds_ddpg_supported)", pi_fm, q_fm)
    if pi_fm.broad or q_fm.broad:  # (include/pds_mlp_broad.h: both networks with a hidden width above 64, up to 512)
        return pi_fm.broad and q_fm.broad and native.load().pds_ddpg_broad_supported(C.byref(pi_fm.m), C.byref(q_fm.m)) == 1
    return native.load().pds_ddpg_supported(C.byref(pi_fm.m), C.byref(q_fm.m)) == 1


def ddpg_target(pi_targ_fm, q_targ_fm, obs2, index, rew, done, gamma, act_limit, target_rows):
    """target_rows[i] = rew[i] + gamma * (1 - done[i]) * Q_targ(obs2[i], act_limit * tanh(pi_targ(obs2[i]))) for the rows
    i = index[g] (index None: every row); the other rows are left alone (include/pds.h pds_ddpg_target)."""
    _refuse_deep("ddpg_target (pds_ddpg_target)", pi_targ_fm, q_targ_fm)
    B = obs2.shape[0] if index is None else index.shape[0]
    native.call("pds_ddpg_broad_target" if pi_targ_fm.broad else "pds_ddpg_target", pi_targ_fm, q_targ_fm, obs2, index, B, rew, done, float(gamma), float(act_limit), target_rows,
                on=obs2)
    return target_rows


def polyak(targ_fm, src_fm, rho):
    """p_targ.mul_(rho); p_targ.add_((1 - rho) * p) over the six tensors of a network pair, one launch, the same bits."""
    _refuse_deep("polyak (pds_polyak)", targ_fm, src_fm)
    native.call("pds_polyak_broad" if targ_fm.broad else "pds_polyak", targ_fm, src_fm, float(rho), on=targ_fm.params[0])


def sac_supported(pi_fm, q1_fm, q2_fm):
    """True when the fused SAC kernels cover this actor / twin-Q triple (D + 4 <= 64, hidden <= 64, d_out 8 / 1 / 1)."""
    _refuse_deep("sac_supported (pds_sac_supported)", pi_fm, q1_fm, q2_fm)
    return native.load().pds_sac_supported(C.byref(pi_fm.m), C.byref(q1_fm.m), C.byref(q2_fm.m)) == 1


def sac_sample(head, act_limit, seed, call, id_base=0, deterministic=False, act_out=None, want_logp=True):
    """(a [n, 4], logp [n] or None) from the actor's output head [n, 8] = [mu | log_std]: the clamped, reparameterised,
    tanh-squashed sample with its log-probability (include/pds.h pds_sac_sample); eps of row i = the variates of
    pds_gaussian_sample for sample id id_base + i in `call` under `seed`."""
    if head.dim() != 2 or head.shape[1] != 8 or not head.is_contiguous() or head.dtype != torch.float32:
        raise ValueError("head must be a contiguous float32 [n, 8] tensor")
    n = head.shape[0]
    act = act_out if act_out is not None else torch.empty(n, 4, device=head.device)
    logp = torch.empty(n, device=head.device) if want_logp else None
    native.call("pds_sac_sample", head, n, float(act_limit), int(seed) & (2 ** 64 - 1), int(call), int(id_base),
                int(bool(deterministic)), act, logp, on=head)
    return act, logp


def sac_target(pi_fm, q1_targ_fm, q2_targ_fm, obs2, index, rew, done, gamma, alpha, act_limit, seed, call, target_rows):
    """target_rows[i] = rew[i] + gamma * (1 - done[i]) * (min(Q1_targ, Q2_targ)(obs2[i], a2) - alpha * logp2) for the rows
    i = index[g] (index None: every row), (a2, logp2) the sample of the CURRENT policy `pi_fm` under the noise of (seed, call)
    at position g; the other rows are left alone (include/pds.h pds_sac_target)."""
    _refuse_deep("sac_target (pds_sac_target)", pi_fm, q1_targ_fm, q2_targ_fm)
    B = obs2.shape[0] if index is None else index.shape[0]
    native.call("pds_sac_target", pi_fm, q1_targ_fm, q2_targ_fm, obs2, index, B, rew, done, float(gamma), float(alpha),
                float(act_limit), int(seed) & (2 ** 64 - 1), int(call), target_rows, on=obs2)
    return target_rows


COLLECT_DDPG, COLLECT_SAC = 0, 1  # `mode` of pds_collect (include/pds.h)


def ddpg_explore(net_out, log_std, act_limit, seed, call, id_base=0, act_out=None):
    """a [n, 4] = clamp(act_limit * tanh(net_out) + exp(log_std) * z, -act_limit, act_limit) from the actor's pre-tanh output
    net_out [n, 4] (include/pds.h pds_ddpg_explore); z of row i = the variates of pds_gaussian_sample for sample id
    id_base + i in `call` under `seed`.  The device function the network waves of pds_collect call."""
    if net_out.dim() != 2 or net_out.shape[1] != 4 or not net_out.is_contiguous() or net_out.dtype != torch.float32:
        raise ValueError("net_out must be a contiguous float32 [n, 4] tensor")
    n = net_out.shape[0]
    act = act_out if act_out is not None else torch.empty(n, 4, device=net_out.device)
    native.call("pds_ddpg_explore", net_out, log_std, n, float(act_limit), int(seed) & (2 ** 64 - 1), int(call), int(id_base), act,
                on=net_out)
    return act


def collect_supported(env, fm_pi, mode):
    """True when pds_collect has a kernel for this env and actor in this mode (COLLECT_DDPG: d_out 4, COLLECT_SAC: d_out 8)."""
    _refuse_deep("collect_supported (pds_collect_supported)", fm_pi)
    return env.lib.pds_collect_supported(env._handle, C.byref(fm_pi.m), int(mode)) == 1


def collect_control_supported(env, fm_pi, mode):
    """True when pds_collect_control (include/pds_collect_control.h) has a kernel for this env and actor in this mode: wherever
    collect_supported holds, and on Hover and Circle under control_mode AttitudeRate / Attitude and / or with the latency ring
    (noise off or the reference's default, with and without motor dynamics)."""
    _refuse_deep("collect_control_supported (pds_collect_control_supported)", fm_pi)
    return env.lib.pds_collect_control_supported(env._handle, C.byref(fm_pi.m), int(mode)) == 1


def collect_tiles(env):
    """rows of the [tiles, 8] statistics slab of one fused_collect launch"""
    return (int(env.num_envs) + 63) // 64


def fused_collect(env, fm_pi, mode, K, act_limit, log_std, seed, first_call, oa, obs2, rew, done, ptr, obs, ep_ret, ep_len,
                  tile_stats, control=False):
    """ONE launch for K closed-loop vector steps of an off-policy trainer (include/pds.h pds_collect, csrc/pds_collect.h): step s
    fills the N rows at (ptr + s N) mod capacity of the ring oa / obs2 / rew / done (capacity = oa.shape[0]), obs [N, D] is
    o(0) on entry and o(K) on return, ep_ret / ep_len run on, tile_stats [collect_tiles(env), 8] receives the finished episodes'
    statistics.  control=True: pds_collect_control (include/pds_collect_control.h), which also flies the PID control modes and
    the latency ring -- collect_control_supported -- and is the same launch wherever pds_collect has one.  Raises
    NotImplementedError / ValueError where the entry point refuses (the env is left as it was)."""
    _refuse_deep("fused_collect (pds_collect)", fm_pi)
    native.call("pds_collect_control" if control else "pds_collect", env._handle, int(K), int(mode), fm_pi, float(act_limit), log_std, int(seed) & (2 ** 64 - 1),
                int(first_call), oa, obs2, rew, done, int(oa.shape[0]), int(ptr), obs, ep_ret, ep_len, tile_stats,
                on=obs, handle=env._handle)
    env._last_obs = obs  # (what a masked reset() copies for the envs outside the mask)


def conjugate_gradients(avp, b, iters, residual_tol=1e-10, eps=1e-6):
    """conjugate_gradients (algs/utils.py:5-38) with one pds_npg_cg_step launch per iteration: `avp(p, out)` writes A p into
    out.  The reference's early break is a device flag that freezes x, r and p (no host sync).  -> (x, state) with state =
    {r.r, stopped} on the device."""
    n = b.numel()
    x, r, p, z = (torch.empty_like(b) for _ in range(4))
    st = torch.zeros(2, device=b.device)

    def step(zz, init):
        native.call("pds_npg_cg_step", n, x, r, p, zz, st, float(eps), float(residual_tol), int(init), on=b)

    step(b, True)
    for _ in range(int(iters)):
        avp(p, z)
        step(z, False)
    return x, st


def random_permutation(n, seed, call, device):
    """int64 tensor p with p[i] = a pseudo-random permutation of range(n) keyed by (seed, call): one launch
    (include/pds.h pds_permutation) where torch.randperm sorts."""
    out = torch.empty(int(n), dtype=torch.int64, device=device)
    native.call("pds_permutation", out, int(n), int(seed) & (2 ** 64 - 1), int(call), on=out)
    return out


def counter_add(counter, inc):
    """counter (int64 device tensor of one element) += inc, stream-ordered (captured-rollout call counter)."""
    native.call("pds_counter_add", counter, int(inc), on=counter)


def fused_rollout(env, fm_pi, fm_v, T, mean, std, eps, log_std, seed, call_offset, deterministic, obs_buf, act_buf, logp_buf,
                  val_buf, rew_buf, term_buf, trunc_buf, cost_buf, fval_buf, last_val, ep_ret, ep_len, stats, call_base=None):
    """ONE launch for the T closed-loop steps of a rollout (include/pds.h pds_rollout, csrc/pds_rollout.h): obs_buf is
    [T + 1, N, D] with o(0) in row 0.  Raises NotImplementedError for env configurations the kernel is not built
    for (the per-step path gives the same bits)."""
    _refuse_deep("fused_rollout (pds_rollout)", fm_pi, fm_v)
    native.call("pds_rollout", env._handle, int(T), fm_pi, fm_v, mean, std, float(eps), log_std, int(seed), call_base,
                int(call_offset), int(bool(deterministic)), obs_buf, act_buf, logp_buf, val_buf, rew_buf, term_buf, trunc_buf,
                cost_buf, fval_buf, last_val, ep_ret, ep_len, stats, on=obs_buf, handle=env._handle)


def rollout_history_latency_supported(env):
    """True where pds_rollout_history_latency (include/pds_history_latency.h) flies this env's rollout in one launch: an env created
    with history_latency=True on the latency ring, Hover or Circle in any control mode, noise off or the reference's default -- and
    no set_latency call since the env's last full reset (the kernel counts the steps of the rule from the handle's own step count,
    which knows nothing of the views such a call froze: those envs step per step until then)."""
    if not getattr(env, "history_latency", False) or getattr(env, "_hist_frozen", False):
        return False
    return native.load().pds_rollout_history_latency_supported(env._handle, int(env.observation_history_size)) == 1


def fused_rollout_history(env, fm_pi, T, H, mean, std, eps, log_std, seed, call_offset, deterministic, obs_buf, act_buf, logp_buf,
                          rew_buf, term_buf, trunc_buf, cost_buf, fin_rows, fin_step, ep_ret, ep_len, stats, call_base=None,
                          latency=False):
    """ONE launch for the T closed-loop steps of a rollout with observation_history_size = H != 2 (include/pds.h
    pds_rollout_history, csrc/pds_rollout_hist.h): obs_buf is [T + 1, N, H * half] with the current histories in row 0; the critic
    is NOT in the kernel (the caller evaluates V over obs_buf and over the final histories in fin_rows [slots, N, H * half],
    whose fin_step [slots, N] (int32, preset to -1) names the step each belongs to).  Raises NotImplementedError for env
    configurations the kernel is not built for (the per-step path gives the same bits).  latency=True: pds_rollout_history_latency
    (include/pds_history_latency.h), the same launch on the latency ring of an env created with history_latency=True."""
    _refuse_deep("fused_rollout_history (pds_rollout_history)", fm_pi)
    if latency and not rollout_history_latency_supported(env):
        raise NotImplementedError("pds_rollout_history_latency: not built for this env (rollout_history_latency_supported)")
    native.call("pds_rollout_history_latency" if latency else "pds_rollout_history", env._handle, int(T), int(H), fm_pi, mean, std, float(eps), log_std, int(seed), call_base,
                int(call_offset), int(bool(deterministic)), obs_buf, act_buf, logp_buf, rew_buf, term_buf, trunc_buf, cost_buf,
                fin_rows, fin_step, int(fin_rows.shape[0]), ep_ret, ep_len, stats, on=obs_buf, handle=env._handle)


def rollout_deep_supported(env, fm_pi):
    """True where pds_rollout_deep (include/pds_rollout_deep.h) flies this env's rollout in one launch under this actor: 3 or 4
    hidden layers, observation_history_size 2, control_mode PWM without latency ring or Kalman hold, every noise setting, motor
    dynamics on Hover and Circle, the ground effect on TakeOff."""
    if not getattr(fm_pi, "deep", False) or getattr(env, "observation_history_size", 2) != 2:
        return False
    return native.load().pds_rollout_deep_supported(env._handle, C.byref(fm_pi.md)) == 1


def fused_rollout_deep(env, fm_pi, T, mean, std, eps, log_std, seed, call_offset, deterministic, obs_buf, act_buf, logp_buf,
                       rew_buf, term_buf, trunc_buf, cost_buf, fin_rows, fin_step, ep_ret, ep_len, stats, call_base=None):
    """ONE launch for the T closed-loop steps of a rollout under an actor with 3 or 4 hidden layers (include/pds_rollout_deep.h
    pds_rollout_deep, csrc/pds_rollout_deep.h): obs_buf is [T + 1, N, D] with o(0) in row 0; the critic is NOT in the kernel (the
    caller evaluates V over obs_buf and over the final observations in fin_rows [slots, N, D], whose fin_step [slots, N] (int32,
    preset to -1) names the step each belongs to).  Raises NotImplementedError where the kernel is not built, before the env is
    touched (the per-step path gives the same bits)."""
    if not rollout_deep_supported(env, fm_pi):
        raise NotImplementedError("pds_rollout_deep: not built for this env and actor (rollout_deep_supported)")
    native.call("pds_rollout_deep", env._handle, int(T), fm_pi, mean, std, float(eps), log_std, int(seed), call_base,
                int(call_offset), int(bool(deterministic)), obs_buf, act_buf, logp_buf, rew_buf, term_buf, trunc_buf, cost_buf,
                fin_rows, fin_step, int(fin_rows.shape[0]), ep_ret, ep_len, stats, on=obs_buf, handle=env._handle)


def gaussian_sample(mu, log_std, act_out, logp_out, seed, call, id_base=0, deterministic=False, call_base=None):
    """act_out[n, d] = mu + exp(log_std) * z, logp_out[n] = log N(act | mu, sigma) summed over d.  The Philox
    call counter is `call` (+ the int64 device word `call_base` when given: hipGraph-capturable form)."""
    native.call("pds_gaussian_sample_dev", mu, log_std, mu.shape[0], mu.shape[1], int(seed), call_base, int(call), int(id_base),
                int(bool(deterministic)), act_out, logp_out, on=mu)


def rollout_record(rew, term, trunc, rew_buf_t, term_buf_t, trunc_buf_t, ep_ret, ep_len, stats):
    """One step of the rollout bookkeeping (see include/pds.h pds_rollout_record)."""
    native.call("pds_rollout_record", rew, term, trunc, rew.shape[0], rew_buf_t, term_buf_t, trunc_buf_t, ep_ret, ep_len, stats, on=rew)
