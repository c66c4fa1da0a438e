"""Soft Actor-Critic on the batched simulator: the reference's off-policy trainer (algs/sac/sac.py) with its update on fused
HIP kernels.

What is restated from the reference: the networks (SquashedGaussianMLPActor / MLPQFunction / MLPActorCritic, sac.py:35-124,
with the `state_dict` keys `pi.net.N.*`, `pi.mu_layer.*`, `pi.log_std_layer.*`, `q1.q.N.*`, `q2.q.N.*`), the two losses
(compute_loss_q / compute_loss_pi, sac.py:295-337: the backup samples the CURRENT policy and takes the min of the twin TARGET
Qs; the policy loss is alpha logp - min(Q1, Q2)), the update order (one Adam step over both Qs, the actor step against the
UPDATED Qs, polyak, sac.py:439-474), the uniform warm-up and the sampled action afterwards (sac.py:393-410), and the logged
columns (sac.py:374-391).  The temperature alpha is fixed, as in the reference.

Two quirks of the reference are recorded here and not reproduced as bugs:
  * `roll_out` uses an undefined `done` (sac.py:417, 430), like DDPG's since the gymnasium migration.  The rollout here
    follows its intent as ddpg.py does: done = terminated or truncated, the stored terminal flag is `terminated & ~truncated`,
    and next_o is info['final_obs'] where the env finished.
  * `self.q_params` is an itertools.chain that the Adam constructor exhausts (sac.py:216-232), so `freeze` / `unfreeze`
    (sac.py:453, 463) are no-ops: loss_pi.backward() also accumulates gradients in the Qs, which the next
    q_optimizer.zero_grad() discards.  No value depends on this; here the Qs are simply only read by the policy step.
The reference's polyak loop runs over all of ac.parameters(); the target actor is never read (the backup samples the current
policy), so only q1 and q2 are averaged here and `ac_targ.pi` stays at its initial values.

The actor's two heads are ONE contiguous Linear(h2, 8) (`pi.head`, rows 0 .. 3 = mu_layer, rows 4 .. 7 = log_std_layer): that
is the pds_mlp the kernels read.  state_dict() / load_state_dict() split and join it at that boundary, so a `model.pt` written
here loads into the reference's MLPActorCritic and the other way round.

The noise is an ARGUMENT of the losses: eps2 for the backup's sample, eps for the policy loss's.  SACTrainer draws both from
the noise contract of the kernels (the variates of pds_gaussian_sample for sample id = position in the
mini-batch, under the update key, calls 2 u + 1 and 2 u + 2 of update u), on either path, so fused=True and fused=False see one
noise.

Batching is DDPGTrainer's (ddpg.py): a ring of `buffer_size / N` vector steps, `steps_per_epoch` vector steps per epoch,
`updates_per_step` updates after a vector step once `update_after` transitions are stored and `update_every` have passed.
One difference: the mini-batch rows are drawn WITHOUT repeats (SACTrainer.sample_rows), see there.
fused=True (csrc/pds_sac.hip): an update is seven launches on the rows `index` of the ring, read in place -- pds_sac_target,
pds_value_grad_step on q1 and on q2 (the same target rows; Adam acts per element, so two steps equal the reference's one
optimiser over both nets), the two launches of pds_sac_policy_grad, pds_polyak on q1 and q2.  fused=False is the same recipe in
torch autograd.  Shapes the kernels are not built for (D + 4 > 64, hidden sizes above 64 such as the reference's (400, 300))
take the autograd path; `trainer.fused` reports which path is in use.  fused_collect=True: after warm-up the vector steps up to
the next update are one pds_collect launch (ddpg.py, csrc/pds_collect.h); SAC already acts through pds_sac_sample, whose device
function the kernel calls, so a run with the flag on is bitwise the run with it off.  control_fused=True: the launch is
pds_collect_control, which also flies AttitudeRate / Attitude and the latency ring (ddpg.py).  Single process only."""
import math
import os
from copy import deepcopy

import torch
import torch.nn as nn
import torch.nn.functional as F

from .ddpg import ACT_DIM, FUSED_MAX_HIDDEN, FUSED_MAX_INPUT, DDPGQFunction, OffPolicyTrainer, ReplayBuffer
from .ppo import _mlp

LOG_STD_MAX, LOG_STD_MIN = 2.0, -20.0  # sac.py:31-32
_UPDATE_KEY = 0x5AC0F5E75AC0F5E7       # the update's Philox key is seed ^ this


def fused_supported(obs_dim, pi_hidden, q_hidden, pi_activation="relu", q_activation="relu"):
    """pds_sac_supported mirrored in Python (include/pds.h: "Built for D + 4 <= 64 and h1, h2 <= 64 of the three networks"):
    two hidden layers of at most 64 units, relu or tanh, D + 4 <= 64; q1 and q2 share q_hidden / q_activation."""
    ok = lambda h: len(h) == 2 and all(1 <= int(u) <= FUSED_MAX_HIDDEN for u in h)
    return (1 <= int(obs_dim) and int(obs_dim) + ACT_DIM <= FUSED_MAX_INPUT and ok(pi_hidden) and ok(q_hidden) and
            pi_activation in ("relu", "tanh") and q_activation in ("relu", "tanh"))


def squashed_sample(head, eps, act_limit):
    """[mu | log_std] rows -> (a, logp) of SquashedGaussianMLPActor.forward (sac.py:47-76) at the noise eps:
    u = mu + exp(clamp(log_std)) * eps, a = act_limit * tanh(u), logp = Normal(mu, std).log_prob(u).sum(-1) minus the tanh
    correction sum 2 (log 2 - u - softplus(-2 u)).  With eps held fixed the Gaussian term is -0.5 eps^2 - log_std -
    0.5 log 2 pi; softplus(-2 u) is -logsigmoid(2 u), the stable form at both ends."""
    A = head.shape[-1] // 2
    mu, log_std = head[..., :A], torch.clamp(head[..., A:], LOG_STD_MIN, LOG_STD_MAX)
    u = mu + torch.exp(log_std) * eps
    logp = (-0.5 * eps * eps - log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    logp = logp - (2.0 * (math.log(2.0) - u + F.logsigmoid(2.0 * u))).sum(-1)
    return act_limit * torch.tanh(u), logp


class SACActor(nn.Module):
    """SquashedGaussianMLPActor (sac.py:35-76): the trunk `net` (its output activation is the hidden activation) and the two
    heads stacked into `head` = Linear(h2, 2 * act_dim); the state dict keeps the reference's mu_layer / log_std_layer keys."""

    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit):
        super().__init__()
        layers = list(_mlp([obs_dim] + list(hidden_sizes) + [2 * act_dim], activation))
        self.net = nn.Sequential(*layers[:2 * len(hidden_sizes)])  # Linear, act, Linear, act: the reference's indices 0, 2
        self.head = layers[2 * len(hidden_sizes)]
        self.act_dim, self.act_limit = int(act_dim), float(act_limit)
        self._register_state_dict_hook(self._split_head)
        self._register_load_state_dict_pre_hook(self._join_head)

    @staticmethod
    def _split_head(module, state_dict, prefix, local_metadata):
        A = module.act_dim
        w, b = state_dict.pop(prefix + "head.weight"), state_dict.pop(prefix + "head.bias")
        for name, rows in (("mu_layer", slice(0, A)), ("log_std_layer", slice(A, 2 * A))):
            state_dict[prefix + name + ".weight"], state_dict[prefix + name + ".bias"] = w[rows], b[rows]

    def _join_head(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        keys = [prefix + n + t for t in (".weight", ".bias") for n in ("mu_layer", "log_std_layer")]
        if all(k in state_dict for k in keys):
            mw, lw, mb, lb = (state_dict.pop(k) for k in keys)
            state_dict[prefix + "head.weight"], state_dict[prefix + "head.bias"] = torch.cat([mw, lw], 0), torch.cat([mb, lb], 0)

    def heads(self, obs):
        """[mu | log_std] (unclamped): what pds_mlp_forward gives for the stacked network"""
        return self.head(self.net(obs))

    def forward(self, obs, eps=None, deterministic=False):
        head = self.heads(obs)
        if deterministic:
            eps = torch.zeros_like(head[..., :self.act_dim])
        elif eps is None:
            eps = torch.randn_like(head[..., :self.act_dim])
        return squashed_sample(head, eps, self.act_limit)


SACQFunction = DDPGQFunction  # MLPQFunction (sac.py:79-88) is ddpg.py's: Sequential `q` on [obs | act]


class SACActorCritic(nn.Module):
    """MLPActorCritic (sac.py:91-123).  ac_kwargs: {"pi": {"hidden_sizes", "activation"}, "q": {...}} -- q1 and q2 are both built
    from "q"; default (64, 64) relu for both (the reference's (400, 300) is accepted; it runs on the autograd path)."""

    def __init__(self, obs_dim, act_dim=ACT_DIM, ac_kwargs=None, act_limit=1.0):
        super().__init__()
        kw = {"pi": {"hidden_sizes": (64, 64), "activation": "relu"}, "q": {"hidden_sizes": (64, 64), "activation": "relu"}}
        for k, v in (ac_kwargs or {}).items():
            kw[k] = {**kw[k], **v}
        self.ac_kwargs = kw
        self.pi = SACActor(obs_dim, act_dim, kw["pi"]["hidden_sizes"], kw["pi"]["activation"], act_limit)
        self.q1 = SACQFunction(obs_dim, act_dim, kw["q"]["hidden_sizes"], kw["q"]["activation"])
        self.q2 = SACQFunction(obs_dim, act_dim, kw["q"]["hidden_sizes"], kw["q"]["activation"])

    def act(self, obs, deterministic=False, eps=None):
        with torch.no_grad():
            return self.pi(obs, eps, deterministic)[0]


# ---- the reference's losses and update, as free functions (float32 or float64, any device); the noise is an argument ------
def loss_q(ac, ac_targ, data, gamma, alpha, eps2):
    """compute_loss_q (sac.py:295-322) -> (loss, {"q1", "q2"}: the Q values)"""
    o, a, r, o2, d = data["obs"], data["act"], data["rew"], data["obs2"], data["done"]
    q1, q2 = ac.q1(o, a), ac.q2(o, a)
    with torch.no_grad():
        a2, logp_a2 = ac.pi(o2, eps2)  # the CURRENT policy
        q_pi_targ = torch.min(ac_targ.q1(o2, a2), ac_targ.q2(o2, a2))
        backup = r + gamma * (1 - d) * (q_pi_targ - alpha * logp_a2)
    return ((q1 - backup) ** 2).mean() + ((q2 - backup) ** 2).mean(), dict(q1=q1.detach(), q2=q2.detach())


def loss_pi(ac, data, alpha, eps):
    """compute_loss_pi (sac.py:324-337) -> (loss, logp)"""
    o = data["obs"]
    pi, logp_pi = ac.pi(o, eps)
    q_pi = torch.min(ac.q1(o, pi), ac.q2(o, pi))
    return (alpha * logp_pi - q_pi).mean(), logp_pi.detach()


def polyak_update(ac, ac_targ, polyak):
    """sac.py:469-474 on the Q networks (the target actor is never read): two in-place ops per tensor"""
    with torch.no_grad():
        for net, net_targ in ((ac.q1, ac_targ.q1), (ac.q2, ac_targ.q2)):
            for p, p_targ in zip(net.parameters(), net_targ.parameters()):
                p_targ.data.mul_(polyak)
                p_targ.data.add_((1 - polyak) * p.data)


def autograd_update(ac, ac_targ, pi_optimizer, q_optimizer, data, gamma, alpha, polyak, eps2, eps):
    """update (sac.py:439-474): one step of the optimiser over both Qs, one actor step against the updated Qs (only read),
    polyak.  -> (loss_q, loss_pi, logp, {"q1", "q2"}) as tensors"""
    q_optimizer.zero_grad()
    lq, qvals = loss_q(ac, ac_targ, data, gamma, alpha, eps2)
    lq.backward()
    q_optimizer.step()
    q_params = list(ac.q1.parameters()) + list(ac.q2.parameters())
    for p in q_params:
        p.requires_grad = False
    pi_optimizer.zero_grad()
    lp, logp = loss_pi(ac, data, alpha, eps)
    lp.backward()
    pi_optimizer.step()
    for p in q_params:
        p.requires_grad = True
    polyak_update(ac, ac_targ, polyak)
    return lq.detach(), lp.detach(), logp, qvals


class SACTrainer(OffPolicyTrainer):
    """SAC on a DroneVecEnv (auto_reset).  Hyper-parameters under the reference's names (sac.py:127-150); the defaults are
    starting values, not tuned ones.  steps_per_epoch, updates_per_step, buffer_size: as DDPGTrainer."""

    def __init__(self, env, ac_kwargs=None, alpha=0.2, gamma=0.99, polyak=0.995, lr=1e-3, mini_batch_size=64, start_steps=10000,
                 update_after=1000, update_every=50, buffer_size=int(1e6), epochs=100, steps_per_epoch=64, updates_per_step=1,
                 seed=0, fused=True, fused_collect=False, control_fused=False):
        if not getattr(env, "_auto_reset", True):
            raise ValueError("SACTrainer needs an env with auto_reset=True")
        if int(env.act_dim) != ACT_DIM:
            raise ValueError(f"act_dim = {env.act_dim}")
        self.env, self.N, self.D = env, int(env.num_envs), int(env.obs_dim)
        self.alpha, self.gamma, self.polyak, self.lr = float(alpha), float(gamma), float(polyak), float(lr)
        self.mini_batch_size = int(mini_batch_size)
        self.start_steps = self.warmup_steps = int(start_steps)  # (warmup_steps: the loop's name for it)
        self.update_after, self.update_every = int(update_after), int(update_every)
        self.epochs, self.steps_per_epoch, self.updates_per_step = int(epochs), int(steps_per_epoch), int(updates_per_step)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.update_seed = self.seed ^ _UPDATE_KEY
        if self.mini_batch_size < 1 or self.steps_per_epoch < 1 or self.updates_per_step < 0 or not 0.0 < self.polyak < 1.0:
            raise ValueError("mini_batch_size, steps_per_epoch >= 1, updates_per_step >= 0, 0 < polyak < 1")
        dev = env.device
        self.act_limit = float(env.action_space.high[0])
        torch.manual_seed(seed)
        self.ac = SACActorCritic(self.D, env.act_dim, ac_kwargs, self.act_limit).to(dev)
        self.ac_targ = deepcopy(self.ac)
        for p in self.ac_targ.parameters():  # only moved by polyak averaging
            p.requires_grad = False
        kw = self.ac.ac_kwargs
        cap = (int(buffer_size) // self.N) * self.N
        if cap < self.N:
            raise ValueError(f"buffer_size = {buffer_size} holds less than one vector step of {self.N} envs")
        self.buffer = ReplayBuffer(cap, self.D, dev, num_envs=self.N, act_dim=env.act_dim, seed=self.seed)
        self.fused = bool(fused) and fused_supported(self.D, kw["pi"]["hidden_sizes"], kw["q"]["hidden_sizes"],
                                                     kw["pi"]["activation"], kw["q"]["activation"])
        if self.fused:
            from .fused import FusedMLP, sac_supported
            pa, qa = kw["pi"]["activation"], kw["q"]["activation"]
            self.fm_pi = FusedMLP(list(self.ac.pi.net) + [self.ac.pi.head], pa)
            self.fm_q1, self.fm_q2 = FusedMLP(self.ac.q1.q, qa), FusedMLP(self.ac.q2.q, qa)
            self.fm_q1_targ, self.fm_q2_targ = FusedMLP(self.ac_targ.q1.q, qa), FusedMLP(self.ac_targ.q2.q, qa)
            if not sac_supported(self.fm_pi, self.fm_q1, self.fm_q2):
                raise RuntimeError("pds_sac_supported disagrees with sac.fused_supported")  # (the two are pinned by a test)
            self.target_rows = torch.zeros(cap, device=dev)
        else:
            self.pi_optimizer = torch.optim.Adam(self.ac.pi.parameters(), lr=self.lr)
            self.q_optimizer = torch.optim.Adam(list(self.ac.q1.parameters()) + list(self.ac.q2.parameters()), lr=self.lr)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed((self.seed + 1) & 0x7FFFFFFFFFFFFFFF)
        self._act = torch.empty(self.N, env.act_dim, device=dev)
        self._zeros4 = torch.zeros(env.act_dim, device=dev)
        self._noise_calls = 0
        self._init_loop()
        from .fused import COLLECT_SAC
        self._init_collect(fused_collect, COLLECT_SAC, control_fused=control_fused)
        self._last = None  # (loss_q, loss_pi, mean logp, index) of the latest update, device tensors

    # ---- acting ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _heads(self, obs):
        return self.fm_pi.forward(obs) if self.fused else self.ac.pi.heads(obs).contiguous()

    @torch.no_grad()
    def policy_action(self, obs):
        """act_limit * tanh(mu(obs)), no noise (the reference's deterministic=True)"""
        from .fused import sac_sample
        return sac_sample(self._heads(obs), self.act_limit, self.seed, 0, deterministic=True)[0]

    @torch.no_grad()
    def get_action(self, obs):
        """sac.py:402-408: uniform in [-1, 1] during warm-up (action_space.sample), afterwards the squashed-Gaussian sample of
        the actor -- pds_mlp_forward, then pds_sac_sample under (seed, env row, call)."""
        if self.in_warm_up:
            return torch.rand(self.N, self.env.act_dim, device=obs.device, generator=self.gen) * 2.0 - 1.0
        from .fused import sac_sample
        self._noise_calls += 1
        return sac_sample(self._heads(obs), self.act_limit, self.seed, self._noise_calls, act_out=self._act, want_logp=False)[0]

    # ---- the update --------------------------------------------------------------------------------------------------------
    def update_noise(self, B, call):
        """eps [B, 4] of the noise contract under the update key: what the kernels draw for `call`"""
        from .fused import gaussian_sample
        dev = self.env.device
        eps, logp = torch.empty(B, ACT_DIM, device=dev), torch.empty(B, device=dev)
        gaussian_sample(torch.zeros(B, ACT_DIM, device=dev), self._zeros4, eps, logp, self.update_seed, call)
        return eps

    def sample_rows(self, batch_size):
        """int64 row indices [batch_size], uniform over the filled rows and DISTINCT (the head of pds_permutation under the
        update key, one launch), where the reference draws with repeats: pds_sac_target writes the backup at the ROW while its
        noise belongs to the POSITION, so a row drawn twice would hold whichever of its two backups was written last.  Falls
        back to ReplayBuffer.sample_indices when the mini-batch is larger than the fill level."""
        if batch_size > len(self.buffer):
            return self.buffer.sample_indices(batch_size)
        from .fused import random_permutation
        return random_permutation(len(self.buffer), self.update_seed, self.updates, self.env.device)[:batch_size]

    def update(self, index=None):
        """One SAC update (sac.py:439-474) on the rows `index` of the buffer (default: sample_rows(mini_batch_size))."""
        buf = self.buffer
        index = self.sample_rows(self.mini_batch_size) if index is None else index
        B = index.shape[0]
        c_targ, c_pi = 2 * self.updates + 1, 2 * self.updates + 2
        if self.fused:
            from .fused import polyak, sac_target
            sac_target(self.fm_pi, self.fm_q1_targ, self.fm_q2_targ, buf.obs2, index, buf.rew, buf.done, self.gamma, self.alpha,
                       self.act_limit, self.update_seed, c_targ, self.target_rows)
            s1 = self.fm_q1.value_grad(buf.oa, self.target_rows, index=index, adam_lr=self.lr)
            s2 = self.fm_q2.value_grad(buf.oa, self.target_rows, index=index, adam_lr=self.lr)
            sp = self.fm_pi.sac_policy_grad(self.fm_q1, self.fm_q2, buf.oa, index, self.alpha, self.act_limit, self.update_seed,
                                            c_pi, adam_lr=self.lr)
            polyak(self.fm_q1_targ, self.fm_q1, self.polyak)
            polyak(self.fm_q2_targ, self.fm_q2, self.polyak)
            # (new tensors: the stats buffers are rewritten by the next update)
            self._last = ((s1[0] + s2[0]) / B, (self.alpha * sp[1] - sp[0]) / B, sp[1] / B, index)
        else:
            lq, lp, logp, _ = autograd_update(self.ac, self.ac_targ, self.pi_optimizer, self.q_optimizer, buf.batch(index),
                                              self.gamma, self.alpha, self.polyak, self.update_noise(B, c_targ),
                                              self.update_noise(B, c_pi))
            self._last = (lq, lp, logp.mean(), index)
        self.updates += 1

    def _update_info(self):
        """LossQ, LossPi, LogPi and the twin Q values of the latest update (zeros during warm-up, sac.py:435-437)"""
        info = dict(loss_q=0.0, loss_pi=0.0, log_pi=0.0)
        for n in ("q1", "q2"):
            info.update({f"{n}_mean": 0.0, f"{n}_min": 0.0, f"{n}_max": 0.0})
        if self._last is not None:
            lq, lp, logp, index = self._last
            info.update(loss_q=float(lq), loss_pi=float(lp), log_pi=float(logp))
            with torch.no_grad():
                b = self.buffer.batch(index)
                for n, q in (("q1", self.ac.q1), ("q2", self.ac.q2)):
                    qv = q(b["obs"], b["act"])
                    info.update({f"{n}_mean": float(qv.mean()), f"{n}_min": float(qv.min()), f"{n}_max": float(qv.max())})
            if not (math.isfinite(info["loss_q"]) and math.isfinite(info["loss_pi"])):
                raise FloatingPointError(f"non-finite loss in epoch {self.epoch + 1}")
        return info

    # ---- artefacts ---------------------------------------------------------------------------------------------------------
    def save_checkpoint(self, log_dir):
        """`torch_save/model.pt` = SACActorCritic.state_dict() under the reference module's keys."""
        os.makedirs(os.path.join(log_dir, "torch_save"), exist_ok=True)
        path = os.path.join(log_dir, "torch_save", "model.pt")
        torch.save({k: v.detach().cpu().clone() for k, v in self.ac.state_dict().items()}, path)
        return path

    def _progress_columns(self):
        """(progress.csv column, log key) pairs: the columns of SoftActorCriticAlgorithm.log (sac.py:374-391)"""
        return [("Epoch", "epoch"), ("EpRet/Mean", "ep_ret"), ("EpRet/Min", "ep_ret_min"), ("EpRet/Max", "ep_ret_max"),
                ("EpRet/Std", "ep_ret_std"), ("EpLen/Mean", "ep_len"), ("EpLen/Min", "ep_len_min"), ("EpLen/Max", "ep_len_max"),
                ("Q1Vals/Mean", "q1_mean"), ("Q1Vals/Min", "q1_min"), ("Q1Vals/Max", "q1_max"),
                ("Q2Vals/Mean", "q2_mean"), ("Q2Vals/Min", "q2_min"), ("Q2Vals/Max", "q2_max"), ("LogPi", "log_pi"),
                ("LossPi", "loss_pi"), ("LossQ", "loss_q"), ("InWarmUp", "in_warm_up"), ("TotalEnvSteps", "total_env_steps"),
                ("Time", "time"), ("FPS", "fps")]
