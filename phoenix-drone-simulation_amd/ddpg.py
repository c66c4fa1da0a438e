"""DDPG on the batched simulator: the reference's off-policy trainer (algs/ddpg/ddpg.py) with its update on fused HIP kernels.

What is restated from the reference: the networks (MLPActor / MLPQFunction / MLPActorCritic, ddpg.py:27-85, with the
`state_dict` keys `pi.pi.N.*` / `q.q.N.*`), the two losses (compute_loss_q / compute_loss_pi, ddpg.py:316-340), the update
order (Q step, actor step against the UPDATED Q, polyak on both nets, ddpg.py:431-464), the exploration action and the
uniform warm-up (ddpg.py:342-345, 393-400), and the logged columns (ddpg.py:374-383).

The reference's `roll_out` cannot run as written: `done` is undefined at ddpg.py:409,422 since its gymnasium migration.  The
rollout here follows its intent: done = terminated or truncated, and the stored terminal flag is false when the TimeLimit cut
the episode (`terminated & ~truncated`).

What batching changes: one vector step stores N transitions, so the replay buffer is a ring of `capacity / N` vector steps,
`steps_per_epoch` counts vector steps, and `updates_per_step` gradient updates follow every vector step once `update_after`
transitions are stored and `update_every` transitions have passed since the last round (the reference's ratio of one update
per transition is updates_per_step = num_envs).  The defaults are starting values, not tuned ones.

fused=True (csrc/pds_ddpg.hip, fused.py): a mini-batch is read IN PLACE through its row index -- pds_ddpg_target writes the
Bellman backup at the rows, pds_value_grad_step takes the Q step on `oa[index]`, pds_ddpg_policy_grad differentiates
-Q(o, pi(o)).mean() through Q into the actor and takes its Adam step, pds_polyak moves the targets: six launches, no gather
copy, no autograd graph.  fused=False is the same recipe in torch autograd (torch.optim.Adam), and is what the kernels are
tested against.  fused_collect=True (csrc/pds_collect.h): once warm-up is over, the vector steps up to the next update are ONE
launch of pds_collect -- actor, exploration noise, env step, the ring rows, the episode statistics -- where step_env issues
about three dozen; `trainer.collect_fused` reports whether that kernel runs (pds_collect_supported: control_mode PWM, history 2,
no latency / hold / ground effect; control_fused=True asks pds_collect_control instead, which also flies AttitudeRate / Attitude
and the latency ring on Hover and Circle, include/pds_collect_control.h -- the default False keeps every answer as it was).  With the flag on, DDPG acts through pds_ddpg_explore on the per-step path too (tanhf where
fused_collect=False calls torch.tanh: the one documented difference between the two settings).
Shapes the kernels are not built for (D + 4 > 64: observation_history_size >= 4, TakeOff from 3; hidden
sizes above 64, e.g. the reference's (400, 300)) take the autograd path; `trainer.fused` reports which path is in use.
broad_fused=True (csrc/pds_mlp_broad.hip, csrc/pds_ddpg_broad.hip, include/pds_mlp_broad.h): hidden sizes above 64, up to 512 in
both networks, run the same six-step update and the policy action on kernels that keep the weights in L2 -- nine launches an
update; `trainer.broad` reports it.  The keyword changes nothing for shapes up to 64, the collection under it stays per step
(`collect_fused` is False), and the default False keeps every answer as it was.
Single process only."""
import math
import os
import time
from copy import deepcopy

import torch
import torch.nn as nn

from .ppo import _mlp

# the limits of csrc/pds_ddpg.hip (include/pds.h: "Built for D + 4 <= 64 and h1, h2 <= 64 of both networks")
FUSED_MAX_INPUT = 64
FUSED_MAX_HIDDEN = 64
# ... and of csrc/pds_ddpg_broad.hip (include/pds_mlp_broad.h), which broad_fused=True asks for: widths above 64 up to this
BROAD_MAX_HIDDEN = 512
# broad_fused=True keeps the autograd path from this mini-batch size upward: at (400, 300) the fused update was measured faster
# than autograd at 128 .. 16384 rows and slower at 32768 and 65536 (profiles/ddpg_broad_timing.txt, README.md); sizes between
# 16384 and 32768 were not measured
BROAD_AUTOGRAD_FROM = 32768
# ... and policy_action of a broad trainer is the torch module from this many rows (envs) upward: the fused forward was measured
# faster at 128 .. 8192 rows and slower from 16384 on (the same file)
BROAD_ACTION_TORCH_FROM = 16384
ACT_DIM = 4


def fused_supported(obs_dim, pi_hidden, q_hidden, pi_activation="relu", q_activation="relu", broad=False):
    """pds_ddpg_supported mirrored in Python: two hidden layers of at most 64 units, relu or tanh, D + 4 <= 64.
    broad=True: pds_ddpg_broad_supported (include/pds_mlp_broad.h) instead -- two hidden layers of at most 512 units with one
    above 64, in BOTH networks; the shapes of the first question get False from this one."""
    if broad:
        ok = lambda h: len(h) == 2 and all(1 <= int(u) <= BROAD_MAX_HIDDEN for u in h) and max(int(u) for u in h) > FUSED_MAX_HIDDEN
    else:
        ok = lambda h: len(h) == 2 and all(1 <= int(u) <= FUSED_MAX_HIDDEN for u in h)
    return (1 <= int(obs_dim) and int(obs_dim) + ACT_DIM <= FUSED_MAX_INPUT and ok(pi_hidden) and ok(q_hidden) and
            pi_activation in ("relu", "tanh") and q_activation in ("relu", "tanh"))


class DDPGActor(nn.Module):
    """MLPActor (ddpg.py:27-38): act_limit * tanh(pi(obs)); the tanh is applied here, so `pi` holds the Linear layers under the
    reference's indices 0, 2, 4."""

    def __init__(self, obs_dim, act_dim, hidden_sizes, activation, act_limit):
        super().__init__()
        self.pi = _mlp([obs_dim] + list(hidden_sizes) + [act_dim], activation)
        self.act_limit = float(act_limit)

    def forward(self, obs):
        return self.act_limit * torch.tanh(self.pi(obs))


class DDPGQFunction(nn.Module):
    """MLPQFunction (ddpg.py:41-50) on [obs | act]"""

    def __init__(self, obs_dim, act_dim, hidden_sizes, activation):
        super().__init__()
        self.q = _mlp([obs_dim + act_dim] + list(hidden_sizes) + [1], activation)

    def forward(self, obs, act):
        return torch.squeeze(self.q(torch.cat([obs, act], dim=-1)), -1)


class DDPGActorCritic(nn.Module):
    """MLPActorCritic (ddpg.py:53-85).  ac_kwargs: {"pi": {"hidden_sizes", "activation"}, "q": {...}}; default (64, 64) relu
    for both (the reference's (400, 300) is accepted; it runs on the autograd path unless DDPGTrainer gets broad_fused=True)."""

    def __init__(self, obs_dim, act_dim=ACT_DIM, ac_kwargs=None, act_limit=1.0):
        super().__init__()
        kw = {"pi": {"hidden_sizes": (64, 64), "activation": "relu"}, "q": {"hidden_sizes": (64, 64), "activation": "relu"}}
        for k, v in (ac_kwargs or {}).items():
            kw[k] = {**kw[k], **v}
        self.ac_kwargs = kw
        self.pi = DDPGActor(obs_dim, act_dim, kw["pi"]["hidden_sizes"], kw["pi"]["activation"], act_limit)
        self.q = DDPGQFunction(obs_dim, act_dim, kw["q"]["hidden_sizes"], kw["q"]["activation"])

    def act(self, obs):
        with torch.no_grad():
            return self.pi(obs)


# ---- the reference's losses and update, as free functions (float32 or float64, any device) --------------------------------
def loss_q(ac, ac_targ, data, gamma):
    """compute_loss_q (ddpg.py:316-334) -> (loss, Q values)"""
    o, a, r, o2, d = data["obs"], data["act"], data["rew"], data["obs2"], data["done"]
    q = ac.q(o, a)
    with torch.no_grad():
        q_pi_targ = ac_targ.q(o2, ac_targ.pi(o2))
        backup = r + gamma * (1 - d) * q_pi_targ
    return ((q - backup) ** 2).mean(), q.detach()


def loss_pi(ac, data):
    """compute_loss_pi (ddpg.py:336-340)"""
    o = data["obs"]
    return -ac.q(o, ac.pi(o)).mean()


def polyak_update(ac, ac_targ, polyak):
    """ddpg.py:459-464: two in-place ops per tensor"""
    with torch.no_grad():
        for p, p_targ in zip(ac.parameters(), ac_targ.parameters()):
            p_targ.data.mul_(polyak)
            p_targ.data.add_((1 - polyak) * p.data)


def autograd_update(ac, ac_targ, pi_optimizer, q_optimizer, data, gamma, polyak):
    """update (ddpg.py:431-464): one Q step, one actor step against the updated (frozen) Q, polyak.  -> (loss_q, loss_pi, Q
    values) as tensors"""
    q_optimizer.zero_grad()
    lq, qvals = loss_q(ac, ac_targ, data, gamma)
    lq.backward()
    q_optimizer.step()
    for p in ac.q.parameters():
        p.requires_grad = False
    pi_optimizer.zero_grad()
    lp = loss_pi(ac, data)
    lp.backward()
    pi_optimizer.step()
    for p in ac.q.parameters():
        p.requires_grad = True
    polyak_update(ac, ac_targ, polyak)
    return lq.detach(), lp.detach(), qvals


def collect_steps(since_update, update_every, N, steps_left_in_epoch):
    """Vector steps of one pds_collect launch: up to the next point at which an update can happen -- the first step at which
    `since_update >= update_every` holds, max(1, ceil((update_every - since_update) / N)) steps ahead -- and not past the epoch."""
    ahead = -((int(since_update) - int(update_every)) // int(N))  # ceil((update_every - since_update) / N)
    return max(1, min(max(1, ahead), int(steps_left_in_epoch)))


class ReplayBuffer:
    """A ring of transitions on one device, filled N rows per vector step: oa [capacity, D + 4] = [obs | act] (the Q network's
    input, read in place by the fused kernels), obs2 [capacity, D], rew, done [capacity] (done as 0. / 1.).  `capacity` must
    be a multiple of the rows stored per step, so a vector step never straddles the wrap-around."""

    def __init__(self, capacity, obs_dim, device, num_envs=None, act_dim=ACT_DIM, seed=0):
        self.capacity, self.obs_dim, self.act_dim = int(capacity), int(obs_dim), int(act_dim)
        if self.capacity < 1:
            raise ValueError(f"capacity = {capacity}")
        self.num_envs = None
        self._check_rows(num_envs)
        f32 = dict(dtype=torch.float32, device=device)
        self.oa = torch.zeros(self.capacity, self.obs_dim + self.act_dim, **f32)
        self.obs2 = torch.zeros(self.capacity, self.obs_dim, **f32)
        self.rew = torch.zeros(self.capacity, **f32)
        self.done = torch.zeros(self.capacity, **f32)
        self.ptr, self.size = 0, 0
        self.gen = torch.Generator(device=device)
        self.gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)

    def _check_rows(self, n):
        if n is None:
            return
        n = int(n)
        if n < 1 or self.capacity % n != 0:
            raise ValueError(f"replay capacity {self.capacity} is not a multiple of num_envs = {n}")
        if self.num_envs is not None and n != self.num_envs:
            raise ValueError(f"{n} rows stored into a ring of {self.num_envs} rows per step")
        self.num_envs = n

    def __len__(self):
        return self.size

    def store(self, obs, act, rew, next_obs, done):
        """one vector step: N rows at the ring position"""
        n = obs.shape[0]
        self._check_rows(n)
        s = slice(self.ptr, self.ptr + n)
        self.oa[s, :self.obs_dim] = obs
        self.oa[s, self.obs_dim:] = act
        self.obs2[s] = next_obs
        self.rew[s] = rew
        self.done[s] = done
        self.ptr = (self.ptr + n) % self.capacity
        self.size = min(self.size + n, self.capacity)

    def advance(self, k):
        """move ptr / size as k store() calls would (the rows were written in place: pds_collect)"""
        if self.num_envs is None:
            raise ValueError("advance() before the rows per step are known")
        rows = int(k) * self.num_envs
        if k < 0:
            raise ValueError(f"k = {k}")
        self.ptr = (self.ptr + rows) % self.capacity
        self.size = min(self.size + rows, self.capacity)

    def sample_indices(self, batch_size):
        """int64 row indices [batch_size], uniform over the filled rows (with repeats), from the buffer's seeded generator"""
        if self.size < 1:
            raise ValueError("the replay buffer is empty")
        return torch.randint(0, self.size, (int(batch_size),), generator=self.gen, device=self.oa.device)

    def batch(self, index):
        """the gathered mini-batch of the autograd path, in the reference's keys"""
        oa = self.oa[index]
        return dict(obs=oa[:, :self.obs_dim], act=oa[:, self.obs_dim:], rew=self.rew[index], obs2=self.obs2[index],
                    done=self.done[index])


class OffPolicyTrainer:
    """The vector-step / update / epoch loop the off-policy trainers share (DDPGTrainer here, sac.SACTrainer).  A subclass
    sets env, N, buffer, warmup_steps, update_after, update_every, steps_per_epoch, updates_per_step and epochs, calls
    _init_loop() and _init_collect(), and provides get_action(obs), update(), _update_info() and _progress_columns()."""

    fused_collect = False   # the constructor's keyword
    control_fused = False   # ... and the one that lets pds_collect_control take the collection (PID control modes, latency ring)
    collect_fused = False   # ... and whether pds_collect / pds_collect_control runs after warm-up
    collect_launches = 0

    def _init_loop(self):
        dev = self.env.device
        self.obs = None
        self.ep_ret, self.ep_len = torch.zeros(self.N, device=dev), torch.zeros(self.N, device=dev)
        self.in_warm_up = True
        self.total_steps, self.updates, self._since_update = 0, 0, 0
        self.epoch, self.log, self._t_total = 0, [], 0.0

    def _init_collect(self, fused_collect, mode, log_std=None, control_fused=False):
        """fused_collect=True: one pds_collect launch per stretch of vector steps between updates, where the kernel is built for the
        env and the actor `fm_pi` (mode: fused.COLLECT_DDPG / COLLECT_SAC; log_std: DDPG's [4] log noise scale).  control_fused=True
        (it changes nothing without fused_collect=True): the launch is pds_collect_control, built for the PID control modes and the
        latency ring as well."""
        self.fused_collect, self.control_fused = bool(fused_collect), bool(control_fused)
        self._collect_mode, self._collect_log_std = mode, log_std
        self.collect_fused, self.collect_launches, self._cobs = False, 0, None
        if self.fused_collect and self.fused and not getattr(self, "broad", False):  # (a broad actor collects per step)
            from .fused import collect_control_supported, collect_supported
            supported = collect_control_supported if self.control_fused else collect_supported
            self.collect_fused = supported(self.env, self.fm_pi, mode)

    # ---- K vector steps in one launch ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def collect(self, k):
        """k vector steps of step_env + the episode bookkeeping of learn_one_epoch as one pds_collect launch (after warm-up only:
        the actions are the policy's).  -> the launch's [tiles, 8] statistics slab"""
        from .fused import collect_tiles, fused_collect
        if self.obs is None:
            self.obs, _ = self.env.reset()
        if self._cobs is None:
            self._cobs = torch.empty_like(self.obs)  # (the env owns the tensors its step() returns)
        if self.obs is not self._cobs:
            self._cobs.copy_(self.obs)
            self.obs = self._cobs
        self.in_warm_up = False
        buf = self.buffer
        slab = torch.empty(collect_tiles(self.env), 8, device=self.env.device)
        fused_collect(self.env, self.fm_pi, self._collect_mode, k, self.act_limit, self._collect_log_std, self.seed,
                      self._noise_calls + 1, buf.oa, buf.obs2, buf.rew, buf.done, buf.ptr, self._cobs, self.ep_ret, self.ep_len, slab,
                      control=self.control_fused)
        self._noise_calls += k
        buf.advance(k)
        self.collect_launches += 1
        self.total_steps += k * self.N
        self._since_update += k * self.N
        return slab

    # ---- one vector step -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step_env(self, act=None):
        """act (default: get_action) -> env.step -> N transitions into the buffer.  next_o is info['final_obs'] where the env
        finished (the returned observation is already the reset one), the terminal flag is terminated & ~truncated.
        -> (reward, done)"""
        if self.obs is None:
            self.obs, _ = self.env.reset()
        o = self.obs
        self.in_warm_up = len(self.buffer) < self.warmup_steps
        a = self.get_action(o) if act is None else act
        next_o, r, terminated, truncated, info = self.env.step(a)
        done = terminated | truncated
        stored_next = torch.where(done.unsqueeze(-1), info["final_obs"], next_o)
        self.buffer.store(o, a, r, stored_next, (terminated & ~truncated).to(torch.float32))
        self.obs = next_o
        self.total_steps += self.N
        self._since_update += self.N
        return r, done

    # ---- epochs ------------------------------------------------------------------------------------------------------------
    def learn_one_epoch(self):
        """steps_per_epoch vector steps with their updates -> the log entry: the loop's columns and those of _update_info()."""
        dev = self.env.device
        t0 = time.time()
        inf = float("inf")
        # finished episodes of the epoch: count, sum, sum of squares, min, max of the return; sum, min, max of the length
        acc = torch.tensor([0.0, 0.0, 0.0, inf, -inf, 0.0, inf, -inf], device=dev)
        steps_left, slabs = self.steps_per_epoch, []
        while steps_left > 0:
            if self.collect_fused and len(self.buffer) >= self.warmup_steps:
                k = collect_steps(self._since_update, self.update_every, self.N, steps_left)
                slabs.append(self.collect(k))
                steps_left -= k
            else:
                r, done = self.step_env()
                steps_left -= 1
                self.ep_ret += r
                self.ep_len += 1.0
                d = done.to(torch.float32)
                ret, ln = self.ep_ret, self.ep_len
                acc[0] += d.sum(); acc[1] += (d * ret).sum(); acc[2] += (d * ret * ret).sum()
                acc[3] = torch.minimum(acc[3], torch.where(done, ret, torch.full_like(ret, inf)).min())
                acc[4] = torch.maximum(acc[4], torch.where(done, ret, torch.full_like(ret, -inf)).max())
                acc[5] += (d * ln).sum()
                acc[6] = torch.minimum(acc[6], torch.where(done, ln, torch.full_like(ln, inf)).min())
                acc[7] = torch.maximum(acc[7], torch.where(done, ln, torch.full_like(ln, -inf)).max())
                self.ep_ret = torch.where(done, torch.zeros_like(ret), ret)
                self.ep_len = torch.where(done, torch.zeros_like(ln), ln)
            if (not self.in_warm_up and len(self.buffer) >= self.update_after and self._since_update >= self.update_every):
                for _ in range(self.updates_per_step):
                    self.update()
                self._since_update = 0
        info = dict(epoch=self.epoch + 1, in_warm_up=float(self.in_warm_up), total_env_steps=self.total_steps,
                    updates=self.updates)
        info.update(self._update_info())
        if slabs:  # the launches' per-tile statistics, once per epoch: three reductions, read back with `acc` in one copy
            t = torch.cat(slabs)
            v = torch.cat([acc, t.sum(0), t.min(0).values, t.max(0).values]).tolist()
            s, su, mn, mx = v[:8], v[8:16], v[16:24], v[24:32]
            s = [s[0] + su[0], s[1] + su[1], s[2] + su[2], min(s[3], mn[3]), max(s[4], mx[4]), s[5] + su[5], min(s[6], mn[6]),
                 max(s[7], mx[7])]
        else:
            s = acc.tolist()
        n = max(s[0], 1.0)
        mean = s[1] / n
        nan = float("nan")
        info.update(episodes=s[0], ep_ret=mean if s[0] else nan, ep_ret_min=s[3] if s[0] else nan, ep_ret_max=s[4] if s[0] else nan,
                    ep_ret_std=math.sqrt(max(s[2] / n - mean * mean, 0.0)) if s[0] else nan, ep_len=s[5] / n if s[0] else nan,
                    ep_len_min=s[6] if s[0] else nan, ep_len_max=s[7] if s[0] else nan)
        dt = time.time() - t0
        self._t_total += dt
        info.update(time=self._t_total, fps=self.steps_per_epoch * self.N / dt)
        self.log.append(info)
        self.epoch += 1
        return info

    def learn(self, epochs=None, verbose=False):
        for _ in range(epochs or self.epochs):
            info = self.learn_one_epoch()
            if verbose:
                print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in info.items()})
        return self.ac, self.env

    def write_progress_csv(self, path):
        """The per-epoch log, one row per epoch (the form of PPOTrainer.write_progress_csv)."""
        cols = self._progress_columns()
        with open(path, "w") as f:
            f.write(",".join(c for c, _ in cols) + "\n")
            for row in self.log:
                f.write(",".join(str(row.get(k, "")) for _, k in cols) + "\n")


class DDPGTrainer(OffPolicyTrainer):
    """DDPG on a DroneVecEnv (auto_reset).  Hyper-parameters under the reference's names (ddpg.py:89-114); the defaults are
    starting values, not tuned ones.  steps_per_epoch: vector steps per epoch; updates_per_step: gradient updates after each
    vector step once updating has begun (see the module docstring); buffer_size is rounded DOWN to a multiple of num_envs."""

    def __init__(self, env, ac_kwargs=None, gamma=0.99, polyak=0.995, pi_lr=1e-4, q_lr=1e-3, mini_batch_size=128,
                 act_noise=0.1, warmup_steps=10000, update_after=1000, update_every=50, buffer_size=int(1e6), epochs=100,
                 steps_per_epoch=64, updates_per_step=1, seed=0, fused=True, broad_fused=False, fused_collect=False,
                 control_fused=False):
        if not getattr(env, "_auto_reset", True):
            raise ValueError("DDPGTrainer needs an env with auto_reset=True")
        self.env, self.N, self.D = env, int(env.num_envs), int(env.obs_dim)
        self.gamma, self.polyak, self.pi_lr, self.q_lr = float(gamma), float(polyak), float(pi_lr), float(q_lr)
        self.mini_batch_size, self.act_noise = int(mini_batch_size), float(act_noise)
        self.warmup_steps, self.update_after, self.update_every = int(warmup_steps), int(update_after), int(update_every)
        self.epochs, self.steps_per_epoch, self.updates_per_step = int(epochs), int(steps_per_epoch), int(updates_per_step)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if self.mini_batch_size < 1 or self.steps_per_epoch < 1 or self.updates_per_step < 0 or not self.act_noise > 0:
            raise ValueError("mini_batch_size, steps_per_epoch >= 1, updates_per_step >= 0, act_noise > 0")
        dev = env.device
        self.act_limit = float(env.action_space.high[0])
        torch.manual_seed(seed)
        self.ac = DDPGActorCritic(self.D, env.act_dim, ac_kwargs, self.act_limit).to(dev)
        self.ac_targ = deepcopy(self.ac)
        kw = self.ac.ac_kwargs
        cap = (int(buffer_size) // self.N) * self.N
        if cap < self.N:
            raise ValueError(f"buffer_size = {buffer_size} holds less than one vector step of {self.N} envs")
        self.buffer = ReplayBuffer(cap, self.D, dev, num_envs=self.N, act_dim=env.act_dim, seed=self.seed)
        self.fused = bool(fused) and fused_supported(self.D, kw["pi"]["hidden_sizes"], kw["q"]["hidden_sizes"],
                                                     kw["pi"]["activation"], kw["q"]["activation"])
        # broad_fused=True: hidden widths above 64 (the reference's default (400, 300)) run on the kernels of
        # include/pds_mlp_broad.h; a shape the kernels above cover is untouched by the keyword
        self.broad = (bool(fused) and bool(broad_fused) and not self.fused and self.mini_batch_size < BROAD_AUTOGRAD_FROM and
                      fused_supported(self.D, kw["pi"]["hidden_sizes"], kw["q"]["hidden_sizes"], kw["pi"]["activation"],
                                      kw["q"]["activation"], broad=True))
        self.fused = self.fused or self.broad
        if self.fused:
            from .fused import FusedMLP, ddpg_supported
            mk = lambda net, act: FusedMLP(net, act, broad=self.broad)
            self.fm_pi, self.fm_q = mk(self.ac.pi.pi, kw["pi"]["activation"]), mk(self.ac.q.q, kw["q"]["activation"])
            self.fm_pi_targ = mk(self.ac_targ.pi.pi, kw["pi"]["activation"])
            self.fm_q_targ = mk(self.ac_targ.q.q, kw["q"]["activation"])
            if not ddpg_supported(self.fm_pi, self.fm_q):
                raise RuntimeError("pds_ddpg_supported disagrees with ddpg.fused_supported")  # (the two are pinned by a test)
            self.target_rows = torch.zeros(cap, device=dev)
        else:
            self.pi_optimizer = torch.optim.Adam(self.ac.pi.parameters(), lr=self.pi_lr)
            self.q_optimizer = torch.optim.Adam(self.ac.q.parameters(), lr=self.q_lr)
        for p in self.ac_targ.parameters():  # only moved by polyak averaging
            p.requires_grad = False
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed((self.seed + 1) & 0x7FFFFFFFFFFFFFFF)
        self._log_noise = torch.full((env.act_dim,), math.log(self.act_noise), device=dev)
        self._act = torch.empty(self.N, env.act_dim, device=dev)
        self._logp = torch.empty(self.N, device=dev)
        self._noise_calls = 0
        self._init_loop()
        from .fused import COLLECT_DDPG
        self._init_collect(fused_collect, COLLECT_DDPG, self._log_noise, control_fused=control_fused)
        self._last = None  # (loss_q, loss_pi, index) of the latest update, device tensors

    # ---- acting ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def policy_action(self, obs):
        """act_limit * tanh(pi(obs)), no noise"""
        if self.fused and not (self.broad and obs.shape[0] >= BROAD_ACTION_TORCH_FROM):
            return self.act_limit * torch.tanh(self.fm_pi.forward(obs))
        return self.ac.pi(obs)

    @torch.no_grad()
    def get_action(self, obs):
        """get_action (ddpg.py:342-345): clip(pi(o) + act_noise * z, -limit, limit), z from pds_gaussian_sample (DESIGN.md
        section 4: Philox keyed by (seed, env row, call)); uniform in [-1, 1] during warm-up (action_space.sample)."""
        if self.in_warm_up:
            return torch.rand(self.N, self.env.act_dim, device=obs.device, generator=self.gen) * 2.0 - 1.0
        if self.fused_collect and self.fused:  # the action rule of pds_collect as its elementwise entry point (tanhf)
            from .fused import ddpg_explore
            self._noise_calls += 1
            return ddpg_explore(self.fm_pi.forward(obs), self._log_noise, self.act_limit, self.seed, self._noise_calls,
                                act_out=self._act)
        from .fused import gaussian_sample
        mu = self.policy_action(obs).contiguous()
        self._noise_calls += 1
        gaussian_sample(mu, self._log_noise, self._act, self._logp, self.seed, self._noise_calls)
        return torch.clamp(self._act, -self.act_limit, self.act_limit)

    # ---- the update --------------------------------------------------------------------------------------------------------
    def update(self, index=None):
        """One DDPG update (ddpg.py:431-464) on the rows `index` of the buffer (default: sample_indices(mini_batch_size))."""
        buf = self.buffer
        index = buf.sample_indices(self.mini_batch_size) if index is None else index
        B = index.shape[0]
        if self.fused:
            from .fused import ddpg_target, polyak
            ddpg_target(self.fm_pi_targ, self.fm_q_targ, buf.obs2, index, buf.rew, buf.done, self.gamma, self.act_limit,
                        self.target_rows)
            sq = self.fm_q.value_grad(buf.oa, self.target_rows, index=index, adam_lr=self.q_lr)
            sp = self.fm_pi.ddpg_policy_grad(self.fm_q, buf.oa, index, self.act_limit, adam_lr=self.pi_lr)
            polyak(self.fm_pi_targ, self.fm_pi, self.polyak)
            polyak(self.fm_q_targ, self.fm_q, self.polyak)
            self._last = (sq[0] / B, -sp[0] / B, index)  # (new tensors: the stats buffers are rewritten by the next update)
        else:
            lq, lp, _ = autograd_update(self.ac, self.ac_targ, self.pi_optimizer, self.q_optimizer, buf.batch(index), self.gamma,
                                        self.polyak)
            self._last = (lq, lp, index)
        self.updates += 1

    def _update_info(self):
        """loss_q, loss_pi and the Q values of the latest update (zeros during warm-up, as the reference stores them,
        ddpg.py:427-429)"""
        info = dict(loss_q=0.0, loss_pi=0.0, q_mean=0.0, q_min=0.0, q_max=0.0)
        if self._last is not None:
            lq, lp, index = self._last
            with torch.no_grad():
                b = self.buffer.batch(index)
                qv = self.ac.q(b["obs"], b["act"])
            info.update(loss_q=float(lq), loss_pi=float(lp), q_mean=float(qv.mean()), q_min=float(qv.min()), q_max=float(qv.max()))
            if not (math.isfinite(info["loss_q"]) and math.isfinite(info["loss_pi"])):
                raise FloatingPointError(f"non-finite loss in epoch {self.epoch + 1}")
        return info

    # ---- artefacts ---------------------------------------------------------------------------------------------------------
    def save_checkpoint(self, log_dir):
        """`torch_save/model.pt` = DDPGActorCritic.state_dict() under the reference module's keys (pi.pi.N.*, q.q.N.*)."""
        os.makedirs(os.path.join(log_dir, "torch_save"), exist_ok=True)
        path = os.path.join(log_dir, "torch_save", "model.pt")
        torch.save({k: v.detach().cpu() for k, v in self.ac.state_dict().items()}, path)
        return path

    def _progress_columns(self):
        """(progress.csv column, log key) pairs: the columns of DeepDeterministicPolciyGradientAlgorithm.log (ddpg.py:374-383)"""
        return [("Epoch", "epoch"), ("EpRet/Mean", "ep_ret"), ("EpRet/Min", "ep_ret_min"), ("EpRet/Max", "ep_ret_max"),
                ("EpRet/Std", "ep_ret_std"), ("EpLen/Mean", "ep_len"), ("EpLen/Min", "ep_len_min"), ("EpLen/Max", "ep_len_max"),
                ("QVals/Mean", "q_mean"), ("QVals/Min", "q_min"), ("QVals/Max", "q_max"), ("LossPi", "loss_pi"),
                ("LossQ", "loss_q"), ("InWarmUp", "in_warm_up"), ("TotalEnvSteps", "total_env_steps"), ("Time", "time"),
                ("FPS", "fps")]
