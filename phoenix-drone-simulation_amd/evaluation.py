"""Batched counterpart of EnvironmentEvaluator (utils/evaluation.py:15-117): one evaluation episode per
env of the batch, all in lockstep on the device.

The reference runs `num_evaluations` episodes one after the other (`eval_once`: reset, act
deterministically until terminated or truncated, sum reward and info['cost']) and writes one value
per line to `returns.csv` / `costs.csv`.  Here every env of the vector env plays exactly one
episode: the accumulators of an env freeze at its first `terminated | truncated`, and the loop ends
after `max_episode_steps` steps at the latest (TimeLimit).

`evaluate_population` scores a whole POPULATION of policies that way -- a checkpoint sweep, model selection during training,
an evolution strategy over actor weights -- in one launch: P policies x E episodes (include/pds.h pds_evaluate_policies).
With `metrics=True` the same launch also reports the flight-quality sums the reference tabulates per real flight
(experiments/02_zero_shot_policy_transfer_hover_task/02_eval_hover_task.py): `FlightMetrics`; `metrics_from_arrays` scores a
logged flight by the same definitions.  With `obs_stats=True` it also sums the observations the policies acted on, for a running
standardisation (`ObsSums`; include/pds.h pds_evaluate_policies_stats).  With `record=R` the launch also writes the flights
themselves out -- state, action and observation of every step of the first R episodes per policy -- as a `Flights`
(include/pds.h pds_evaluate_policies_record).  A population of actors with three or four hidden layers flies in one launch as well
(include/pds_evaluate_deep.h pds_evaluate_policies_deep: the plain and the metrics call; with deep_forms_fused=True the stats and
the record call of include/pds_evaluate_deep_forms.h too), every other form on the composed path."""
import ctypes as C
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import native
from .native import _ptr


def _write_episode_csvs(log_dir, ret, cost):
    """returns.csv and, where `cost` is given, costs.csv in `log_dir`: one value per line"""
    os.makedirs(log_dir, exist_ok=True)
    for name, values in (("returns.csv", ret), ("costs.csv", cost)):
        if values is not None:
            with open(os.path.join(log_dir, name), "w") as f:
                f.write("\n".join(str(float(x)) for x in values) + "\n")


def _as_policy(policy):
    if hasattr(policy, "step") and hasattr(policy, "pi"):  # ActorCritic: deterministic in eval mode
        return lambda obs: policy.step(obs)[0]
    return policy


@torch.no_grad()
def evaluate(env, policy, log_dir=None, log_costs=True):
    """-> (returns [N], ep_lengths [N], costs [N]) float32 CPU tensors, one episode per env.
    `policy`: ActorCritic (evaluated with exploration noise off), JsonPolicy or any obs -> action
    callable on device tensors."""
    was_training = getattr(policy, "training", False)
    if hasattr(policy, "eval"):
        policy.eval()  # disable exploration noise (evaluation.py:63)
    act = _as_policy(policy)
    n, dev = env.num_envs, env.device
    ret = torch.zeros(n, device=dev); cost = torch.zeros(n, device=dev); length = torch.zeros(n, device=dev)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    obs, _ = env.reset()
    for _ in range(env._max_episode_steps):
        obs, r, term, trunc, info = env.step(act(obs).contiguous())
        ret += torch.where(alive, r, torch.zeros_like(r))
        cost += torch.where(alive, info["cost"], torch.zeros_like(r))
        length += alive.float()
        alive &= ~(term | trunc)
    if hasattr(policy, "train") and was_training:
        policy.train()  # back to train mode (evaluation.py:91)
    ret, length, cost = ret.cpu(), length.cpu(), cost.cpu()
    if log_dir is not None:
        _write_episode_csvs(log_dir, ret, cost if log_costs else None)
    return ret, length, cost


@torch.no_grad()
def get_batch(env, policy, steps):
    """TrajectoryGenerator.get_batch (utils/trajectory_generator.py:84-118) for the whole batch:
    X[t] = the observation the policy acted on (standardised when `policy` carries scaling
    parameters, as `obs_rms(x)` there), Y[t] = the observation the step returned -- for an env that
    finished at t that is its terminal observation (`final_obs`), and X[t+1] its reset observation,
    exactly as the reference resets after appending y.  Returns (X, Y) of shape [steps, N, D]."""
    if hasattr(policy, "eval"):
        policy.eval()
    act = _as_policy(policy)
    n, d, dev = env.num_envs, env.obs_dim, env.device
    X = torch.empty(steps, n, d, device=dev); Y = torch.empty(steps, n, d, device=dev)
    mean, std, eps = getattr(policy, "mean", None), getattr(policy, "std", None), getattr(policy, "eps", 0.0)
    obs, _ = env.reset()
    for t in range(steps):
        X[t] = (obs - mean) / (std + eps) if mean is not None else obs
        obs, r, term, trunc, info = env.step(act(obs).contiguous())
        done = (term | trunc).unsqueeze(-1)
        Y[t] = torch.where(done, info["final_obs"], obs)
    return X, Y


# ---- a population of policies in one launch ----------------------------------------------------------------------------
_ACT_MODULE = {"relu": nn.ReLU, "tanh": nn.Tanh}
POPULATION_DEPTHS = (2, 3, 4)  # hidden layers of a population's actors: struct pds_mlp, or struct pds_mlp_deep at 3 and 4
POPULATION_MAX_WIDTH = 64      # ... and the widest hidden layer pds_mlp_deep stages


def _actor_shape(net):
    """(d_in, hidden sizes, d_out, activation name) of an nn.Sequential(Linear, act, ..., Linear[, Identity]) with two, three or
    four hidden layers and one activation type."""
    lin = [l for l in net if isinstance(l, nn.Linear)]
    acts = [l for l in net if not isinstance(l, (nn.Linear, nn.Identity))]
    if len(lin) - 1 not in POPULATION_DEPTHS or len(acts) != len(lin) - 1 or any(type(a) is not type(acts[0]) for a in acts[1:]):
        raise ValueError("a population holds actors with two, three or four hidden layers and one activation")
    name = {nn.ReLU: "relu", nn.Tanh: "tanh"}.get(type(acts[0]))
    if name is None:
        raise ValueError(f"activation {type(acts[0]).__name__}: relu or tanh")
    return lin[0].in_features, tuple(l.out_features for l in lin[:-1]), lin[-1].out_features, name


def _flat_params(net):
    """W1, b1, ..., W(L+1), b(L+1) in torch parameter order: the layout of pds_mlp_param_count / pds_mlp_deep_param_count."""
    lin = [l for l in net if isinstance(l, nn.Linear)]
    return torch.cat([t.detach().reshape(-1).float().cpu() for l in lin for t in (l.weight, l.bias)])


class PolicyPopulation:
    """P actors of ONE shape as data: `theta` [P, param_count] float32 (row p = W1, b1, W2, b2, W3, b3 of policy p in torch
    order), the shape (d_in, hidden_sizes, d_out = 4), the activation, optional observation standardisation `mean`, `std`
    [P, D] (both or none) and its eps.  Mixed shapes or activations raise ValueError: group by shape, one population each.
    hidden_sizes holds two, three or four widths.  At three and four (`deep`) a row is W1, b1, ..., W(L+1), b(L+1) in torch order
    (pds_mlp_deep_param_count's layout), every width is at most 64 and `mlp(p)` is a struct pds_mlp_deep."""

    def __init__(self, theta, d_in, hidden_sizes, activation, mean=None, std=None, eps=1e-5, d_out=4):
        hidden_sizes = tuple(int(h) for h in hidden_sizes)
        if len(hidden_sizes) not in POPULATION_DEPTHS:
            raise ValueError(f"two, three or four hidden layers, not {len(hidden_sizes)}")
        if len(hidden_sizes) > 2 and not all(1 <= h <= POPULATION_MAX_WIDTH for h in hidden_sizes):
            raise ValueError(f"hidden sizes {hidden_sizes}: with {len(hidden_sizes)} hidden layers every width is 1 .. {POPULATION_MAX_WIDTH}")
        if activation not in native.ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: relu or tanh")
        self.d_in, self.hidden_sizes, self.d_out, self.activation = int(d_in), hidden_sizes, int(d_out), activation
        if self.deep:
            sizes = (self.d_in,) + hidden_sizes + (self.d_out,)
            self.param_count = sum(sizes[j + 1] * sizes[j] + sizes[j + 1] for j in range(len(sizes) - 1))
        else:
            h1, h2 = hidden_sizes
            self.param_count = h1 * self.d_in + h1 + h2 * h1 + h2 + self.d_out * h2 + self.d_out
        theta = torch.as_tensor(theta, dtype=torch.float32)
        if theta.dim() == 1:
            theta = theta.unsqueeze(0)
        if theta.dim() != 2 or theta.shape[1] != self.param_count:
            raise ValueError(f"theta must be [P, {self.param_count}] for this shape, got {tuple(theta.shape)}")
        self.theta = theta.contiguous()
        if (mean is None) != (std is None):
            raise ValueError("mean and std come together")
        self.mean = self.std = None
        if mean is not None:
            mean, std = torch.as_tensor(mean, dtype=torch.float32), torch.as_tensor(std, dtype=torch.float32)
            want = (self.P, self.d_in)
            if mean.dim() == 1:  # one standardisation for every policy
                mean, std = mean.expand(*want), std.expand(*want)
            if tuple(mean.shape) != want or tuple(std.shape) != want:
                raise ValueError(f"mean and std must be {list(want)}")
            self.mean, self.std = mean.contiguous(), std.contiguous()
        self.eps = float(eps)

    @property
    def P(self):
        return int(self.theta.shape[0])

    def __len__(self):
        return self.P

    @property
    def deep(self):
        """three or four hidden layers: struct pds_mlp_deep and its entry points"""
        return len(self.hidden_sizes) > 2

    @classmethod
    def _from_nets(cls, nets, means, stds, epss):
        if len(nets) == 0:
            raise ValueError("an empty population")
        shapes = [_actor_shape(n) for n in nets]
        if any(s != shapes[0] for s in shapes[1:]):
            raise ValueError(f"mixed actor shapes or activations in one population: {sorted(set(shapes))}")
        with_stats = [m is not None for m in means]
        if any(w != with_stats[0] for w in with_stats[1:]):
            raise ValueError("policies with and without observation standardisation in one population")
        if with_stats[0] and any(e != epss[0] for e in epss[1:]):
            raise ValueError(f"mixed standardisation eps in one population: {sorted(set(epss))}")
        d_in, hidden, d_out, act = shapes[0]
        theta = torch.stack([_flat_params(n) for n in nets])
        mean = torch.stack([m.detach().float().cpu() for m in means]) if with_stats[0] else None
        std = torch.stack([s.detach().float().cpu() for s in stds]) if with_stats[0] else None
        return cls(theta, d_in, hidden, act, mean, std, epss[0] if with_stats[0] else 1e-5, d_out=d_out)

    @classmethod
    def from_actor_critics(cls, acs):
        """ActorCritic list (ppo.py): the actors `pi.net`, standardisation from `obs_oms`."""
        acs = list(acs)
        oms = [getattr(ac, "obs_oms", None) for ac in acs]
        return cls._from_nets([ac.pi.net for ac in acs], [o.mean if o is not None else None for o in oms],
                              [o.std if o is not None else None for o in oms], [o.eps if o is not None else None for o in oms])

    @classmethod
    def from_json_policies(cls, policies):
        """policy_io.JsonPolicy list: `net`, `mean`, `std`, `eps`."""
        ps = list(policies)
        return cls._from_nets([p.net for p in ps], [p.mean for p in ps], [p.std for p in ps], [p.eps for p in ps])

    @classmethod
    def from_flat(cls, theta, d_in, hidden_sizes, activation, mean=None, std=None, eps=1e-5):
        """theta [P, param_count] as an evolution strategy holds it."""
        return cls(theta, d_in, hidden_sizes, activation, mean, std, eps)

    def to(self, device):
        """A population whose tensors live on `device`; this one stays where it is."""
        has = self.mean is not None
        return PolicyPopulation(self.theta.to(device), self.d_in, self.hidden_sizes, self.activation,
                                self.mean.to(device) if has else None, self.std.to(device) if has else None, self.eps, d_out=self.d_out)

    def policy(self, p):
        """The p-th actor as nn.Sequential(Linear, act, ..., Linear, Identity) on the CPU (no standardisation)."""
        sizes = [self.d_in, *self.hidden_sizes, self.d_out]
        last = len(sizes) - 2
        row, off, layers = self.theta[p].detach().cpu(), 0, []
        for j in range(last + 1):
            lin = nn.Linear(sizes[j], sizes[j + 1])
            nw, nb = sizes[j + 1] * sizes[j], sizes[j + 1]
            lin.weight.data = row[off:off + nw].reshape(sizes[j + 1], sizes[j]).clone()
            lin.bias.data = row[off + nw:off + nw + nb].clone()
            off += nw + nb
            layers += [lin, _ACT_MODULE[self.activation]() if j < last else nn.Identity()]
        return nn.Sequential(*layers)

    def mlp(self, p=0):
        """struct pds_mlp of policy p -- struct pds_mlp_deep with three or four hidden layers --: pointers into row p of theta."""
        base = self.theta.data_ptr() + 4 * p * self.param_count
        if self.deep:
            return native.mlp_deep(self.d_in, self.hidden_sizes, self.d_out, self.activation, base=base)
        return native.mlp(self.d_in, *self.hidden_sizes, self.d_out, self.activation, base=base)


def _check_population_call(env, population):
    P, n = population.P, int(env.num_envs)
    if n % P != 0:
        raise ValueError(f"env.num_envs = {n} is not P x E for the population's P = {P}")
    E = n // P
    if E % 64 != 0:
        raise ValueError(f"episodes per policy E = {n} / {P} = {E} is not a multiple of 64 (one tile)")
    return P, E


def fused_evaluation_built(env):
    """Whether pds_evaluate_policies has a kernel for this env: a handle with auto_reset whose configuration is one the fused
    rollout is built for, and observation_history_size == 2."""
    return getattr(env, "observation_history_size", 2) == 2 and bool(env.lib.pds_evaluate_supported(env._handle))


def fused_deep_evaluation_built(env, population):
    """Whether pds_evaluate_policies_deep (include/pds_evaluate_deep.h) has a kernel for this env and this population of actors
    with three or four hidden layers: a handle with auto_reset, observation_history_size == 2, control_mode PWM without latency
    ring or Kalman hold (every noise setting; motor dynamics on Hover and Circle, the ground effect on TakeOff), the actors
    reading the env's observation.  False for a population with two hidden layers: that is fused_evaluation_built's question."""
    if not getattr(population, "deep", False) or getattr(env, "observation_history_size", 2) != 2:
        return False
    return env.lib.pds_evaluate_deep_supported(env._handle, C.byref(population.mlp(0))) == 1


def fused_deep_forms_evaluation_built(env, population, form):
    """Whether the stats (`form` "stats": pds_evaluate_policies_deep_stats) or the record form ("record":
    pds_evaluate_policies_deep_record; include/pds_evaluate_deep_forms.h) of the deep evaluation has a kernel for this env and this
    population: what fused_deep_evaluation_built asks, and the form's code object of the env's variant being one the library
    launches.  False for a population with two hidden layers."""
    if form not in ("stats", "record"):
        raise ValueError("form: 'stats' or 'record'")
    if not getattr(population, "deep", False) or getattr(env, "observation_history_size", 2) != 2:
        return False
    code = native.EVALUATE_DEEP_FORM_STATS if form == "stats" else native.EVALUATE_DEEP_FORM_RECORD
    return env.lib.pds_evaluate_deep_forms_supported(env._handle, C.byref(population.mlp(0)), code) == 1


def fused_history_evaluation_built(env):
    """Whether pds_evaluate_policies_history has a kernel for this env and its observation_history_size H: a handle with auto_reset
    whose configuration is one the history rollout is built for, and H x half <= 192 network inputs."""
    return env.lib.pds_evaluate_history_supported(env._handle, int(getattr(env, "observation_history_size", 2))) == 1


def fused_history_stats_evaluation_built(env):
    """Whether pds_evaluate_policies_history_stats has a kernel for this env and its observation_history_size H: what
    fused_history_evaluation_built asks, and that the stats form of the kernel is built for the input width of H x half."""
    return env.lib.pds_evaluate_history_stats_supported(env._handle, int(getattr(env, "observation_history_size", 2))) == 1


def _history_latency_env(env):
    """An env created with history_latency=True whose views are not frozen (set_latency since the last full reset): the one the
    latency forms of the history evaluation may fly, as fused.rollout_history_latency_supported says for the rollout."""
    return bool(getattr(env, "history_latency", False)) and not getattr(env, "_hist_frozen", False)


def fused_history_latency_evaluation_built(env):
    """Whether pds_evaluate_policies_history_latency (include/pds_history_latency_evaluate.h) has a kernel for this env and its
    observation_history_size H: an env created with history_latency=True on the latency ring, Hover or Circle in any control mode,
    noise off or the reference's default, H x half <= 192 -- and no set_latency since the last full reset (frozen views)."""
    if not _history_latency_env(env):
        return False
    return env.lib.pds_evaluate_history_latency_supported(env._handle, int(env.observation_history_size)) == 1


def fused_history_latency_stats_evaluation_built(env):
    """Whether pds_evaluate_policies_history_latency_stats has a kernel for this env and its observation_history_size H: what
    fused_history_latency_evaluation_built asks, and that the stats form of the kernel is built for the input width of H x half."""
    if not _history_latency_env(env):
        return False
    return env.lib.pds_evaluate_history_latency_stats_supported(env._handle, int(env.observation_history_size)) == 1


# ---- flight-quality metrics (include/pds.h PDS_EM_*) -------------------------------------------------------------------
METRIC_NAMES = ("roll_sq", "pitch_sq", "rate_sq", "action_rate_sq", "tilt_max", "saturated_steps", "roll_rate_crossings",
                "pitch_rate_crossings")  # column j of `raw` = PDS_EM_* value j


class FlightMetrics:
    """The eight raw per-episode values of pds_evaluate_policies_metrics: `raw` [P, E, 8] float32 on the CPU (columns:
    METRIC_NAMES; sums over the states x(0) .. x(L - 1) the policy acted in, x(s) the true state before step s), `length` [P, E]
    the episode lengths L, `step_seconds` the simulated time of one env step (time_step x aggregate_phy_steps).  Every column
    is also an attribute, a [P, E] view: `fm.roll_sq`, `fm.tilt_max`, ...  `table()` derives what 02_eval_hover_task.py prints."""

    def __init__(self, raw, length, step_seconds):
        self.raw = torch.as_tensor(raw, dtype=torch.float32)
        self.length = torch.as_tensor(length, dtype=torch.float32)
        self.step_seconds = float(step_seconds)
        if self.raw.dim() != 3 or self.raw.shape[2] != len(METRIC_NAMES) or tuple(self.raw.shape[:2]) != tuple(self.length.shape):
            raise ValueError(f"raw must be [P, E, {len(METRIC_NAMES)}] and length [P, E]")

    def __getattr__(self, name):
        if name in METRIC_NAMES:
            return self.raw[..., METRIC_NAMES.index(name)]
        raise AttributeError(name)

    def per_episode(self):
        """The derived quantities per episode, each [P, E] float64, in the units of 02_eval_hover_task.py: flight_time [s],
        mse_roll_deg2 / mse_pitch_deg2 [deg^2] (the mean over the episode's steps), freq_roll_rate_hz / freq_pitch_rate_hz
        (two sign changes of the rate are one oscillation), action_rate (mean squared change of the action per step),
        saturated_share (of the steps), tilt_max_deg."""
        raw, L = self.raw.double(), self.length.double()
        deg2 = (180.0 / math.pi) ** 2
        t = L * self.step_seconds
        col = lambda name: raw[..., METRIC_NAMES.index(name)]
        return dict(flight_time=t, mse_roll_deg2=col("roll_sq") / L * deg2, mse_pitch_deg2=col("pitch_sq") / L * deg2,
                    freq_roll_rate_hz=col("roll_rate_crossings") / (2.0 * t), freq_pitch_rate_hz=col("pitch_rate_crossings") / (2.0 * t),
                    action_rate=col("action_rate_sq") / L, saturated_share=col("saturated_steps") / L,
                    tilt_max_deg=col("tilt_max") * (180.0 / math.pi))

    def table(self):
        """-> {name: [P] float64}: per policy the mean over its E episodes of every quantity of per_episode()."""
        return {k: v.mean(dim=1) for k, v in self.per_episode().items()}


def metrics_from_arrays(rpy, omega, actions, last_action0):
    """The eight raw values (METRIC_NAMES order, float64 numpy) of ONE flight from its log: rpy [L, 3] and omega [L, 3] the
    attitude [rad] and body rates at the L instants a command was issued, actions [L, 4] the commands in the policy's units (1 =
    full scale), last_action0 [4] the command in force before the first.  Straight from the definitions (include/pds.h), so a real
    flight and a simulated one are scored alike."""
    rpy, omega = np.asarray(rpy, dtype=np.float64).reshape(-1, 3), np.asarray(omega, dtype=np.float64).reshape(-1, 3)
    actions, u = np.asarray(actions, dtype=np.float64).reshape(-1, 4), np.asarray(last_action0, dtype=np.float64).reshape(4)
    L = rpy.shape[0]
    if L < 1 or omega.shape[0] != L or actions.shape[0] != L:
        raise ValueError("rpy, omega and actions hold one row per step, at least one")
    out = np.zeros(len(METRIC_NAMES))
    out[0] = np.sum(rpy[:, 0] ** 2)
    out[1] = np.sum(rpy[:, 1] ** 2)
    out[2] = np.sum(omega ** 2)
    before = np.vstack([u[None, :], actions[:-1]])  # the command in force when step s was issued
    out[3] = np.sum((actions - before) ** 2)
    for v in np.fmax(np.abs(rpy[:, 0]), np.abs(rpy[:, 1])):  # (fmax and `>`: a NaN angle is passed over)
        if v > out[4]:
            out[4] = v
    out[5] = np.count_nonzero((np.abs(actions) > 1.0).any(axis=1))
    for j, k in ((0, 6), (1, 7)):
        neg = omega[:, j] < 0.0
        out[k] = np.count_nonzero(neg[1:] != neg[:-1])
    return out


def _compose_metrics(acc, prev_neg, alive, rpy, omega, act, last):
    """One step of the PDS_EM_* sums as separate elementwise float32 ops (what the kernel does with one instruction each), for the
    envs still `alive`.  acc [8][N]; -> the signs of (wx, wy) for the next step."""
    zero, one = torch.zeros_like(acc[0]), torch.ones_like(acc[0])
    roll, pitch = rpy[:, 0], rpy[:, 1]
    wx, wy, wz = omega[:, 0], omega[:, 1], omega[:, 2]
    acc[0] += torch.where(alive, roll * roll, zero)
    acc[1] += torch.where(alive, pitch * pitch, zero)
    acc[2] += torch.where(alive, (wx * wx + wy * wy) + wz * wz, zero)
    d = act - last
    dd = d * d
    acc[3] += torch.where(alive, ((dd[:, 0] + dd[:, 1]) + dd[:, 2]) + dd[:, 3], zero)
    for v in (roll.abs(), pitch.abs()):
        acc[4].copy_(torch.where(alive & (v > acc[4]), v, acc[4]))
    acc[5] += torch.where(alive & (act.abs() > 1.0).any(dim=1), one, zero)
    neg = omega[:, :2] < 0
    if prev_neg is not None:
        crossed = (neg != prev_neg) & alive.unsqueeze(1)
        acc[6] += torch.where(crossed[:, 0], one, zero)
        acc[7] += torch.where(crossed[:, 1], one, zero)
    return neg


# ---- observation sums (include/pds.h pds_evaluate_policies_stats) ------------------------------------------------------
SLAB_WAVES, SLAB_FEATURES, SLAB_ROWS = 4, 64, 16  # d_obs_sums [tiles, 4, 2, 64]; a network wave sums 16 rows of its tile
SLAB_WIDTHS = (64, 96, 128, 192)  # ... and [tiles, 4, 2, W] for the histories (include/pds_history_stats.h): W = slab_features(H x half)
_OBS_STATS_LOG = None  # a list: the composed path appends (d [N, D] float64, alive [N] bool), on the CPU, per step (the tests' float64 sums)


def slab_features(d_in):
    """The columns W of the slab for `d_in` network inputs: 16 x rollout_hist_tiles(d_in) of csrc/pds_types.h -- 64, 96, 128 or 192,
    the smallest that holds d_in (SLAB_FEATURES up to 64 inputs)."""
    d_in = int(d_in)
    if d_in < 1 or d_in > SLAB_WIDTHS[-1]:
        raise ValueError(f"{d_in} network inputs: a slab holds 1 .. {SLAB_WIDTHS[-1]} features")
    return next(w for w in SLAB_WIDTHS if d_in <= w)


def tree_reduce_rows(acc):
    """[N, D] per-env float32 sums -> [N / 64, 4, D]: the 16 envs of every quarter tile added in the kernel's fixed tree -- env j
    + env j + 8, then j + (j + 4), then + 2, then + 1 -- with one float32 add per level (slice adds, never torch.sum, whose order
    is its own)."""
    n, d = acc.shape
    if n % 64 != 0:
        raise ValueError(f"{n} envs are not whole tiles of 64")
    x = acc.reshape(n // 64, SLAB_WAVES, SLAB_ROWS, d)
    for h in (8, 4, 2, 1):
        x = x[:, :, :h] + x[:, :, h:2 * h]
    return x[:, :, 0]


def _compose_slab(s1, s2):
    """the per-env sums [N, D] of the composed path -> the kernel's slab [tiles, 4, 2, W], W = slab_features(D) (features >= D zero)"""
    n, d = s1.shape
    slab = torch.zeros(n // 64, SLAB_WAVES, 2, slab_features(d), device=s1.device)
    slab[:, :, 0, :d] = tree_reduce_rows(s1)
    slab[:, :, 1, :d] = tree_reduce_rows(s2)
    return slab


class ObsSums:
    """What evaluate_population(..., obs_stats=True) sums over every observation o a first-episode policy acted on, per policy p
    and feature k: with d = o_k - shift[p][k], `sum_d` = sum d and `sum_d2` = sum d^2, each [P, D] float64 on the CPU -- the
    kernel's float32 partial sums (`slab` [tiles, 4, 2, W], raw; W = 64, or 96 / 128 / 192 for the wider histories: SLAB_WIDTHS, W >= D) added over the policy's tiles and the four waves of a tile in
    float64.  `count` [P] float64: the number of observations, length.sum(1).  `shift` [P, D] float64: the means that were
    subtracted (the population's own standardisation means; zeros without one).
    The float64 sums are taken where the slab lives (a population of a million envs writes 33 MB of partial sums: summed on
    the device, [P, D] comes to the host); `slab` brings the raw float32 array to the CPU when it is first asked for."""

    def __init__(self, slab, count, shift):
        self._slab = torch.as_tensor(slab, dtype=torch.float32)
        self._slab_cpu = None
        self.count = torch.as_tensor(count, dtype=torch.float64).reshape(-1)
        self.shift = torch.as_tensor(shift, dtype=torch.float64)
        P, D = self.shift.shape
        W = int(self._slab.shape[3]) if self._slab.dim() == 4 else 0
        if (self._slab.dim() != 4 or tuple(self._slab.shape[1:3]) != (SLAB_WAVES, 2) or W not in SLAB_WIDTHS or self._slab.shape[0] % P != 0 or D > W):
            raise ValueError(f"slab must be [tiles, {SLAB_WAVES}, 2, W] with W one of {SLAB_WIDTHS}, at least D = {D}, and tiles a multiple of P = {P}")
        if self.count.numel() != P:
            raise ValueError(f"count must hold {P} values")
        per = self._slab.reshape(P, -1, 2, W).sum(dim=1, dtype=torch.float64).cpu()
        self.sum_d, self.sum_d2 = per[:, 0, :D].contiguous(), per[:, 1, :D].contiguous()

    @property
    def slab(self):
        if self._slab_cpu is None:
            self._slab_cpu = self._slab.cpu()
        return self._slab_cpu

    @staticmethod
    def _moments(n, shift, sd, sd2):
        n_ = n.unsqueeze(-1) if sd.dim() == 2 else n
        safe = torch.where(n_ > 0, n_, torch.ones_like(n_))
        mean = shift + sd / safe
        m2 = torch.clamp(sd2 - sd * sd / safe, min=0.0)  # (sum (x - mean)^2 >= 0: the rounding of the float32 sums may say otherwise)
        return n, mean, m2

    def moments(self):
        """-> (count [P], mean [P, D], M2 [P, D]) float64 per policy: mean = shift + sum_d / count, M2 = sum (o - mean)^2 =
        sum_d2 - sum_d^2 / count.  A policy without observations (count 0) gets mean = shift and M2 = 0."""
        return self._moments(self.count, self.shift, self.sum_d, self.sum_d2)

    def pooled(self):
        """-> (count, mean [D], M2 [D]) float64 over all policies.  Their sums add up as they are where all policies share one
        shift; otherwise every policy's sums are first re-centred to the shift c of policy 0 in float64: with e = shift_p - c,
        sum (d + e) = sum_d + n e and sum (d + e)^2 = sum_d2 + 2 e sum_d + n e^2."""
        c = self.shift[0]
        e = self.shift - c
        n = self.count.unsqueeze(-1)
        sd = (self.sum_d + n * e).sum(dim=0)
        sd2 = (self.sum_d2 + 2.0 * e * self.sum_d + n * e * e).sum(dim=0)
        return self._moments(self.count.sum(), c, sd, sd2)


# ---- the recorded flights (include/pds.h pds_evaluate_policies_record) ----------------------------------------------------------
class Flights:
    """What evaluate_population(..., record=R) records of the first R episodes of each of P policies, float32 on the CPU:
    `state` [P, R, T, 12] the true state x(s) the policy acted in, in the column order of a flight log (simopt.OBS_COLUMNS: x y z,
    x_dot y_dot z_dot, roll pitch yaw, roll_dot pitch_dot yaw_dot), `action` [P, R, T, 4] the raw action a(s) handed to step s,
    `observation` [P, R, T, D] the raw (unstandardised) observation o(s) the policy acted on, or None, `length` [P, R] the
    episode lengths L and `step_seconds` the simulated time of one env step.  Rows s >= L are zero.  The terminal state x(L) and
    the terminal observation are not part of the record.  `last_action0` [P, R, 4]: the command in force before the first step
    (the env's last_action after its reset), `control_mode` the env's."""

    def __init__(self, state, action, observation, length, step_seconds, last_action0=None, control_mode="PWM"):
        self.state = torch.as_tensor(state, dtype=torch.float32)
        self.action = torch.as_tensor(action, dtype=torch.float32)
        self.observation = None if observation is None else torch.as_tensor(observation, dtype=torch.float32)
        self.length = torch.as_tensor(length, dtype=torch.float32)
        self.step_seconds = float(step_seconds)
        self.control_mode = control_mode
        if self.state.dim() != 4 or self.state.shape[3] != 12:
            raise ValueError(f"state must be [P, R, T, 12], got {tuple(self.state.shape)}")
        P, R, T = self.state.shape[:3]
        if tuple(self.action.shape) != (P, R, T, 4) or tuple(self.length.shape) != (P, R):
            raise ValueError(f"action must be [{P}, {R}, {T}, 4] and length [{P}, {R}]")
        if self.observation is not None and (self.observation.dim() != 4 or tuple(self.observation.shape[:3]) != (P, R, T)):
            raise ValueError(f"observation must be [{P}, {R}, {T}, D]")
        if bool((self.length < 0).any()) or bool((self.length > T).any()):
            raise ValueError(f"lengths outside 0 .. {T}")
        self.last_action0 = torch.zeros(P, R, 4) if last_action0 is None else torch.as_tensor(last_action0, dtype=torch.float32).reshape(P, R, 4)

    @property
    def P(self):
        return int(self.state.shape[0])

    @property
    def R(self):
        return int(self.state.shape[1])

    def episode(self, p, e):
        """-> dict(state [L, 12], action [L, 4], observation [L, D] or None): episode e of policy p, cut to its length L."""
        L = int(self.length[p, e])
        return dict(state=self.state[p, e, :L], action=self.action[p, e, :L],
                    observation=None if self.observation is None else self.observation[p, e, :L])

    def metrics(self):
        """-> [P, R, 8] float64 numpy: metrics_from_arrays of every recorded episode (METRIC_NAMES order) -- the definitions in
        float64 over the recorded float32 states, next to the float32 sums of the launch (FlightMetrics.raw)."""
        out = np.zeros((self.P, self.R, len(METRIC_NAMES)))
        for p in range(self.P):
            for e in range(self.R):
                ep = self.episode(p, e)
                x = ep["state"].numpy()
                out[p, e] = metrics_from_arrays(x[:, 6:9], x[:, 9:12], ep["action"].numpy(), self.last_action0[p, e].numpy())
        return out

    def pairs(self):
        """-> (X, Y), each [sum over the episodes of (L - 1), D] float32: X = o(s), Y = o(s + 1) for s + 1 < L within an episode,
        the episodes in order (policy, then episode).  These are get_batch's pairs WITHOUT the terminal row of each episode -- the
        pair (o(L - 1), terminal observation) is not there, the terminal observation not being recorded -- and unstandardised."""
        if self.observation is None:
            raise ValueError("recorded without observations (record_observations=False)")
        xs, ys = [], []
        for p in range(self.P):
            for e in range(self.R):
                o = self.episode(p, e)["observation"]
                xs.append(o[:-1]); ys.append(o[1:])
        return torch.cat(xs), torch.cat(ys)

    def _logs(self):
        """per recorded episode ((p, e), the 12 log columns [L, 12] float64, the PWMs [L, 4] a fully charged battery takes)"""
        if self.control_mode != "PWM":
            raise ValueError(f"control mode {self.control_mode}: the actions are motor PWMs under control_mode PWM only")
        for p in range(self.P):
            for e in range(self.R):
                ep = self.episode(p, e)
                yield (p, e), ep["state"].double().numpy(), (np.clip(ep["action"].double().numpy(), -1.0, 1.0) + 1.0) * 30000.0

    def to_csv_dir(self, path, voltage=3.9):
        """One CSV per recorded episode, `path`/policy_<p>_episode_<e>.csv, in the layout MiniTrajectories.from_csv_dir reads:
        simopt.OBS_COLUMNS, simopt.PWM_COLUMNS and `bat`.  PWM = (clip(a, -1, 1) + 1) * 30000 is what the motors took; the file
        holds the PWM that gives the same thrust at the constant battery `voltage` (the battery model of the logs inverted, as
        examples/run_simulation_optimization.py synthetic_logs does), so that from_csv_dir recovers the actions.  control_mode PWM
        only: ValueError otherwise.  -> the list of files."""
        from . import simopt
        mt = simopt.MiniTrajectories
        logs = list(self._logs())
        os.makedirs(path, exist_ok=True)
        files = []
        for (p, e), log, pwm in logs:
            grams = pwm / 65535 * 60
            raw = (mt.BATTERY_QUAD * grams ** 2 + mt.BATTERY_LIN * grams) / voltage * 65535
            name = os.path.join(path, f"policy_{p:04d}_episode_{e:05d}.csv")
            with open(name, "w") as f:
                f.write(",".join(simopt.OBS_COLUMNS + simopt.PWM_COLUMNS + ["bat"]) + "\n")
                for s in range(log.shape[0]):
                    f.write(",".join(repr(float(v)) for v in list(log[s]) + list(raw[s]) + [voltage]) + "\n")
            files.append(name)
        return files

    def mini_trajectories(self, T=35, pre_steps=5, skip=10):
        """-> simopt.MiniTrajectories: create_trajectory_slices of every recorded episode that is long enough for one slice
        (L > T + pre_steps), concatenated in order; the actions are the clipped ones the motors took.  control_mode PWM only."""
        from . import simopt
        parts = [simopt.MiniTrajectories.create_trajectory_slices(log, pwm, T, pre_steps, skip)
                 for _, log, pwm in self._logs() if log.shape[0] > T + pre_steps]
        if not parts:
            raise ValueError(f"no recorded episode is longer than T + pre_steps = {T + pre_steps} steps")
        return simopt.MiniTrajectories(*[np.concatenate([part[k] for part in parts]) for k in range(3)])


def _plan_population_call(env, population, fused, max_steps, metrics, obs_stats, history_fused, record, record_limit_bytes,
                          history_stats_fused=False):
    """The argument checks of evaluate_population and its choice of path, with the env untouched -> (P, E, T, R or None, the
    form "plain" / "metrics" / "stats" / "record", whether the kernel path flies, and H where that is the history kernel, else None)"""
    return _plan_population(env, population, fused, max_steps, metrics, obs_stats, history_fused, record, record_limit_bytes,
                            history_stats_fused)


def _plan_population(env, population, fused, max_steps, metrics, obs_stats, history_fused, record, record_limit_bytes,
                     history_stats_fused=False, history_latency_fused=False, deep_forms_fused=False):
    """_plan_population_call (which is this plan with history_latency_fused at its default), and with history_latency_fused=True:
    the latency forms of the history kernel count as built where their predicates hold -- an env on the ring, for which the other
    predicates answer False; evaluate_population tells `_fly_kernel` which by the same predicate.  deep_forms_fused=True: the stats
    and the record form of a deep population count as built where fused_deep_forms_evaluation_built holds."""
    P, E = _check_population_call(env, population)
    if population.d_in != env.obs_dim:
        raise ValueError(f"the population's actors read {population.d_in} inputs, the env observes {env.obs_dim}")
    if isinstance(fused, str):
        if fused != "auto":
            raise ValueError("fused: True, False or 'auto'")
    else:
        fused = bool(fused)  # (1, 0, numpy.bool_: below `fused is True` must mean what it says)
    if not isinstance(history_fused, (bool, np.bool_)):
        raise ValueError("history_fused: True or False")
    if not isinstance(history_stats_fused, (bool, np.bool_)):
        raise ValueError("history_stats_fused: True or False")
    if not isinstance(history_latency_fused, (bool, np.bool_)):
        raise ValueError("history_latency_fused: True or False")
    if not isinstance(deep_forms_fused, (bool, np.bool_)):
        raise ValueError("deep_forms_fused: True or False")
    T = int(env._max_episode_steps if max_steps is None else max_steps)
    if T < 1:
        raise ValueError(f"max_steps = {T}")
    R = None
    if record is not None:  # (what pds_evaluate_policies_record refuses, before the library is asked anything)
        if isinstance(record, (bool, np.bool_)) or int(record) != record:
            raise ValueError(f"record = {record!r}: a number of episodes per policy")
        R = int(record)
        if R < 64 or R % 64 != 0 or R > E:
            raise ValueError(f"record = {R} is not a positive multiple of 64 (one tile) up to E = {E}")
        if obs_stats:
            raise ValueError("record and obs_stats do not come together: no kernel form gathers both")
        need = T * P * R * (64 + 4 * int(env.obs_dim))
        if need > int(record_limit_bytes):
            raise ValueError(f"the record of {T} steps x {P} x {R} episodes takes {need} bytes, above record_limit_bytes = "
                             f"{int(record_limit_bytes)}: record fewer episodes or fewer steps, or raise the limit")
    form = "record" if R is not None else "stats" if obs_stats else "metrics" if metrics else "plain"
    H = int(getattr(env, "observation_history_size", 2))
    if getattr(population, "deep", False):
        # three or four hidden layers: evaluate_deep_kernel's plain / metrics form, and where deep_forms_fused asks for them its
        # stats and record forms; the composed path flies every form on pds_mlp_deep_forward, whose inputs end at 64 -- no
        # observation history reaches it
        if H != 2:
            raise NotImplementedError(f"observation_history_size {H} with {len(population.hidden_sizes)} hidden layers: pds_mlp_deep_forward "
                                      "reads up to 64 inputs, on either path")
        use_kernel = False
        if fused is not False:
            if form in ("plain", "metrics"):
                built = fused_deep_evaluation_built(env, population)
            else:
                built = bool(deep_forms_fused) and fused_deep_forms_evaluation_built(env, population, form)
            if fused is True and not built:
                raise NotImplementedError("pds_evaluate_policies_deep has no kernel for this call (built: the plain and the metrics form -- "
                                          "obs_stats and record with deep_forms_fused=True only --, auto_reset, control_mode PWM without latency ring or Kalman hold; "
                                          "motor dynamics on Hover and Circle, the ground effect on TakeOff); fused='auto' runs the composed path")
            use_kernel = built
        return P, E, T, R, form, use_kernel, None
    # (the history kernel has a plain / metrics form, a record form and a stats form; the stats form flies where history_stats_fused asks for it)
    use_history = bool(history_fused) and H != 2
    use_kernel = False
    if fused is not False and use_history:
        if obs_stats:
            built = bool(history_stats_fused) and fused_history_stats_evaluation_built(env)
        else:
            built = fused_history_evaluation_built(env)
        if not built and history_latency_fused:  # (on the latency ring: the predicates above answer False there)
            if obs_stats:
                built = bool(history_stats_fused) and fused_history_latency_stats_evaluation_built(env)
            else:
                built = fused_history_latency_evaluation_built(env)
        if fused is True and not built:
            raise NotImplementedError("pds_evaluate_policies_history has no kernel for this call (built: auto_reset, the env configurations "
                                      "of the history rollout, H x half <= 192 inputs; obs_stats with history_stats_fused=True only, where "
                                      "pds_evaluate_history_stats_supported holds); fused='auto' runs the composed path")
        use_kernel = built
    elif fused is not False:
        built = fused_evaluation_built(env)
        if fused is True and not built:
            raise NotImplementedError("pds_evaluate_policies has no kernel for this env (built: observation_history_size 2, auto_reset, "
                                      "the env configurations of the fused rollout); fused='auto' runs the composed path")
        use_kernel = built
    return P, E, T, R, form, use_kernel, (H if use_history else None)


def _fly_kernel(env, population, obs, P, E, T, form, H, rec, latency=False):
    """One launch -> (ret, length, cost, raw, slab) on the device, raw / slab None where the form has none; the record is written
    into `rec`'s arrays.  Per form the entry point and what trails d_cost in its argument list; the history kernel leads with H
    and takes d_metrics or NULL, its record form (pds_evaluate_policies_history_record) what the record form takes, its stats form
    (pds_evaluate_policies_history_stats) what the stats form takes, the slab slab_features(H x half) columns wide.  latency=True:
    the three history entry points on the latency ring (include/pds_history_latency_evaluate.h), the same argument lists.
    A deep population: pds_evaluate_policies_deep (plain or metrics), which takes d_metrics or NULL, and for the stats and the
    record form pds_evaluate_policies_deep_stats / _deep_record (include/pds_evaluate_deep_forms.h), the same trailing arguments
    as at two hidden layers."""
    dev, n = env.device, env.num_envs
    ret = torch.zeros(n, device=dev); cost = torch.zeros(n, device=dev); length = torch.zeros(n, device=dev)
    raw = torch.zeros(n, len(METRIC_NAMES), device=dev) if form != "plain" else None
    slab = torch.zeros(n // 64, SLAB_WAVES, 2, slab_features(population.d_in) if H is not None else SLAB_FEATURES, device=dev) if form == "stats" else None
    _, R, flight, obs_rec = rec if rec is not None else (None,) * 4
    if population.deep:  # d_metrics or NULL in every form; the struct goes in by reference
        name, trail = {"stats": ("pds_evaluate_policies_deep_stats", (slab,)),
                       "record": ("pds_evaluate_policies_deep_record", (R, flight, obs_rec))}.get(form, ("pds_evaluate_policies_deep", ()))
        native.call(name, env._handle, P, E, C.byref(population.mlp(0)), population.theta, population.mean,
                    population.std, population.eps, T, obs, ret, length, cost, raw, *trail, on=dev, handle=env._handle)
        return ret, length, cost, raw, slab
    name, trail = {"plain": ("pds_evaluate_policies", ()),
                   "metrics": ("pds_evaluate_policies_metrics", (raw,)),
                   "stats": ("pds_evaluate_policies_stats", (raw, slab)),
                   "record": ("pds_evaluate_policies_record", (raw, R, flight, obs_rec))}[form]
    lead = ()
    if H is not None:  # ([N, H * half]: the histories env.reset() returns; the record and the stats form take what theirs take at H = 2)
        obs, lead = obs.contiguous(), (H,)
        name, trail = {"record": ("pds_evaluate_policies_history_record", trail),
                       "stats": ("pds_evaluate_policies_history_stats", trail)}.get(form, ("pds_evaluate_policies_history", (raw,)))
        if latency:
            name = name.replace("pds_evaluate_policies_history", "pds_evaluate_policies_history_latency")
    native.call(name, env._handle, *lead, P, E, population.mlp(0), population.theta, population.mean, population.std,
                population.eps, T, obs, ret, length, cost, *trail, on=dev, handle=env._handle)
    return ret, length, cost, raw, slab


def _fly_composed(env, population, obs, P, E, T, metrics, obs_stats, rec):
    """The same flight step by step -> _fly_kernel's tuple, the same bits: per step one pds_mlp_forward per policy on its block of
    the observation (pds_mlp_deep_forward for a population with three or four hidden layers), env.step and the accumulator updates
    of `evaluate`, every sum a torch op of its own."""
    dev, n, D = env.device, env.num_envs, env.obs_dim
    ret = torch.zeros(n, device=dev); cost = torch.zeros(n, device=dev); length = torch.zeros(n, device=dev)
    raw = slab = None
    mlps = [population.mlp(p) for p in range(P)]
    forward = "pds_mlp_forward"
    if population.deep:  # (three or four hidden layers: the same call on struct pds_mlp_deep, which goes in by reference)
        forward, mlps = "pds_mlp_deep_forward", [C.byref(m) for m in mlps]
    act = torch.empty(n, 4, device=dev)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    has = population.mean is not None
    acc = [torch.zeros(n, device=dev) for _ in METRIC_NAMES] if metrics else None
    prev_neg = None
    if obs_stats:  # per-env sums of d and d * d, d = o - mean of the env's policy
        s1, s2 = torch.zeros(n, D, device=dev), torch.zeros(n, D, device=dev)
        shift_rows = population.mean.repeat_interleave(E, dim=0) if has else None
        zero_nd = torch.zeros(n, D, device=dev)
    if rec is not None:
        rec_env, R, flight, obs_rec = rec
    for s in range(T):
        if metrics:  # x(s): the state the policy acts in
            rpy, omega, last = env.get_state("rpy"), env.get_state("omega"), env.get_state("last_action")
        for p in range(P):
            native.call(forward, mlps[p], _ptr(obs, 4 * p * E * D), None, E, _ptr(population.mean, 4 * p * D) if has else None,
                        _ptr(population.std, 4 * p * D) if has else None, population.eps, _ptr(act, 16 * p * E), on=dev)
        if metrics:
            prev_neg = _compose_metrics(acc, prev_neg, alive, rpy, omega, act, last)
        if rec is not None:  # x(s), a(s) and o(s) of the recorded envs alive in front of step s
            x = torch.cat([env.get_state(f) for f in ("pos", "vel", "rpy", "omega")] + [act], dim=1)[rec_env]  # [P R, 16]
            on = alive[rec_env].unsqueeze(1)
            flight[s] = torch.where(on, x, torch.zeros_like(x)).reshape(P * R, 4, 4).transpose(0, 1)
            if obs_rec is not None:
                o = obs[rec_env]
                obs_rec[s] = torch.where(on, o, torch.zeros_like(o))
        if obs_stats:  # o(s), for the envs alive in front of step s
            d = obs - shift_rows if has else obs
            on = alive.unsqueeze(1)
            s1 += torch.where(on, d, zero_nd)
            s2 += torch.where(on, d * d, zero_nd)
            if _OBS_STATS_LOG is not None:
                _OBS_STATS_LOG.append((d.double().cpu(), alive.cpu().clone()))
        obs, r, term, trunc, info = env.step(act)
        ret += torch.where(alive, r, torch.zeros_like(r))
        cost += torch.where(alive, info["cost"], torch.zeros_like(r))
        length += alive.float()
        alive &= ~(term | trunc)
    if metrics:
        raw = torch.stack(acc, dim=1)
    if obs_stats:
        slab = _compose_slab(s1, s2)
    return ret, length, cost, raw, slab


def _population_result(env, population, P, E, T, flown, metrics, obs_stats, rec, u0, log_dir):
    """What evaluate_population returns, from a flight's device tensors; the CSVs of log_dir"""
    ret, length, cost, raw, slab = flown
    D, step_seconds = env.obs_dim, float(env.cfg.time_step) * int(env.cfg.aggregate_phy_steps)
    ret, length, cost = ret.cpu().reshape(P, E), length.cpu().reshape(P, E), cost.cpu().reshape(P, E)
    fm = FlightMetrics(raw.cpu().reshape(P, E, len(METRIC_NAMES)), length, step_seconds) if metrics else None
    if log_dir is not None:
        for p in range(P):
            d = os.path.join(log_dir, str(p))
            _write_episode_csvs(d, ret[p], cost[p])
            if metrics:  # one row per episode: the eight raw values and the length
                with open(os.path.join(d, "metrics.csv"), "w") as f:
                    f.write(",".join(METRIC_NAMES) + ",length\n")
                    for e in range(E):
                        f.write(",".join(repr(float(x)) for x in fm.raw[p, e]) + f",{float(length[p, e])!r}\n")
    out = (ret, length, cost, fm) if metrics else (ret, length, cost)
    if obs_stats:
        shift = population.mean.cpu().double() if population.mean is not None else torch.zeros(P, D, dtype=torch.float64)
        out = out + (ObsSums(slab, length.double().sum(dim=1), shift),)
    if rec is not None:
        _, R, flight, obs_rec = rec
        fl = flight.permute(2, 0, 1, 3).contiguous().cpu().reshape(P, R, T, 16)  # [column, step, piece, 4]: the 12 log columns, then the action
        out = out + (Flights(fl[..., :12], fl[..., 12:], None if obs_rec is None else obs_rec.permute(1, 0, 2).contiguous().cpu().reshape(P, R, T, D),
                             length[:, :R], step_seconds, u0.reshape(P, R, 4),
                             control_mode={v: k for k, v in native.CONTROL_MODES.items()}[int(env.cfg.control_mode)]),)
    return out


@torch.no_grad()
def evaluate_population(env, population, fused="auto", log_dir=None, *, max_steps=None, metrics=False, obs_stats=False,
                        history_fused=False, record=None, record_observations=True, record_limit_bytes=1 << 30, history_latency_fused=False,
                        deep_forms_fused=False, history_stats_fused=False):
    """-> (returns, ep_lengths, costs), each [P, E] float32 on the CPU: policy p of `population` flies the E = num_envs / P
    envs of block p, one episode per env, deterministically (action = actor mean), as `evaluate` does for one policy.
    metrics=True: -> (returns, ep_lengths, costs, FlightMetrics) -- the first three are the same bits; the kernel path is
    pds_evaluate_policies_metrics, the composed path reads rpy, omega and last_action in front of every step and sums with
    separate torch ops: the same bits again.
    obs_stats=True: the return value gains a LAST element, an `ObsSums`: per policy and feature the sums of d = o - mean[p] and
    d^2 over every observation the policy acted on in a first episode.  The kernel path is pds_evaluate_policies_stats (it also
    produces the metrics: metrics=False drops them); the composed path keeps per-env float32 sums with one torch op per
    difference, product and sum and adds them in the kernel's tree order (`tree_reduce_rows`): the same slab on the bits.
    record=R (a positive multiple of 64, at most E; not together with obs_stats): the return value gains a LAST element, a
    `Flights`: of every policy's first R episodes the true state x(s) the policy acted in, the raw action a(s) and -- unless
    record_observations=False -- the raw observation o(s) it acted on, for every step s < length; rows past an episode's end
    are zero.  Not recorded: the terminal state x(L) and the terminal observation (a finished env is reset in place inside the
    step).  The kernel path is pds_evaluate_policies_record (it also produces the metrics: metrics=False drops them); the
    composed path -- every env without a fused kernel, and observation histories without history_fused=True; o(s) of a history
    env is the history the actor read, H x half columns on either path -- reads pos, vel, rpy and omega in front of every step:
    the same bits.  The record takes max_steps x P x R x (64 + 4 D)
    bytes on the device and again on the host; above record_limit_bytes the call raises ValueError before it allocates.

    fused=True: one launch (pds_evaluate_policies, csrc/pds_evaluate.h); NotImplementedError where no kernel is built --
    observation_history_size != 2 included -- with the env untouched.  fused=False: the composed path, per step one
    pds_mlp_forward per policy on its block of the observation + env.step + the accumulator updates of `evaluate`: the same
    bits.  fused="auto": the kernel where it is built, the composed path elsewhere.
    history_fused=True (it changes nothing at observation_history_size == 2): an env with another history size H flies in one
    launch too (pds_evaluate_policies_history, csrc/pds_evaluate_hist.h: the same bits as its composed path, metrics=True served
    from the same launch; with record=R pds_evaluate_policies_history_record, the record form of the same kernel) where
    `fused_history_evaluation_built(env)` holds; where it does not, and with obs_stats=True unless history_stats_fused=True says
    otherwise, fused=True raises NotImplementedError with the env untouched and "auto" runs the composed path.
    history_stats_fused=True (it changes nothing without history_fused=True and obs_stats=True, and nothing at
    observation_history_size == 2): the observation sums of a history env come from the launch too
    (pds_evaluate_policies_history_stats, the stats form of the same kernel: the same slab on the bits as its composed path, the
    metrics from the same launch) where `fused_history_stats_evaluation_built(env)` holds; where it does not, fused=True raises
    NotImplementedError with the env untouched and "auto" runs the composed path.  The slab of a history env -- on either path --
    is [tiles, 4, 2, W] with W = slab_features(H x half): 64, 96, 128 or 192 columns.
    history_latency_fused=True (it changes nothing without history_fused=True, and nothing on an env without the latency ring):
    an env created with history_latency=True on the latency ring flies in one launch as well -- the plain / metrics call
    pds_evaluate_policies_history_latency, record=R pds_evaluate_policies_history_latency_record, obs_stats=True with
    history_stats_fused=True pds_evaluate_policies_history_latency_stats (include/pds_history_latency_evaluate.h: the V::LAT forms
    of the same kernel, the same bits as the composed path) -- where `fused_history_latency_evaluation_built(env)` /
    `fused_history_latency_stats_evaluation_built(env)` hold; where they do not (TakeOff, the Kalman hold, the ground effect,
    partial noise, views frozen by set_latency), fused=True raises NotImplementedError with the env untouched and "auto" runs the
    composed path.
    A population of actors with THREE or FOUR hidden layers (`population.deep`) flies in one launch through
    pds_evaluate_policies_deep (include/pds_evaluate_deep.h, csrc/pds_evaluate_deep.h: the same bits as its composed path, the
    metrics from the same launch) where `fused_deep_evaluation_built(env, population)` holds and the call is plain or
    metrics=True; with obs_stats=True or record=R, and on an env outside that kernel's family (the latency ring, a PID control
    mode, the Kalman hold, the ground effect off TakeOff), fused=True raises NotImplementedError with the env untouched and "auto"
    runs the composed path, which serves every form with one pds_mlp_deep_forward per policy and step.  An env with
    observation_history_size != 2 raises NotImplementedError for such a population on either path; the history keywords change nothing.
    deep_forms_fused=True (it changes nothing for a population with two hidden layers, and nothing for the plain and the metrics
    call): obs_stats=True and record=R of a deep population come from one launch as well -- pds_evaluate_policies_deep_stats and
    pds_evaluate_policies_deep_record (include/pds_evaluate_deep_forms.h: the stats and the record form of the same kernel, the
    same slab and the same record on the bits as the composed path, the metrics from the same launch; record_observations=False
    hands the kernel no observation array) -- where `fused_deep_forms_evaluation_built(env, population, form)` holds; where it does
    not, fused=True raises NotImplementedError with the env untouched and "auto" runs the composed path.
    The env is reset first and not afterwards: after the fused path it refuses to step until the next reset() of every env
    (a masked reset is refused as well).  `population` is not modified: the call works on device copies of its tensors.
    max_steps: the number of steps flown, by default the env's max_episode_steps (the TimeLimit ends every episode by then)."""
    P, E, T, R, form, use_kernel, H = _plan_population(env, population, fused, max_steps, metrics, obs_stats, history_fused, record,
                                                       record_limit_bytes, history_stats_fused, history_latency_fused, deep_forms_fused)
    # (the two families of predicates exclude each other -- with and without the ring --: a kernel flight the latency one allows is its)
    latency = use_kernel and H is not None and bool(history_latency_fused) and fused_history_latency_evaluation_built(env)
    population = population.to(env.device)
    dev, D = env.device, env.obs_dim
    rec = u0 = None
    obs, _ = env.reset()
    if R is not None:  # zero-filled: the rows past an episode's end stay zero on both paths
        rec_env = (torch.arange(P, device=dev).unsqueeze(1) * E + torch.arange(R, device=dev).unsqueeze(0)).reshape(-1)  # [P R] env of column j
        u0 = env.get_state("last_action")[rec_env].cpu()  # the command in force before the first (Flights.metrics)
        rec = (rec_env, R, torch.zeros(T, 4, P * R, 4, device=dev), torch.zeros(T, P * R, D, device=dev) if record_observations else None)
    if use_kernel:
        flown = _fly_kernel(env, population, obs, P, E, T, form, H, rec, latency)
    else:
        flown = _fly_composed(env, population, obs, P, E, T, metrics, obs_stats, rec)
    return _population_result(env, population, P, E, T, flown, metrics, obs_stats, rec, u0, log_dir)
