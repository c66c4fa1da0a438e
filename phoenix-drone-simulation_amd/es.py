"""An evolution strategy over actor weights: the trainer that `evaluate_population` (evaluation.py) was written to serve.

OpenAI-ES (Salimans et al. 2017, "Evolution Strategies as a Scalable Alternative to Reinforcement Learning"): a population of
antithetic pairs mu +- sigma eps_i around one centre, centred-rank fitness shaping, Adam on the centre.  It is not part of the
reference; it stands where the reference spreads independent evaluations over MPI cores, and it is the trainer that spends its
time where this simulator is strong -- P policies x E episodes of a generation fly in ONE launch (pds_evaluate_policies), the
update touches param_count floats.

The device side is csrc/pds_es.hip: `pds_es_perturb` writes theta [P, n] from the centre (no host copy), `pds_es_gradient` turns
P fitness values into the search gradient by REGENERATING the noise from its counters (the draws of
pds_gaussian_sample), so the noise is never stored.  fused=False composes the same recipe from entry points that were there
before: the noise through `fused.gaussian_sample` on zeros, perturbation and weighted sum as torch ops."""
import ctypes as C
import math
import os
import time

import torch

from . import native
from .evaluation import METRIC_NAMES, PolicyPopulation, evaluate_population
from .fused import gaussian_sample
from .ppo import ActorCritic

WARMUP_STEPS = 32  # obs_stats="warmup": random-action env steps that feed the observation statistics before they are frozen


def centered_ranks(fitness):
    """Centred-rank shaping: the rank of every fitness value among the P (stable argsort: ties go to the lower index first),
    mapped linearly onto [-0.5, 0.5].  NaN ranks below everything, -inf included.  -> float32, on fitness's device."""
    f = torch.as_tensor(fitness, dtype=torch.float32).reshape(-1)
    P = f.numel()
    nan = torch.isnan(f)
    order = torch.argsort(torch.where(nan, torch.full_like(f, -math.inf), f), stable=True)
    first = nan[order]
    order = torch.cat([order[first], order[~first]])  # (both halves keep their order: NaNs by index, then the rest)
    ranks = torch.empty(P, dtype=torch.float32, device=f.device)
    ranks[order] = torch.arange(P, dtype=torch.float32, device=f.device)
    return ranks / (P - 1) - 0.5 if P > 1 else torch.zeros_like(ranks)


def pair_weights(u):
    """[2 H] shaped fitness -> [H]: what the antithetic pair i contributes along eps_i, u[2 i] - u[2 i + 1]."""
    u = torch.as_tensor(u)
    return u[0::2] - u[1::2]


def ars_pair_weights(fitness, top_b):
    """The pair weights of Augmented Random Search (Mania et al. 2018, "Simple random search provides a competitive approach to
    reinforcement learning", algorithm 2, V1-t / V2-t): fitness [2 H], rows 2 i / 2 i + 1 the returns r+ / r- of pair i.  The
    pairs are ranked by max(r+, r-) (stable: ties go to the lower index); the best `top_b` get (r+ - r-) / sigma_R, sigma_R the
    standard deviation (as numpy.std: divisor 2 top_b) of their 2 top_b returns; every other pair 0.  A pair with a non-finite
    return gets 0 and takes no place among the top_b.  sigma_R = 0 (all 2 top_b returns equal: every difference is 0): zeros.
    -> float32 [H] on fitness's device."""
    f = torch.as_tensor(fitness, dtype=torch.float32).reshape(-1)
    if f.numel() < 2 or f.numel() % 2 != 0:
        raise ValueError(f"fitness must hold the returns of whole pairs, got {f.numel()} values")
    H, b = f.numel() // 2, int(top_b)
    if b < 1 or b > H:
        raise ValueError(f"top_b = {top_b}: between 1 and the number of pairs {H}")
    plus, minus = f[0::2], f[1::2]
    ok = torch.isfinite(plus) & torch.isfinite(minus)
    score = torch.where(ok, torch.maximum(plus, minus), torch.full_like(plus, -math.inf))
    order = torch.argsort(score, descending=True, stable=True)
    chosen = order[:b]
    chosen = chosen[ok[chosen]]
    w = torch.zeros(H, dtype=torch.float32, device=f.device)
    if chosen.numel() == 0:
        return w
    sigma_r = torch.cat([plus[chosen], minus[chosen]]).std(unbiased=False)
    if not bool(sigma_r > 0):
        return w
    w[chosen] = (plus[chosen] - minus[chosen]) / sigma_r
    return w


def penalised_return(weights):
    """A ready-made `fitness` for ESTrainer: the mean over the E episodes of return - sum_m weights[m] x raw_m, with raw_m the
    raw per-episode sum of flight metric m (evaluation.METRIC_NAMES: "action_rate_sq", "rate_sq", ...).  The raw values are sums
    over the steps of the episode, as the return is, so a weight is a penalty per step.  Unknown names raise ValueError."""
    weights = {str(k): float(w) for k, w in dict(weights).items()}
    unknown = sorted(set(weights) - set(METRIC_NAMES))
    if unknown:
        raise ValueError(f"unknown flight metrics {unknown}: one of {list(METRIC_NAMES)}")

    def fitness(ret, length, cost, metrics):
        score = ret.clone()
        for name, w in weights.items():
            score = score - w * metrics.raw[..., METRIC_NAMES.index(name)]
        return score.mean(dim=1)

    fitness.weights = weights
    return fitness


class ESTrainer:
    """OpenAI-ES on a DroneVecEnv of N = population x E envs (E a multiple of 64: evaluate_population's layout).
    The defaults are starting values, not tuned ones.

    The centre is an ActorCritic (ppo.py) whose `pi.net` parameters are views into ONE flat float32 tensor `mu` in the layout
    of pds_mlp_param_count, so checkpoints are the reference's (`save_checkpoint`).  hidden_sizes: two widths, or THREE or FOUR
    widths of 1 .. 64 each (include/pds_mlp_deep.h: the (50, 30, 20) and (32, 32, 32, 32) actors of the reference's architecture
    search) -- `mu` is then W1 b1 .. W(L+1) b(L+1), the layout of pds_mlp_deep_param_count and of PolicyPopulation.from_flat, the
    Adam step pds_mlp_deep_adam_step, the generation's launch pds_evaluate_policies_deep; an env with observation_history_size != 2
    has no path at these depths (ValueError).  deep_forms_fused: the `deep_forms_fused` of the generation's call -- with
    obs_stats="online" the sums of a deep centre's generation come from the launch too (pds_evaluate_policies_deep_stats, where it
    is built: the same statistics and the same centre on the bits); it changes nothing at two hidden layers.  obs_stats: None (mean 0, std 1), a
    (mean, std) pair, or "warmup" (WARMUP_STEPS random-action steps through OnlineMeanStd); frozen afterwards -- the
    statistics are not perturbed.  obs_stats="online" starts as "warmup" does and then keeps them running: every generation's
    launch also sums the observations its policies acted on (evaluate_population(..., obs_stats=True)), and their pooled
    moments are merged into `ac.obs_oms` (OnlineMeanStd.merge_moments) behind the generation, so generation g is standardised
    with what the generations before it saw -- "V2" of Augmented Random Search.  The centre's evaluation reads the statistics
    its population flew with and contributes none.
    shaping: "ranks" (centred ranks, scale -1 / (2 H sigma)) or "ars" (ars_pair_weights on the best `top_b` pairs -- by default
    all H --, scale -1 / top_b: ARS divides by sigma_R inside the weights and not by the exploration noise).
    evaluate_fused: the `fused` of the generation's evaluate_population call ("auto": the kernel where it is built); history_fused: its `history_fused`
    -- an env with observation_history_size != 2 flies its generations in one launch too; obs_stats="online" stays composed there unless
    history_stats_fused=True, the `history_stats_fused` of the call: the sums then come from the launch as well (pds_evaluate_policies_history_stats,
    where it is built: the same statistics and the same centre on the bits).  history_latency_fused: the `history_latency_fused` of both calls --
    an env created with history_latency=True on the latency ring flies them in one launch as well (pds_evaluate_policies_history_latency*).  eval_every: every that many generations the centre alone flies all N envs.
    fitness: None (the mean return over the E episodes) or a callable fitness(ret, length, cost, metrics) -> [P] on the [P, E]
    results and the FlightMetrics of evaluate_population(..., metrics=True), e.g. penalised_return({"action_rate_sq": 0.1})."""

    def __init__(self, env, population, hidden_sizes=(50, 50), activation="relu", sigma=0.02, lr=0.01, l2=0.005,
                 betas=(0.9, 0.999), seed=0, obs_stats=None, fused=True, eval_every=10, adam_eps=1e-8, fitness=None, shaping="ranks", top_b=None,
                 evaluate_fused="auto", history_fused=False, history_stats_fused=False, history_latency_fused=False,
                 deep_forms_fused=False):
        P, N = int(population), int(env.num_envs)
        hidden_sizes = tuple(int(h) for h in hidden_sizes)
        if not 2 <= len(hidden_sizes) <= native.MLP_DEEP_MAX_HIDDEN:
            raise ValueError(f"hidden_sizes = {hidden_sizes}: 2 to {native.MLP_DEEP_MAX_HIDDEN} hidden layers")
        deep = len(hidden_sizes) > 2
        if deep and any(h < 1 or h > 64 for h in hidden_sizes):
            raise ValueError(f"hidden_sizes = {hidden_sizes}: with {len(hidden_sizes)} hidden layers every width is 1 to 64")
        if deep and int(getattr(env, "observation_history_size", 2)) != 2:
            raise ValueError(f"hidden_sizes = {hidden_sizes} on an env with observation_history_size {env.observation_history_size}: "
                             "3 and 4 hidden layers fly at observation_history_size 2 only (2 hidden layers: any)")
        if P < 2 or P % 2 != 0:
            raise ValueError(f"population = {P}: antithetic pairs need an even number of policies")
        if N % P != 0:
            raise ValueError(f"env.num_envs = {N} is not population x E for population = {P}")
        if (N // P) % 64 != 0:
            raise ValueError(f"episodes per policy E = {N} / {P} = {N // P} is not a multiple of 64 (one tile)")
        if activation not in native.ACTIVATIONS:
            raise ValueError(f"activation {activation!r}: relu or tanh")
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"sigma = {sigma}")
        if fitness is not None and not callable(fitness):
            raise ValueError("fitness: None or a callable fitness(ret, length, cost, metrics) -> [P]")
        if shaping not in ("ranks", "ars"):
            raise ValueError("shaping: 'ranks' or 'ars'")
        self.shaping, self.top_b = shaping, int(P // 2 if top_b is None else top_b)
        if self.top_b < 1 or self.top_b > P // 2:
            raise ValueError(f"top_b = {top_b}: between 1 and the number of pairs {P // 2}")
        self.online = isinstance(obs_stats, str) and obs_stats == "online"
        self.evaluate_fused = evaluate_fused
        self.history_fused = history_fused
        self.history_stats_fused = history_stats_fused
        self.history_latency_fused = history_latency_fused
        self.deep_forms_fused = bool(deep_forms_fused)
        self.deep = deep
        self.fitness = fitness
        self.env, self.P, self.H, self.E, self.N = env, P, P // 2, N // P, N
        self.hidden_sizes, self.activation = hidden_sizes, activation
        self.sigma, self.lr, self.l2, self.betas, self.adam_eps = float(sigma), float(lr), float(l2), tuple(betas), float(adam_eps)
        self.seed, self.fused, self.eval_every = int(seed) & 0xFFFFFFFFFFFFFFFF, bool(fused), int(eval_every)
        self.pair_base = 0  # (a later multi-rank form gives each rank a slice of the pairs)
        self.lib = native.load()
        dev = env.device
        torch.manual_seed(seed)
        self.ac = ActorCritic(env.obs_dim, env.act_dim,
                              {"pi": {"hidden_sizes": self.hidden_sizes, "activation": activation},
                               "val": {"hidden_sizes": (64, 64), "activation": "tanh"}}).to(dev)
        # the flat centre: W1, b1, ..., W(L+1), b(L+1) in torch parameter order; the actor's parameters become views into it
        lin = [l for l in self.ac.pi.net if isinstance(l, torch.nn.Linear)]
        params = [p for l in lin for p in (l.weight, l.bias)]
        self.n = sum(p.numel() for p in params)
        self.mu = torch.cat([p.detach().reshape(-1) for p in params]).contiguous()
        off = 0
        for p in params:
            p.data = self.mu[off:off + p.numel()].view_as(p)
            off += p.numel()
        if deep:  # struct pds_mlp_deep: read by pds_mlp_deep_adam_step (by reference)
            m = native.mlp_deep(env.obs_dim, self.hidden_sizes, env.act_dim, activation, tensors=params)
            if self.lib.pds_mlp_deep_param_count(C.byref(m)) != self.n:
                raise ValueError("layer sizes outside the deep kernels' range (d_in <= 64, 3 or 4 hidden widths of 1 .. 64, d_out <= 8)")
        else:
            m = native.mlp(env.obs_dim, *self.hidden_sizes, env.act_dim, activation, tensors=params)
            if self.lib.pds_mlp_param_count(C.byref(m)) != self.n:
                raise ValueError("layer sizes outside the fused kernels' range (d_in <= 192, h1, h2 <= 64, d_out <= 8)")
        self._mlp = m
        self.Q = (self.n + 7) // 8
        self.grad = torch.zeros(self.n, device=dev)
        self.exp_avg, self.exp_avg_sq = torch.zeros(self.n, device=dev), torch.zeros(self.n, device=dev)
        self._theta = torch.empty(P, self.n, device=dev)
        self._workspace = torch.empty(int(self.lib.pds_es_workspace_floats(self.n, self.H)), device=dev) if self.fused else None
        self._set_obs_stats(obs_stats)
        oms = self.ac.obs_oms
        self._mean_P = oms.mean.detach().expand(P, -1).contiguous()
        self._std_P = oms.std.detach().expand(P, -1).contiguous()
        self.generation = 0
        self.log = []
        self._t_total = 0.0

    # ---- observation statistics ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _set_obs_stats(self, obs_stats):
        oms = self.ac.obs_oms
        if obs_stats is None:
            return
        if isinstance(obs_stats, str):
            if obs_stats not in ("warmup", "online"):
                raise ValueError("obs_stats: None, (mean, std), 'warmup' or 'online'")
            env = self.env
            gen = torch.Generator(device=env.device)
            gen.manual_seed(self.seed & 0x7FFFFFFFFFFFFFFF)
            obs, _ = env.reset()
            oms.update(obs)
            for _ in range(WARMUP_STEPS):
                act = torch.rand(env.num_envs, env.act_dim, device=env.device, generator=gen) * 2.0 - 1.0
                obs, *_ = env.step(act)
                oms.update(obs)
            return
        mean, std = obs_stats
        oms.mean.data.copy_(torch.as_tensor(mean, dtype=torch.float32).reshape(-1))
        oms.std.data.copy_(torch.as_tensor(std, dtype=torch.float32).reshape(-1))

    @torch.no_grad()
    def merge_obs_sums(self, sums):
        """obs_stats="online": the pooled moments of a generation's ObsSums into `ac.obs_oms`, and the new statistics IN PLACE
        into the [P, D] rows the next ask() hands to the kernel (their addresses stay)."""
        count, mean, m2 = sums.pooled()
        oms = self.ac.obs_oms
        oms.merge_moments(float(count), mean, m2)
        self._mean_P.copy_(oms.mean.detach().expand(self.P, -1))
        self._std_P.copy_(oms.std.detach().expand(self.P, -1))

    # ---- the two halves of a generation ----------------------------------------------------------------------------------
    def _noise(self):
        """eps [H, n] of this generation through pds_gaussian_sample (the composed path, and what the tests compare against)"""
        dev, rows = self.mu.device, self.H * self.Q
        out, logp = torch.empty(rows, 8, device=dev), torch.empty(rows, device=dev)
        gaussian_sample(torch.zeros(rows, 8, device=dev), torch.zeros(8, device=dev), out, logp, self.seed, self.generation,
                        id_base=self.pair_base * self.Q)
        return out.reshape(self.H, 8 * self.Q)[:, :self.n]

    def _population(self, theta, mean, std):
        return PolicyPopulation.from_flat(theta, self.env.obs_dim, self.hidden_sizes, self.activation, mean, std,
                                          self.ac.obs_oms.eps)

    @torch.no_grad()
    def ask(self):
        """-> the PolicyPopulation of this generation: rows 2 i / 2 i + 1 = mu +- sigma eps_i.  Its `theta` is the device tensor
        the kernel wrote (the trainer's own buffer, overwritten by the next ask)."""
        theta = self._theta
        if self.fused:
            native.call("pds_es_perturb", self.mu, self.n, self.H, self.sigma, self.seed, self.generation, self.pair_base, theta, on=theta)
        elif self.deep:
            # a deep centre: the contract of pds_es_perturb as tests/test_gpu_es.py states it, float32(float64(mu) +- float64(sigma)
            # float64(eps)) -- the product of two float32 values is exact in float64, so this is the kernel's fmaf up to the double
            # rounding, and the two recipes hand the same population to the launch.  (Two hidden layers keep the float32 ops below,
            # whose bits their runs have.)
            step = float(torch.tensor(self.sigma, dtype=torch.float32)) * self._noise().double()
            theta[0::2] = (self.mu.double() + step).float()
            theta[1::2] = (self.mu.double() - step).float()
        else:
            step = self.sigma * self._noise()
            theta[0::2] = self.mu + step
            theta[1::2] = self.mu - step
        return self._population(theta, self._mean_P, self._std_P)

    @torch.no_grad()
    def tell(self, fitness):
        """One update from the fitness [P] of the population of the last ask(): centred ranks -> pair weights -> search gradient
        (scale -1 / (2 H sigma): pds_adam_step descends, so the centre climbs fitness) -> Adam on mu -> generation += 1."""
        f = torch.as_tensor(fitness, dtype=torch.float32).reshape(-1)
        if f.numel() != self.P:
            raise ValueError(f"fitness must hold {self.P} values, got {f.numel()}")
        if not bool(torch.isfinite(f).any()):
            raise FloatingPointError(f"every fitness of generation {self.generation} is non-finite")
        if self.shaping == "ars":
            w = ars_pair_weights(f, self.top_b).to(self.mu.device).contiguous()
            scale = -1.0 / self.top_b
        else:
            w = pair_weights(centered_ranks(f)).to(self.mu.device).contiguous()
            scale = -1.0 / (2.0 * self.H * self.sigma)
        if self.fused:
            native.call("pds_es_gradient", w, self.mu, self.n, self.H, scale, self.l2, self.seed, self.generation, self.pair_base,
                        self.grad, self._workspace, on=w)
        else:
            self.grad.copy_(scale * (w @ self._noise()) + self.l2 * self.mu)
        # (a deep centre: the same step over struct pds_mlp_deep's 2 (L + 1) tensors, which are `mu` end to end)
        name, m = ("pds_mlp_deep_adam_step", C.byref(self._mlp)) if self.deep else ("pds_adam_step", self._mlp)
        native.call(name, m, self.grad, self.exp_avg, self.exp_avg_sq, self.generation + 1, self.lr, self.betas[0],
                    self.betas[1], self.adam_eps, on=self.mu)
        self.generation += 1

    @torch.no_grad()
    def evaluate_centre(self):
        """The centre alone on all N envs (P = 1) -> (returns, lengths, costs), each [1, N] on the CPU."""
        oms = self.ac.obs_oms
        pop = self._population(self.mu.unsqueeze(0), oms.mean.detach().unsqueeze(0), oms.std.detach().unsqueeze(0))
        return evaluate_population(self.env, pop, fused="auto", history_fused=self.history_fused, history_latency_fused=self.history_latency_fused)

    def _sync(self):
        torch.cuda.synchronize(self.env.device)
        return time.perf_counter()

    def learn_one_generation(self):
        """ask -> evaluate_population (fitness = mean return over the E episodes) -> tell.  Every `eval_every` generations the
        centre the population was drawn around flies all N envs first (`centre_return`, NaN otherwise).  -> the log entry:
        generation (updates done), fitness mean / min / max over the finite values, mean episode length, centre return, gradient
        norm, env steps flown (the sum of the episode lengths, the centre's included), seconds in perturb / evaluate / update."""
        t0 = self._sync()
        pop = self.ask()
        t1 = self._sync()
        out = evaluate_population(self.env, pop, fused=self.evaluate_fused, metrics=self.fitness is not None, obs_stats=self.online,
                                  history_fused=self.history_fused, history_stats_fused=self.history_stats_fused,
                                  history_latency_fused=self.history_latency_fused, deep_forms_fused=self.deep_forms_fused)
        sums = out[-1] if self.online else None
        if self.fitness is None:
            ret, length = out[0], out[1]
            fitness = ret.mean(dim=1)
        else:
            ret, length, cost, fm = out[:4]
            fitness = torch.as_tensor(self.fitness(ret, length, cost, fm), dtype=torch.float32).reshape(-1)
        t2 = self._sync()
        steps, centre = float(length.sum()), float("nan")
        if self.eval_every > 0 and self.generation % self.eval_every == 0:
            c_ret, c_len, _ = self.evaluate_centre()
            centre, steps = float(c_ret.mean()), steps + float(c_len.sum())
        t3 = self._sync()
        self.tell(fitness)
        if self.online:  # behind the centre's evaluation: it flew with its population's statistics
            self.merge_obs_sums(sums)
        t4 = self._sync()
        finite = fitness[torch.isfinite(fitness)]
        self._t_total += t4 - t0
        info = dict(generation=self.generation, fitness_mean=float(finite.mean()), fitness_min=float(finite.min()),
                    fitness_max=float(finite.max()), ep_len=float(length.mean()), centre_return=centre,
                    grad_norm=float(self.grad.norm()), env_steps=steps, t_perturb=t1 - t0, t_evaluate=t2 - t1,
                    t_update=t4 - t3, time=self._t_total)
        self.log.append(info)
        return info

    def learn(self, generations, verbose=False):
        for _ in range(int(generations)):
            info = self.learn_one_generation()
            if verbose:
                print({k: (round(v, 4) if isinstance(v, float) else v) for k, v in info.items()})
        return self.ac, self.env

    # ---- artefacts ---------------------------------------------------------------------------------------------------------
    def save_checkpoint(self, log_dir):
        """As PPOTrainer.save_checkpoint: `torch_save/model.pt` = the centre's ActorCritic.state_dict() with the reference's keys,
        and the firmware JSON of the actor next to it (examples/evaluate_policies.py reads the directory)."""
        from .policy_io import convert_actor_critic_to_json
        os.makedirs(os.path.join(log_dir, "torch_save"), exist_ok=True)
        path = os.path.join(log_dir, "torch_save", "model.pt")
        torch.save({k: v.detach().cpu() for k, v in self.ac.state_dict().items()}, path)
        convert_actor_critic_to_json(self.ac, os.path.join(log_dir, "model.json"), self.activation)
        return path

    def _progress_columns(self):
        """(progress.csv column, log key) pairs of write_progress_csv"""
        return [("Generation", "generation"), ("Fitness/Mean", "fitness_mean"), ("Fitness/Min", "fitness_min"),
                ("Fitness/Max", "fitness_max"), ("EpLen/Mean", "ep_len"), ("CentreRet/Mean", "centre_return"),
                ("GradNorm", "grad_norm"), ("EnvSteps", "env_steps"), ("Time/Perturb", "t_perturb"),
                ("Time/Evaluate", "t_evaluate"), ("Time/Update", "t_update"), ("Time", "time")]

    def write_progress_csv(self, path):
        """The per-generation log, one row per generation (the form of PPOTrainer.write_progress_csv)."""
        cols = self._progress_columns()
        with open(path, "w") as f:
            f.write(",".join(c for c, _ in cols) + "\n")
            for row in self.log:
                f.write(",".join(str(row.get(k, "")) for _, k in cols) + "\n")
