"""The closed loop of tests/flight_oracle.py `fly` restated with an L-layer numpy actor in front of the CPU oracle: the reference
of the population evaluation for actors with THREE or FOUR hidden layers (pds_evaluate_policies_deep and the composed path on
pds_mlp_deep_forward).  TEST INFRASTRUCTURE: tests/test_flight_deep_oracle_cpu.py pins its float32 run against its float64 run,
its actor against a float64 torch Sequential, and checks that the mistakes a deep kernel could make would show;
tests/test_gpu_evaluate_deep.py holds the kernel and the composed path against the float64 run.

Nothing here comes from phoenix_drone_simulation_amd.  What is kept of a flight, and when it is read off the oracle, is
flight_oracle.fly's, word for word (state, action, observation and last_action IN FRONT OF env.step of step s; the first
episode's sums); the metrics are flight_oracle.metrics_of, the observation sums flight_oracle.obs_sums_of, the units
flight_oracle.units_of.  What differs is the actor: a row of the population is W1 b1 ... W(L+1) b(L+1) in torch order (weight
[out, in], then bias), L = len(hidden) hidden layers with one activation, none on the output.

A DeepCase is an evaluate_oracle.Case whose `shape` is (d_in, h1, ..., hL).  Its flights live where flight_oracle.flight keeps
them (case._memo[("flight", precision)]), so flight_oracle.flight, agreeing and units_of, evaluate_oracle.unit_of and the check
functions of the GPU reference tests serve it unchanged; `flight` below is the way in -- it flies on first use.

`precision` "f64": everything in float64, the action rounded to float32 where the device hands it to the env.  "f32": oracle,
network and every running sum in float32."""
import numpy as np

import evaluate_oracle as eo
import flight_oracle as fo
from oracle import oracle


def param_count(sizes):
    """sizes = (d_in, h1, ..., hL, d_out)"""
    return sum(sizes[j + 1] * sizes[j] + sizes[j + 1] for j in range(len(sizes) - 1))


def split_rows(rows, sizes, real):
    """[P, param_count] -> [(W [P, out, in], b [P, out])] per layer, torch order"""
    rows = np.asarray(rows)
    assert rows.ndim == 2 and rows.shape[1] == param_count(sizes), (rows.shape, sizes)
    out, k = [], 0
    for n_in, n_out in zip(sizes[:-1], sizes[1:]):
        W = rows[:, k:k + n_out * n_in].reshape(-1, n_out, n_in).astype(real); k += n_out * n_in
        b = rows[:, k:k + n_out].astype(real); k += n_out
        out.append((W, b))
    return out


def actor(layers, x, act):
    """x [G, E, d_in] through group g's network layers[l] = (W [G, out, in], b [G, out]): act behind every layer but the last"""
    for l, (W, b) in enumerate(layers):
        x = np.einsum("goi,gei->geo", W, x) + b[:, None, :]
        if l < len(layers) - 1:
            x = act(x)
    return x


def random_actors(P, d_in, hidden, seed, bias_lo=-0.6, bias_hi=0.6):
    """evaluate_oracle.random_actors' recipe carried to L layers: per policy, per layer, weight then bias, uniform
    +- 1 / sqrt(fan_in) from one RandomState(seed); output biases spread from bias_lo to bias_hi over the policies"""
    sizes = (d_in,) + tuple(hidden) + (4,)
    rs = np.random.RandomState(seed)
    rows = np.empty((P, param_count(sizes)), np.float32)
    for p in range(P):
        k = 0
        for n_in, n_out in zip(sizes[:-1], sizes[1:]):
            for count in (n_out * n_in, n_out):
                rows[p, k:k + count] = ((rs.random_sample(count) * 2 - 1) / np.sqrt(n_in)).astype(np.float32)
                k += count
        rows[p, -4:] += np.float32(bias_lo + (bias_hi - bias_lo) * p / max(P - 1, 1))
    return rows


ACT = {"relu": lambda real: (lambda x: np.maximum(x, real(0))), "tanh": lambda real: np.tanh}


def fly(task, env_kwargs, population_rows, shape, activation, mean, std, eps, E, max_steps, limit, seed, precision, tick0=0,
        net=actor, tile_policy=None):
    """flight_oracle.fly for shape = (d_in, h1, ..., hL): the same dict (ret, length, cost, u0, metrics, sum_d, sum_d2, state,
    action, observation, the unmasked *_all, rows0, rows_all, done_all, cut_all, shift).
    For the teeth tests: `net` (layers, x, act) -> actions replaces the actor; `tile_policy` [N / 64] gives the policy whose row
    and standardisation each 64-env tile flies (default: tile t flies policy t // (E / 64))."""
    real = np.float64 if precision == "f64" else np.float32
    d_in, hidden = int(shape[0]), tuple(int(h) for h in shape[1:])
    sizes = (d_in,) + hidden + (4,)
    rows = np.asarray(population_rows, np.float32)
    P = rows.shape[0]
    N, T = P * E, int(max_steps)
    assert E % 64 == 0
    tiles = N // 64
    pol = np.arange(tiles) // (E // 64) if tile_policy is None else np.asarray(tile_policy, np.int64)
    layers = [(W[pol], b[pol]) for W, b in split_rows(rows, sizes, real)]  # per TILE: the rows a kernel stages
    act = ACT[activation](real)
    mu = den = None
    if mean is not None:
        mu = np.asarray(mean, np.float32).astype(real)[pol][:, None, :]
        den = np.asarray(std, np.float32).astype(real)[pol][:, None, :] + real(eps)
    env = oracle.OracleBatch(task, N, precision=precision, max_episode_steps=int(limit), **eo.oracle_kwargs(env_kwargs))
    assert env.obs_dim == d_in, (env.obs_dim, d_in)
    f = fo._fields(env)
    obs = np.array(env.reset(seed, tick0), real)
    rows0 = obs.copy()
    u0 = np.array(f["last_action"], real)
    ret, length, cost = np.zeros(N, real), np.zeros(N, real), np.zeros(N, real)
    first = np.ones(N, bool)
    state_all, action_all, obs_all, u_all = (np.zeros((N, T, k), real) for k in (12, 4, d_in, 4))
    rows_all, done_all, cut_all = np.zeros((T, N, env.obs_dim), real), np.zeros((T, N), bool), np.zeros((T, N), bool)
    for s in range(T):
        state_all[:, s] = np.concatenate([f[k] for k in fo.STATE_FIELDS], axis=1)
        u_all[:, s] = f["last_action"]
        obs_all[:, s] = obs
        x = np.asarray(obs, real).reshape(tiles, 64, d_in)
        if mu is not None:
            x = (x - mu) / den
        a = net(layers, x, act)
        assert a.dtype == real and a.shape == (tiles, 64, 4)
        a = a.reshape(N, 4).astype(np.float32)
        action_all[:, s] = a
        row, r, term, trunc, c = env.step(a, seed=seed, tick=tick0 + 1 + s, auto_reset=True)
        done = term.astype(bool) | trunc.astype(bool)
        rows_all[s], done_all[s], cut_all[s] = row, done, trunc.astype(bool) & ~term.astype(bool)
        ret = np.where(first, ret + r, ret).astype(real)
        cost = np.where(first, cost + c, cost).astype(real)
        length = np.where(first, length + real(1), length).astype(real)
        first &= ~done
        obs = np.array(row, real)
    L = length.astype(np.int64)
    on = (np.arange(T)[None, :] < L[:, None])[:, :, None]
    shift = None if mean is None else np.repeat(np.asarray(mean, np.float32).astype(real), E, axis=0)
    s1, s2 = fo.obs_sums_of(obs_all, shift, L, real)
    out = dict(ret=ret, length=length, cost=cost, u0=u0, metrics=fo.metrics_of(state_all[:, :, 6:9], state_all[:, :, 9:12], action_all, u_all, L, real),
               sum_d=s1, sum_d2=s2, state=np.where(on, state_all, 0), action=np.where(on, action_all, 0),
               observation=np.where(on, obs_all, 0), state_all=state_all, action_all=action_all, observation_all=obs_all, u_all=u_all)
    out = {k: np.asarray(v, np.float64).reshape((P, E) + np.shape(v)[1:]) for k, v in out.items()}
    out.update(rows0=rows0.astype(np.float64), rows_all=rows_all.astype(np.float64), done_all=done_all, cut_all=cut_all, shift=shift, history=2)
    return out


class DeepCase(eo.Case):
    """an evaluate_oracle.Case whose actors have len(hidden) = 3 or 4 hidden layers: shape = (d_in,) + hidden"""

    def __init__(self, name, env_id, kwargs, hidden, activation, with_stats, P=8, E=128, limit=40, seed=11, rows_seed=1, terminates=True,
                 bias_lo=-1.4, bias_hi=1.4, max_steps=None):
        d = eo._obs_dim(env_id, kwargs)
        rows = random_actors(P, d, hidden, rows_seed, bias_lo, bias_hi)
        mean = std = None
        if with_stats:  # flight_oracle.HistoryCase's: a per-policy standardisation, std bounded away from 0
            rs = np.random.RandomState(rows_seed + 50)
            mean = (0.1 * rs.standard_normal((P, d))).astype(np.float32)
            std = (0.5 + rs.random_sample((P, d))).astype(np.float32)
        super().__init__(name, env_id, kwargs, rows, (d,) + tuple(hidden), activation, E, limit, max_steps=max_steps, mean=mean, std=std,
                         seed=seed, terminates=terminates)
        self.hidden = tuple(hidden)

    def reference(self, precision):
        fl = flight(self, precision)
        return fl["ret"], fl["length"], fl["cost"]


def flight(case, precision):
    """the flight of a DeepCase, computed once per precision, kept where flight_oracle.flight looks and handed out read-only"""
    key = ("flight", precision)
    if key not in case._memo:
        out = fly(eo.TASK_OF[case.env_id], case.kwargs, case.rows, case.shape, case.activation, case.mean, case.std, case.eps, case.E,
                  case.max_steps, case.limit, case.seed, precision)
        for x in out.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        case._memo[key] = out
    return case._memo[key]


def units_of(case):
    """flight_oracle.units_of on the two flights of a DeepCase (flown here first)"""
    flight(case, "f32"); flight(case, "f64")
    return fo.units_of(case)


# ---- the cases: P = 8, E = 128, limit 40, env seed 11, rows_seed 1; output biases spread from -1.4 to 1.4 -------------------------
LEAN = eo.LEAN
_DEEP = {
    "hover_lean": lambda: DeepCase("hover_lean", eo.HOVER, LEAN, (50, 30, 20), "relu", False),
    "hover_default": lambda: DeepCase("hover_default", eo.HOVER, {}, (32, 32, 32, 32), "tanh", True),
    "circle_lean_motor": lambda: DeepCase("circle_lean_motor", eo.CIRCLE, dict(LEAN, use_motor_dynamics=True), (40, 40, 40), "tanh", True),
    "circle_default": lambda: DeepCase("circle_default", eo.CIRCLE, {}, (25, 25, 25, 25), "relu", False),
    "takeoff_default": lambda: DeepCase("takeoff_default", eo.TAKEOFF, {}, (30, 30, 30), "relu", False, terminates=False),
    "takeoff_ge_lean": lambda: DeepCase("takeoff_ge_lean", eo.TAKEOFF, dict(LEAN, use_ground_effect=True), (64, 64, 64, 64), "tanh", True,
                                        terminates=False),
}
DEEP_CASES = list(_DEEP)
_cases = {}


def deep_case(name):
    """(a table of its own: the names repeat evaluate_oracle's)"""
    if name not in _cases:
        _cases[name] = _DEEP[name]()
    return _cases[name]


def edge_case(edge):
    """the edges of evaluate_oracle._edge on a deep row: Hover lean, P = 4, E = 64, (17, 33, 5) tanh, rows_seed 3"""
    kw = dict(P=4, E=64, rows_seed=3, bias_lo=-0.6, bias_hi=0.6)
    hidden = (17, 33, 5)
    if edge == "max_steps_1":
        return DeepCase(edge, eo.HOVER, LEAN, hidden, "tanh", False, limit=40, max_steps=1, **kw)
    if edge == "max_steps_7_limit_40":
        return DeepCase(edge, eo.HOVER, LEAN, hidden, "tanh", False, limit=40, max_steps=7, **kw)
    if edge == "max_steps_40_limit_25":
        return DeepCase(edge, eo.HOVER, LEAN, hidden, "tanh", False, limit=25, max_steps=40, **kw)
    if edge == "one_tile_ends_by_step_3":  # evaluate_oracle's biases: policy 0 at +3, +3, -3, -3 whatever the network says, the others hover on
        c = DeepCase(edge, eo.HOVER, LEAN, hidden, "tanh", False, limit=40, **dict(kw, bias_lo=0.0, bias_hi=0.0))
        c.rows[0, -4:] = (3.0, 3.0, -3.0, -3.0)
        c.rows[1:, -4:] = np.float32(-0.05)
        return c
    raise KeyError(edge)


EDGES = ("max_steps_1", "max_steps_7_limit_40", "max_steps_40_limit_25", "one_tile_ends_by_step_3")
