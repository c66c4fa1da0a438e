"""The reference flight of evaluate_population on the latency ring with observation_history_size = H: a population flown closed
loop on tests/history_latency_oracle.HistoryLatencyEnv -- the reference's own deque of views of action_buffer[-1] around ONE env of
the CPU oracle, pinned to tests/golden/history_latency.npz by tests/test_history_latency_cpu.py -- with the network, the metric and
the sum definitions of tests/flight_oracle.py.  TEST INFRASTRUCTURE: tests/test_history_latency_evaluate_cpu.py pins its float32 run
to its float64 run and shows that the slips a kernel could make would show; tests/test_gpu_evaluate_history_latency.py holds the
one-launch evaluation and the composed path against the float64 run.

Nothing here comes from phoenix_drone_simulation_amd, and `fly` does not know the closed-form rule: the histories are what
HistoryLatencyEnv returns.  Resets are the device's: env i draws po_philox_reset_sample(seed, i, tick), tick 0 for the first and
1 + s for the one behind step s (tests/test_gpu_history_latency.py, the lockstep test).  The oracle env has no per-step noise
streams here, so the cases are lean ones (no observation noise, no thrust noise, no domain randomisation): the noisy configurations
are held to the composed path bit for bit instead.

`restack` is the closed-form rule of include/pds_history_latency.h written once more, open loop over the rows and actions a flight
kept -- with a `slip` it is one of the MISTAKES a kernel could make (the teeth test); without, it must give `fly`'s histories."""
import numpy as np

import evaluate_oracle as eo
import flight_oracle as fo
import history_latency_oracle as hlo

SLIPS = ("no_rule", "clipped_action", "j_plus_1", "one_slot_more", "one_slot_fewer")


def oracle_kwargs(env_kwargs):
    """the env constructor's kwargs as the oracle takes them: history_latency is the device env's switch, not a configuration"""
    return eo.oracle_kwargs({k: v for k, v in env_kwargs.items() if k != "history_latency"})


def fly(task, env_kwargs, population_rows, shape, activation, mean, std, eps, E, max_steps, limit, seed, precision, history):
    """flight_oracle.fly's dict (the same keys, shapes and masks), flown env by env on HistoryLatencyEnv; also `buf_size` (the
    ring's rows B) and `agg` (aggregate_phy_steps), which `restack` is fed with"""
    real = np.float64 if precision == "f64" else np.float32
    d_in, h1, h2 = shape
    rows = np.asarray(population_rows, np.float32)
    P, H = rows.shape[0], int(history)
    N, T = P * E, int(max_steps)
    W1, b1, W2, b2, W3, b3 = eo.split_rows(rows, d_in, h1, h2, real)
    act = {"relu": lambda x: np.maximum(x, real(0)), "tanh": np.tanh}[activation]
    mu = den = None
    if mean is not None:
        mu = np.asarray(mean, np.float32).astype(real).reshape(P, 1, d_in)
        den = np.asarray(std, np.float32).astype(real).reshape(P, 1, d_in) + real(eps)
    envs = [hlo.HistoryLatencyEnv(task, H, precision, max_episode_steps=int(limit), **oracle_kwargs(env_kwargs)) for _ in range(N)]
    assert envs[0].half * H == d_in, (envs[0].half, H, d_in)
    state_of = lambda o: np.concatenate([o.env.get(k) for k in fo.STATE_FIELDS])  # noqa: E731
    obs = np.stack([o.reset(o.env.philox_reset_sample(seed, i, 0)) for i, o in enumerate(envs)]).astype(real)
    rows0 = np.stack([o.row for o in envs])
    u0 = np.stack([o.env.get("last_action") for o in envs]).astype(real)
    ret, length, cost = np.zeros(N, real), np.zeros(N, real), np.zeros(N, real)
    first = np.ones(N, bool)
    state_all, action_all, obs_all, u_all = (np.zeros((N, T, k), real) for k in (12, 4, d_in, 4))
    rows_all, done_all, cut_all = np.zeros((T, N, 2 * envs[0].half), real), np.zeros((T, N), bool), np.zeros((T, N), bool)
    for s in range(T):
        state_all[:, s] = np.stack([state_of(o) for o in envs])
        u_all[:, s] = np.stack([o.env.get("last_action") for o in envs])
        obs_all[:, s] = obs
        x = np.asarray(obs, real).reshape(P, E, d_in)
        if mu is not None:
            x = (x - mu) / den
        x = act(np.einsum("phd,ped->peh", W1, x) + b1[:, None, :])
        x = act(np.einsum("pkh,peh->pek", W2, x) + b2[:, None, :])
        a = np.einsum("pok,pek->peo", W3, x) + b3[:, None, :]
        assert a.dtype == real
        a = a.reshape(N, 4).astype(np.float32)
        action_all[:, s] = a
        nxt = np.zeros_like(obs)
        for i, o in enumerate(envs):
            h, r, term, trunc, c = o.step(a[i])
            done = term or trunc
            rows_all[s, i], done_all[s, i], cut_all[s, i] = o.row, done, trunc and not term
            if first[i]:
                ret[i] += real(r); cost[i] += real(c); length[i] += real(1)
            if done:  # auto-reset in place: the env restarts from its reset, drawn at the step's tick
                first[i] = False
                h = o.reset(o.env.philox_reset_sample(seed, i, 1 + s))
                rows_all[s, i] = o.row
            nxt[i] = h
        obs = nxt
    L = length.astype(np.int64)
    on = (np.arange(T)[None, :] < L[:, None])[:, :, None]
    shift = None if mean is None else np.repeat(np.asarray(mean, np.float32).astype(real), E, axis=0)
    s1, s2 = fo.obs_sums_of(obs_all, shift, L, real)
    out = dict(ret=ret, length=length, cost=cost, u0=u0,
               metrics=fo.metrics_of(state_all[:, :, 6:9], state_all[:, :, 9:12], action_all, u_all, L, real),
               sum_d=s1, sum_d2=s2, state=np.where(on, state_all, 0), action=np.where(on, action_all, 0),
               observation=np.where(on, obs_all, 0), state_all=state_all, action_all=action_all, observation_all=obs_all, u_all=u_all)
    out = {k: np.asarray(v, np.float64).reshape((P, E) + np.shape(v)[1:]) for k, v in out.items()}
    out.update(rows0=rows0.astype(np.float64), rows_all=rows_all.astype(np.float64), done_all=done_all, cut_all=cut_all, shift=shift,
               history=H, buf_size=envs[0].buf_size, agg=int(envs[0].env.cfg.aggregate_phy_steps))
    return out


def restack(rows0, rows_all, done_all, action_all, H, B, agg, slip=None):
    """the histories in front of steps 0 .. T - 1 [T, N, H half] by the closed-form rule: flight_oracle.stack_reset /
    stack_advance, and between the shift and the restart, at step j = 1, 2, ... of an episode, where j <= H and
    floor(j agg / B) > floor((j - 1) agg / B), the action columns of the slots 0 .. H - j become the step's raw action.
    rows_all[s] is the row step s returned (the reset's where the env finished), action_all [N, T, 4].  `slip`: one of SLIPS."""
    T, N = done_all.shape
    half = rows0.shape[1] // 2
    stack = fo.stack_reset(rows0, H)
    j = np.ones(N, np.int64)  # the step of its episode every env is about to take
    out = [stack]
    for s in range(T - 1):
        a = action_all[:, s]
        if slip == "clipped_action":
            a = np.clip(a, -1.0, 1.0)
        moved = np.concatenate([stack[:, half:], rows_all[s][:, half:]], axis=1)
        jj = j + 1 if slip == "j_plus_1" else j
        views = H - jj + 1 + {"one_slot_more": 1, "one_slot_fewer": -1}.get(slip, 0)
        fire = (jj * agg // B > (jj - 1) * agg // B) & (slip != "no_rule")
        for slot in range(H):
            hit = fire & (slot < views)
            moved[hit, slot * half + half - 4:slot * half + half] = a[hit]
        stack = np.where(done_all[s][:, None], fo.stack_reset(rows_all[s], H), moved)
        j = np.where(done_all[s], 1, j + 1)
        out.append(stack)
    return np.stack(out)


class LatencyCase(eo.Case):
    """a flight_oracle.HistoryCase on the latency ring: `kwargs` are the device env's (use_latency, latency, history_latency=True,
    ...), flown by `fly` above; flight_oracle.flight / units_of / agreeing read its flights from the case's memo"""

    def __init__(self, name, env_id, kwargs, H, hidden, activation, limit, max_steps, with_stats, P=2, E=64, seed=11, rows_seed=1,
                 bias_lo=-1.4, bias_hi=1.4, crash_first=False):
        kwargs = dict(kwargs, use_latency=True, history_latency=True)
        half = eo._obs_dim(env_id, oracle_kwargs(kwargs)) // 2
        d = H * half
        rows = eo.random_actors(P, d, hidden[0], hidden[1], rows_seed, bias_lo, bias_hi)
        if crash_first:  # policy 0: two motors at full thrust and two at none -- the 300 deg/s bound ends its episodes within a few steps
            rows[0, -4:] = np.float32([3.0, 3.0, -3.0, -3.0])
        mean = std = None
        if with_stats:
            rs = np.random.RandomState(rows_seed + 50)
            mean = (0.1 * rs.standard_normal((P, d))).astype(np.float32)
            std = (0.5 + rs.random_sample((P, d))).astype(np.float32)
        super().__init__(name, env_id, kwargs, rows, (d,) + tuple(hidden), activation, E, limit, max_steps=max_steps, mean=mean, std=std,
                         seed=seed)
        self.history, self.half = H, half

    def reference(self, precision):
        fl = flight(self, precision)
        return fl["ret"], fl["length"], fl["cost"]


def flight(case, precision):
    """the flight of a LatencyCase, computed once per precision, read-only, under the key flight_oracle.flight looks up"""
    key = ("flight", precision)
    if key not in case._memo:
        out = fly(eo.TASK_OF[case.env_id], case.kwargs, case.rows, case.shape, case.activation, case.mean, case.std, case.eps, case.E,
                  case.max_steps, case.limit, case.seed, precision, case.history)
        for x in out.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        case._memo[key] = out
    return case._memo[key]


def units_of(case):
    """flight_oracle.units_of over this module's flights"""
    flight(case, "f32"); flight(case, "f64")
    return fo.units_of(case)


# ring rows B x sub-steps agg: (3, 2) fires at j = 2, 3, 5, 6 -- at some but not all j <= H = 4, so "the rule always on" shows --;
# (1, 1) fires at every j; (2, 1) at the even j; H = 1 has one slot, rewritten at j = 1 alone
_CASES = {
    "hover_lean_motor_h4_b3_agg2": lambda: LatencyCase("hover_lean_motor_h4_b3_agg2", eo.HOVER, dict(eo.LEAN, use_motor_dynamics=True, latency=0.035,
                                                       aggregate_phy_steps=2), 4, (32, 48), "tanh", 9, 14, True, rows_seed=3),
    "circle_lean_attrate_h3_b1": lambda: LatencyCase("circle_lean_attrate_h3_b1", eo.CIRCLE, dict(eo.LEAN, control_mode="AttitudeRate", latency=0.015),
                                                     3, (64, 64), "relu", 7, 14, False, rows_seed=2),
    "hover_lean_h6_b2": lambda: LatencyCase("hover_lean_h6_b2", eo.HOVER, dict(eo.LEAN, latency=0.025), 6, (32, 48), "tanh", 8, 14, True, rows_seed=3,
                                            crash_first=True),
    "hover_lean_h1_b1": lambda: LatencyCase("hover_lean_h1_b1", eo.HOVER, dict(eo.LEAN, latency=0.015), 1, (32, 48), "tanh", 5, 12, False, rows_seed=4),
}
CASES = list(_CASES)
RING = {"hover_lean_motor_h4_b3_agg2": (3, 2), "circle_lean_attrate_h3_b1": (1, 1), "hover_lean_h6_b2": (2, 1), "hover_lean_h1_b1": (1, 1)}
case = eo._table(_CASES)
