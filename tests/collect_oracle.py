"""The off-policy collection loop (roll_out, algs/ddpg/ddpg.py:386-429 and algs/sac/sac.py:402-437, for N envs side by side)
restated on the CPU oracle with a plain numpy MLP and the numpy noise contract in front of it.  TEST INFRASTRUCTURE:
tests/test_collect_oracle_cpu.py pins its float32 run against its float64 run, tests/test_gpu_collect_reference.py holds
pds_collect and the composed per-step path against the float64 run, with the float32 run's distance as the unit of the bar.

Nothing here comes from phoenix_drone_simulation_amd: the loop is written out again, from the reference's text --
    o = reset; every step: a = explore(actor(o)); o', r, terminated, truncated = step(a); ep_ret += r; ep_len += 1;
    store (o, a, r, o', terminal) with terminal = False at the time horizon; where the episode is over: log (ep_ret, ep_len),
    reset, ep_ret = ep_len = 0
-- for a vector env with auto-reset: the stored o' of a finished env is its `final_obs` (the returned row is already the next
episode's first), and the log is kept as eight accumulators per 64-env tile (count; sum, sum of squares, min, max of the
return; sum, min, max of the length).  Global env id = row index; the env's seed and ticks as pds_reset / pds_step use them
(reset at tick 0, step s at tick 1 + s); the noise of step s is tests/sampler_oracle.py normals64(N, 4, noise_seed,
first_call + s): sample id = env row.

The two exploration rules (get_action, algs/ddpg/ddpg.py:342-345; SquashedGaussianMLPActor.forward, algs/sac/sac.py:47-76):
    DDPG   a = clip(limit tanh(y) + exp(log_std) z, +-limit)               y = the actor's four outputs
    SAC    a = limit tanh(mu + exp(clip(log_std, -20, 2)) z)               [mu | log_std] = the actor's eight outputs"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import oracle  # noqa: E402

import evaluate_oracle as eo  # noqa: E402
import sampler_oracle as so  # noqa: E402

HOVER, CIRCLE, TAKEOFF = eo.HOVER, eo.CIRCLE, eo.TAKEOFF
DDPG, SAC = 0, 1
MODE_NAME = {DDPG: "ddpg", SAC: "sac"}
TILE = 64
STATS = 8
NEUTRAL = (0.0, 0.0, 0.0, np.inf, -np.inf, 0.0, np.inf, -np.inf)
LEAN = eo.LEAN
MOTOR = dict(use_motor_dynamics=True)
LOG_STD = tuple(float(np.log(v)) for v in (0.1, 0.3, 0.5, 0.7))  # four distinct entries: a permuted component shows
NOISE_SEED = (0xC0FFEE << 32) | 0x5EED0123                       # >= 2^32: the key's high word is in use
FIRST_CALL = 2 ** 33 + 5                                         # ... and the counter's


def random_actor(d_in, h1, h2, mode, seed):
    """a seeded actor as six float32 arrays (torch order: weight [out, in], bias [out]), nn.Linear's initialisation (uniform
    +- 1 / sqrt(fan_in)); the four motors' output biases are driven slightly apart (-0.15 .. 0.15), SAC's log_std rows get a
    bias of -0.5 (sigma about 0.6): under this noise Hover envs tumble over the 300 deg/s bound from the first steps on while
    others reach the TimeLimit"""
    rs = np.random.RandomState(seed)
    d_out = 8 if mode == SAC else 4
    out = []
    for n_out, n_in in ((h1, d_in), (h2, h1), (d_out, h2)):
        out.append(((rs.random_sample((n_out, n_in)) * 2 - 1) / np.sqrt(n_in)).astype(np.float32))
        out.append(((rs.random_sample(n_out) * 2 - 1) / np.sqrt(n_in)).astype(np.float32))
    out[5][:4] += np.array([-0.15, -0.05, 0.05, 0.15], np.float32)
    if mode == SAC:
        out[5][4:] -= np.float32(0.5)
    return out


def explore(mode, head, z, limit, log_std, real):
    """the exploration action in precision `real` from the actor's output rows `head` [N, 4 or 8] and the variates z [N, 4]"""
    limit = real(limit)
    if mode == DDPG:
        sig = np.exp(np.asarray(log_std, np.float32).astype(real))
        return np.clip(limit * np.tanh(head) + sig * z, -limit, limit).astype(real)
    mu, ls = head[:, :4], np.clip(head[:, 4:], real(-20), real(2))
    return (limit * np.tanh(mu + np.exp(ls) * z)).astype(real)


def collect_reference(task, env_kwargs, actor, activation, mode, N, launches, limit, env_seed, noise_seed, first_call, act_limit,
                      log_std, capacity, ptr, precision, fill=0.0):
    """sum(launches) closed-loop vector steps from a fresh reset, cut into consecutive launches (the running return and length,
    the observation and the call index carry over; each launch has a statistics slab of its own).  -> dict of float64 / bool
    arrays:
        oa [capacity, D + 4], obs2 [capacity, D], rew, done [capacity]   the ring (rows no step reached keep `fill`)
        a_bar [capacity, 4]      per element: the elementwise float32 bar of the exploration rule at this row (see below)
        obs [N, D]               o(K)
        ep_ret, ep_len [N]       the running sums after the last step
        slabs                    per launch [tiles, 8]
        fin, term, trunc [K, N]  per step: finished (terminated | truncated), and the two flags
        ep_len_at [launches + 1, N]   the running length in front of each launch and behind the last
        ptr, size                the ring position and fill count afterwards
    precision "f64": everything in float64, the action rounded to float32 where the device hands it to the env; "f32": oracle,
    network, exploration rule and running sums in float32 (z is drawn in float64 and rounded: the contract's variates).

    a_bar: what the project already holds the two rules to elementwise, against float64 at the device's own variates --
    DDPG 1e-6 absolute (test_ddpg_explore_against_float64), SAC 2^-22 (limit + limit (|mu| + sigma |z|)) (_check_sample,
    tests/test_gpu_sac_kernels.py)."""
    real = np.float64 if precision == "f64" else np.float32
    W1, b1, W2, b2, W3, b3 = (np.asarray(w, np.float32).astype(real) for w in actor)
    act = {"relu": lambda x: np.maximum(x, real(0)), "tanh": np.tanh}[activation]
    K = int(sum(launches))
    tiles = (N + TILE - 1) // TILE
    assert capacity % N == 0 and ptr % N == 0 and 0 <= ptr < capacity
    env = oracle.OracleBatch(task, N, precision=precision, max_episode_steps=int(limit), **eo.oracle_kwargs(env_kwargs))
    D = env.obs_dim
    assert W1.shape[1] == D and W3.shape[0] == (8 if mode == SAC else 4)
    oa, obs2 = np.full((capacity, D + 4), fill, np.float64), np.full((capacity, D), fill, np.float64)
    rew, done, a_bar = np.full(capacity, fill, np.float64), np.full(capacity, fill, np.float64), np.zeros((capacity, 4))
    fin, term, trunc = np.zeros((K, N), bool), np.zeros((K, N), bool), np.zeros((K, N), bool)
    ep_ret, ep_len = np.zeros(N, real), np.zeros(N, real)
    ep_len_at, slabs = [ep_len.astype(np.float64)], []
    size = 0
    o = np.array(env.reset(env_seed, 0), real)
    s = 0
    for k in launches:
        slab = np.tile(np.asarray(NEUTRAL, real), (tiles, 1))
        for _ in range(k):
            h = act(o @ W1.T + b1)
            h = act(h @ W2.T + b2)
            head = h @ W3.T + b3
            assert head.dtype == real
            z = so.normals64(N, 4, noise_seed, first_call + s).astype(real)
            a = explore(mode, head, z, act_limit, log_std, real).astype(np.float32)
            o_next, r, te, tr, _ = env.step(a, seed=env_seed, tick=1 + s, auto_reset=True)
            o_next, r, te, tr = np.array(o_next, real), np.array(r, real), te.astype(bool), tr.astype(bool)
            over = te | tr
            rows = slice(ptr, ptr + N)
            oa[rows, :D], oa[rows, D:] = o, a
            obs2[rows] = np.where(over[:, None], np.array(env.final_obs, real), o_next)
            rew[rows] = r
            done[rows] = (te & ~tr).astype(np.float64)
            if mode == DDPG:
                a_bar[rows] = 1e-6
            else:
                u_abs = np.abs(head[:, :4]) + np.exp(np.clip(head[:, 4:], -20, 2)) * np.abs(z)
                a_bar[rows] = 2.0 ** -22 * (act_limit + act_limit * u_abs.astype(np.float64))
            fin[s], term[s], trunc[s] = over, te, tr
            # ep_ret += r; ep_len += 1; the log where the episode is over; then zero
            ep_ret = (ep_ret + r).astype(real)
            ep_len = (ep_len + real(1)).astype(real)
            for t in range(tiles):
                m = over[t * TILE:(t + 1) * TILE]
                if m.any():
                    rt, ln = ep_ret[t * TILE:(t + 1) * TILE][m], ep_len[t * TILE:(t + 1) * TILE][m]
                    q = slab[t]
                    q[0] += real(m.sum()); q[1] += rt.sum(dtype=real); q[2] += (rt * rt).sum(dtype=real)
                    q[3], q[4] = min(q[3], rt.min()), max(q[4], rt.max())
                    q[5] += ln.sum(dtype=real); q[6], q[7] = min(q[6], ln.min()), max(q[7], ln.max())
            ep_ret = np.where(over, real(0), ep_ret).astype(real)
            ep_len = np.where(over, real(0), ep_len).astype(real)
            o = o_next
            ptr = (ptr + N) % capacity
            size = min(size + N, capacity)
            s += 1
        slabs.append(slab.astype(np.float64))
        ep_len_at.append(ep_len.astype(np.float64))
    return dict(oa=oa, obs2=obs2, rew=rew, done=done, a_bar=a_bar, obs=o.astype(np.float64), ep_ret=ep_ret.astype(np.float64),
                ep_len=ep_len.astype(np.float64), slabs=slabs, fin=fin, term=term, trunc=trunc, ep_len_at=np.stack(ep_len_at),
                ptr=ptr, size=size)


# ---- the cases of tests/test_collect_oracle_cpu.py and tests/test_gpu_collect_reference.py ---------------------------------------
class Case:
    """one collection: env id + kwargs, an actor as plain arrays, the launches' sizes and scalar arguments"""

    def __init__(self, name, env_id, kwargs, mode, N=128, launches=(16,), limit=12, hidden=(32, 48), activation="tanh",
                 act_limit=1.0, log_std=LOG_STD, blocks=None, ptr_block=0, env_seed=11, actor_seed=1, noise_seed=NOISE_SEED,
                 first_call=FIRST_CALL, fill=0.0):
        self.name, self.env_id, self.kwargs, self.mode = name, env_id, dict(kwargs), mode
        self.N, self.launches, self.limit, self.activation = N, tuple(launches), limit, activation
        self.K = sum(self.launches)
        self.D = eo._obs_dim(env_id, kwargs)
        self.hidden = tuple(hidden)
        self.actor = random_actor(self.D, hidden[0], hidden[1], mode, actor_seed)
        self.act_limit, self.log_std = float(act_limit), tuple(log_std)
        self.capacity, self.ptr = (blocks or self.K) * N, ptr_block * N
        self.env_seed, self.noise_seed, self.first_call, self.fill = env_seed, noise_seed, first_call, fill
        self.task = eo.TASK_OF[env_id]
        self.terminates = env_id == HOVER  # under these limits Circle stays in its tube; TakeOff never sets `done`
        self._memo = {}

    @property
    def tiles(self):
        return (self.N + TILE - 1) // TILE

    def block(self, s):
        """first ring row of step s"""
        return (self.ptr + s * self.N) % self.capacity

    def survives(self, s):
        """whether the ring block of step s is still there after the last step"""
        return self.K - s <= self.capacity // self.N

    def reference(self, precision):
        """collect_reference's dict, computed once per precision and handed out read-only"""
        if precision not in self._memo:
            out = collect_reference(self.task, self.kwargs, self.actor, self.activation, self.mode, self.N, self.launches,
                                    self.limit, self.env_seed, self.noise_seed, self.first_call, self.act_limit, self.log_std,
                                    self.capacity, self.ptr, precision, self.fill)
            for x in list(out.values()) + out["slabs"]:
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
            self._memo[precision] = out
        return self._memo[precision]


_VARIANT_ENVS = {
    "hover_lean": (HOVER, LEAN),
    "hover_full": (HOVER, {}),
    "hover_full_motor": (HOVER, MOTOR),
    "circle_lean_motor": (CIRCLE, dict(LEAN, **MOTOR)),
    "takeoff_full": (TAKEOFF, {}),
}


def _builders():
    b = {}
    for mode, mn in MODE_NAME.items():
        # N = 128 (two tiles), K = 16 over a limit of 12
        for env, (env_id, kw) in _VARIANT_ENVS.items():
            b[f"{env}-{mn}"] = lambda env=env, env_id=env_id, kw=kw, mode=mode, mn=mn: Case(f"{env}-{mn}", env_id, kw, mode)
        b[f"hover_full-limit0.5-{mn}"] = lambda mode=mode, mn=mn: Case(f"hover_full-limit0.5-{mn}", HOVER, {}, mode, act_limit=0.5)
        # N = 67: one full tile whose blocks of odd s start 8 bytes off a 16-byte boundary, and a tile of 3 rows
        b[f"hover_lean-N67-{mn}"] = lambda mode=mode, mn=mn: Case(f"hover_lean-N67-{mn}", HOVER, LEAN, mode, N=67, launches=(5,), limit=4)
        b[f"hover_full-N67-limit0.5-{mn}"] = lambda mode=mode, mn=mn: Case(f"hover_full-N67-limit0.5-{mn}", HOVER, {}, mode, N=67,
                                                                          launches=(5,), limit=4, act_limit=0.5, env_seed=15,
                                                                          actor_seed=2)  # (seeds with terminations in 4 steps)
        # two launches on one env and one ring: the second starts in the middle of the episodes
        b[f"hover_full-two_launches-{mn}"] = lambda mode=mode, mn=mn: Case(f"hover_full-two_launches-{mn}", HOVER, {}, mode,
                                                                          launches=(5, 7), limit=8)
        # the ring: capacity 4 N entered at 3 N (blocks 3 N, 0, N; block 2 N keeps the fill), and capacity N (every step on
        # the same block: the last one stays).  A limit of 2: the TimeLimit falls inside the three steps.
        b[f"hover_lean-wrap-{mn}"] = lambda mode=mode, mn=mn: Case(f"hover_lean-wrap-{mn}", HOVER, LEAN, mode, launches=(3,), limit=2,
                                                                  blocks=4, ptr_block=3, fill=-7.5)
        b[f"hover_lean-capacity_N-{mn}"] = lambda mode=mode, mn=mn: Case(f"hover_lean-capacity_N-{mn}", HOVER, LEAN, mode,
                                                                        launches=(3,), limit=2, blocks=1, fill=-7.5)
    return b


_BUILDERS = _builders()
CASES = list(_BUILDERS)
case = eo._table(_BUILDERS)


# ---- the comparison rule, one statement for the CPU and the GPU test ---------------------------------------------------------
BAR_UNITS = 4.0          # the project's margin for a device path against float64 (test_losses_against_the_reference)
SLAB_RTOL = 1e-5         # return sum and sum of squares of a tile (tests/test_gpu_collect.py)
FLOAT_ARRAYS = ("oa_obs", "oa_act", "obs2", "rew", "obs_out", "ep_ret", "slab_ret_minmax")


def derived_fin(c, got):
    """-> (fin [K, N] bool, known [K] bool): the finished flags as the ring shows them -- the stored o' of step s differs from
    the o of step s + 1 (the last step: from o(K)) exactly where the env finished and the next row is a reset one.  A step is
    known when its block and its successor's are still in the ring."""
    D, N = c.D, c.N
    fin, known = np.zeros((c.K, N), bool), np.zeros(c.K, bool)
    for s in range(c.K):
        if not c.survives(s):
            continue
        b = c.block(s)
        nxt = got["obs"] if s == c.K - 1 else got["oa"][c.block(s + 1):c.block(s + 1) + N, :D]
        fin[s] = (got["obs2"][b:b + N] != nxt).any(axis=1)
        known[s] = True
    return fin, known


def agreement(c, got, ref):
    """-> agree [N] bool: the envs whose `done` column and finished flags equal the reference's at every step the ring still
    shows.  `got` has the keys of collect_reference's dict that a device path produces (oa, obs2, rew, done, obs, ...)."""
    N = c.N
    fin, known = derived_fin(c, got)
    agree = np.ones(N, bool)
    for s in range(c.K):
        if known[s]:
            agree &= fin[s] == ref["fin"][s]
        if c.survives(s):
            b = c.block(s)
            agree &= got["done"][b:b + N] == ref["done"][b:b + N]
    return agree


def _row_mask(c, agree):
    """ring rows that are compared: the surviving blocks' rows of the agreeing envs (other rows must hold the fill)"""
    m = np.zeros(c.capacity, bool)
    for s in range(c.K):
        if c.survives(s):
            m[c.block(s):c.block(s) + c.N] = agree
    return m


def float_views(c, d, rows, agree, tiles_ok):
    """the float arrays of the rule as flat vectors over what is compared"""
    slab = np.concatenate([s[tiles_ok][:, 3:5].reshape(-1) for s in d["slabs"]])
    return dict(oa_obs=d["oa"][rows, :c.D], oa_act=d["oa"][rows, c.D:], obs2=d["obs2"][rows], rew=d["rew"][rows],
                obs_out=d["obs"][agree], ep_ret=d["ep_ret"][agree], slab_ret_minmax=slab[np.isfinite(slab)])


def units_of(c):
    """-> (units {array: float}, agree [N], distances {array: float}): per float array the float32 reference's max distance from
    the float64 reference over the envs on which the two agree, floored at one float32 rounding of the array's largest entry
    (the float32 run carries its running sums in float32: the measured distance holds their rounding)"""
    r32, r64 = c.reference("f32"), c.reference("f64")
    agree = agreement(c, r32, r64)
    rows, tiles_ok = _row_mask(c, agree), tiles_compared(c, agree)
    v32, v64 = float_views(c, r32, rows, agree, tiles_ok), float_views(c, r64, rows, agree, tiles_ok)
    units, dist = {}, {}
    for k in FLOAT_ARRAYS:
        dist[k] = float(np.abs(v32[k] - v64[k]).max()) if v64[k].size else 0.0
        top = float(np.abs(v64[k]).max()) if v64[k].size else 0.0
        units[k] = max(dist[k], 2.0 ** -24 * top)
    return units, agree, dist


def tiles_compared(c, agree):
    """tiles without an excluded env"""
    pad = np.ones(c.tiles * TILE, bool)
    pad[:c.N] = agree
    return pad.reshape(c.tiles, TILE).all(axis=1)


def check(c, got, path, record=None):
    """the rule for one device result `got` (float64 / bool numpy arrays: oa, obs2, rew, done, obs, ep_ret, ep_len, slabs (list),
    ptr, size) against the float64 reference -> {array: ratio}.  Prints one MARGIN line per float array."""
    ref = c.reference("f64")
    units, _, _ = units_of(c)
    agree = agreement(c, got, ref)
    excluded = int((~agree).sum())
    print(f"EXCLUDED {c.name} {path} {excluded} of {c.N} (cap {eo.length_cap(c.N)}): envs {np.flatnonzero(~agree)[:8].tolist()}")
    assert excluded <= eo.length_cap(c.N), (c.name, path, excluded, np.flatnonzero(~agree)[:8].tolist())
    rows, tiles_ok = _row_mask(c, agree), tiles_compared(c, agree)
    # ---- exact (done and the finished flags ARE the agreement: what binds them is the cap above) ----
    assert (got["ptr"], got["size"]) == (ref["ptr"], ref["size"]), (c.name, path, got["ptr"], got["size"])
    assert np.array_equal(got["ep_len"][agree], ref["ep_len"][agree]), (c.name, path)
    untouched = np.ones(c.capacity, bool)
    for s in range(c.K):
        untouched[c.block(s):c.block(s) + c.N] = False
    for k in ("oa", "obs2", "rew", "done"):
        assert (got[k][untouched] == c.fill).all(), (c.name, path, k)
    assert len(got["slabs"]) == len(ref["slabs"])
    for j, (g, r) in enumerate(zip(got["slabs"], ref["slabs"])):
        assert g.shape == r.shape == (c.tiles, STATS)
        for col in (0, 5, 6, 7):
            assert np.array_equal(g[tiles_ok, col], r[tiles_ok, col]), (c.name, path, "slab", j, col, g[:, col], r[:, col])
        for col in (1, 2):
            assert (np.abs(g[tiles_ok, col] - r[tiles_ok, col]) <= SLAB_RTOL * np.abs(r[tiles_ok, col])).all(), (c.name, path, "slab", j, col)
        inf = ~np.isfinite(r[:, 3:5])
        assert np.array_equal(g[:, 3:5][inf & tiles_ok[:, None]], r[:, 3:5][inf & tiles_ok[:, None]])
    # ---- float ----
    vg, vr = float_views(c, got, rows, agree, tiles_ok), float_views(c, ref, rows, agree, tiles_ok)
    ratios = {}
    for k in FLOAT_ARRAYS:
        assert vg[k].shape == vr[k].shape, (c.name, path, k)
        err = np.abs(vg[k] - vr[k])
        tol = np.full(err.shape, BAR_UNITS * units[k])
        if k == "oa_act":  # the elementwise bar of the exploration rule is a floor of the tolerance
            tol = np.maximum(tol, ref["a_bar"][rows])
        ratios[k] = float((err / (tol / BAR_UNITS)).max()) if err.size else 0.0
        print(f"MARGIN {c.name} {path} {k} unit={units[k]:.3e} err={float(err.max()) if err.size else 0.0:.3e} "
              f"ratio={ratios[k]:.3f} excluded={excluded}")
        if record is not None:
            record(f"ratio_{path}_{k}", ratios[k])
    for k in FLOAT_ARRAYS:
        assert ratios[k] <= BAR_UNITS, (c.name, path, k, ratios[k], units[k])
    return ratios
