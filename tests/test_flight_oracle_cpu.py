"""tests/flight_oracle.py pinned on the CPU, for every case tests/test_gpu_evaluate_forms_reference.py flies: its float32 run
against its float64 run per quantity group (the distance is the UNIT of the GPU test's bar, printed here), the integer metrics
equal inside the cap, the history stack against the reference's own trajectories (tests/golden/history.npz) and against a
flight written out env by env, and TEETH: on the float64 reference alone, each mistake a kernel or the composed path could make
-- x(s + 1) for x(s), the clipped action for the raw one in u, the noisy observation's rates for rpy_dot, two swapped column
groups, the alive mask one step late, the history restarting one step late -- moves the affected quantity by more than 100 bars
(a bar is BAR_UNITS = 4 units), so a device result inside the bar cannot hold it."""
import os

import numpy as np
import pytest

import evaluate_oracle as eo
import flight_oracle as fo

BAR_UNITS = 4.0
TEETH = 100 * BAR_UNITS
ALL = fo.FORM_CASES + [("history", n) for n in fo.HISTORY_CASES]
IDS = [f"{k}-{n}" for k, n in ALL]
_case = fo.form_case


def _noisy(case):
    return case.kwargs.get("observation_noise", 1) > 0


@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_float32_flight_against_float64_flight(kind, name):
    """the units, printed; lengths and integer metrics agree inside length_cap; the three sums of the flight are those of
    evaluate_oracle.evaluate_reference, a second statement of the same loop"""
    c = _case(kind, name)
    f32, f64 = fo.flight(c, "f32"), fo.flight(c, "f64")
    agree = fo.agreeing(c)
    excluded = int((~agree).sum())
    units = fo.units_of(c)
    print(f"{name}: N = {c.N}, T = {c.max_steps}, {excluded} envs excluded (cap {eo.length_cap(c.N)})")
    for k, v in units.items():
        print(f"UNIT {name} {k} {v:.3e}")
        assert np.isfinite(v) and v > 0, k
    assert excluded <= eo.length_cap(c.N)
    wrong = agree & (f32["metrics"][..., list(fo.EM_INTEGER)] != f64["metrics"][..., list(fo.EM_INTEGER)]).any(axis=-1)
    print(f"{name}: integer metrics differ on {int(wrong.sum())} agreeing envs (cap {eo.length_cap(c.N)}): "
          f"{[int((agree & (f32['metrics'][..., j] != f64['metrics'][..., j])).sum()) for j in fo.EM_INTEGER]}")
    assert int(wrong.sum()) <= eo.length_cap(c.N)
    if kind != "history":  # (a HistoryCase's reference() IS its flight)
        for prec, fl in (("f32", f32), ("f64", f64)):
            r, l, co = eo.Case.reference(c, prec)
            assert np.array_equal(r, fl["ret"]) and np.array_equal(l, fl["length"]) and np.array_equal(co, fl["cost"])
    L = f64["length"].astype(int)
    T = c.max_steps
    assert f64["state"].shape == (c.P, c.E, T, 12) and f64["observation"].shape == (c.P, c.E, T, c.shape[0])
    past = np.arange(T)[None, None, :] >= L[:, :, None]
    for k in ("state", "action", "observation"):
        assert not f64[k][past].any()
    # the counters are bounded by the episode
    m = f64["metrics"]
    assert (m[..., 5] <= L).all() and (m[..., 6] <= L - 1).all() and (m[..., 7] <= L - 1).all() and (m[..., :5] >= 0).all()


@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_u_is_the_raw_action_of_the_step_before(kind, name):
    """the oracle's last_action in front of step s >= 1 of an episode is the raw float32 action a(s - 1), also where it saturates
    and under the latency ring; u0 lies in [-1, 1] (the reset's own action is clipped: envs/hover.py:223-229)"""
    c = _case(kind, name)
    f64 = fo.flight(c, "f64")
    done = f64["done_all"].T.reshape(c.P, c.E, -1)
    same_episode = ~done[:, :, :-1]
    assert np.array_equal(f64["u_all"][:, :, 1:][same_episode], f64["action_all"][:, :, :-1][same_episode])
    assert np.abs(f64["u0"]).max() <= 1.0
    assert np.array_equal(f64["u0"], f64["u_all"][:, :, 0])


def _recorded(case, fl):
    """[P, E, T] bool: the recorded steps s < length"""
    return np.arange(case.max_steps)[None, None, :] < fl["length"].astype(int)[:, :, None]


@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_teeth_of_the_record(kind, name):
    """x(s + 1) for x(s), and two swapped column groups, in every group of the state; a(s + 1) for a(s); o(s + 1) for o(s)"""
    c = _case(kind, name)
    f64, units = fo.flight(c, "f64"), fo.units_of(c)
    on = _recorded(c, f64)
    both = on[:, :, 1:]  # s and s + 1 both recorded
    for g, sl in fo.GROUPS.items():
        x = f64["state"][..., sl]
        moved = float(np.abs(x[:, :, 1:] - x[:, :, :-1])[both].max())
        print(f"TEETH {name} x(s+1) {g} moved {moved:.3e} = {moved / (BAR_UNITS * units[g]):.0f} bars")
        assert moved > TEETH * units[g], (g, moved, units[g])
    for k in ("action", "observation"):
        x = f64[k]
        moved = float(np.abs(x[:, :, 1:] - x[:, :, :-1])[both].max())
        assert moved > TEETH * units[k], (k, moved, units[k])
    for a, b in (("position", "velocity"), ("attitude", "body_rates"), ("velocity", "attitude")):
        d = float(np.abs(f64["state"][..., fo.GROUPS[a]] - f64["state"][..., fo.GROUPS[b]])[on].max())
        print(f"TEETH {name} swapped {a} / {b}: {d:.3e}")
        assert d > TEETH * max(units[a], units[b]), (a, b, d)


@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_teeth_of_the_metrics_and_the_sums(kind, name):
    """the clipped action for the raw one in u (action_rate_sq); the noisy observation's rates for rpy_dot (rate_sq and the
    body rates; only where the observation is noisy -- without noise the observation's rates ARE rpy_dot, there is no such
    mistake to make); x(s + 1) for x(s) and the alive mask one step late (every metric sum, tilt_max, the part sums)"""
    c = _case(kind, name)
    f64, units = fo.flight(c, "f64"), fo.units_of(c)
    N, T = c.N, c.max_steps
    flat = lambda k: f64[k].reshape((N,) + f64[k].shape[2:])
    L = flat("length").astype(int)
    st, a, u, m = flat("state_all"), flat("action_all"), flat("u_all"), flat("metrics")
    rpy, omega = st[:, :, 6:9], st[:, :, 9:12]
    again = fo.metrics_of(rpy, omega, a, u, L, np.float64)
    assert np.array_equal(again, m)

    def moved(other, j):
        return float(np.abs(other[:, j] - m[:, j]).max())

    clipped = fo.metrics_of(rpy, omega, a, np.clip(u, -1.0, 1.0), L, np.float64)
    print(f"TEETH {name} clipped u: action_rate_sq moved {moved(clipped, 3):.3e} = {moved(clipped, 3) / (BAR_UNITS * units['action_rate_sq']):.0f} bars")
    assert moved(clipped, 3) > TEETH * units["action_rate_sq"]
    if _noisy(c):
        half = c.shape[0] // f64["history"]
        seen = flat("observation_all")[:, :, -half:][:, :, 10:13]  # the newest half: xyz 0:3, quat 3:7, velocity 7:10, rates 10:13
        noisy = fo.metrics_of(rpy, seen, a, u, L, np.float64)
        d = float(np.abs(seen - omega)[_recorded(c, f64).reshape(N, T)].max())
        print(f"TEETH {name} noisy rates: rate_sq moved {moved(noisy, 2):.3e}, the rates {d:.3e}")
        assert moved(noisy, 2) > TEETH * units["rate_sq"] and d > TEETH * units["body_rates"]
    # x(s + 1) for x(s): the state one step on (the last column repeated: an env at its last step has no next)
    nxt = np.concatenate([st[:, 1:], st[:, -1:]], axis=1)
    shifted = fo.metrics_of(nxt[:, :, 6:9], nxt[:, :, 9:12], a, u, L, np.float64)
    late = fo.metrics_of(rpy, omega, a, u, np.minimum(L + 1, T), np.float64)
    bars = lambda other, j: moved(other, j) / (BAR_UNITS * units[fo.EM[j]])
    for j in (0, 1, 2, 4):
        print(f"TEETH {name} x(s+1): {fo.EM[j]} moved {moved(shifted, j):.3e} = {bars(shifted, j):.0f} bars")
        # (tilt_max is printed only: a maximum that is reached late in the flight is the same one step on; it reads the roll and
        # pitch that roll_sq and pitch_sq read)
        assert j == 4 or bars(shifted, j) > 100, fo.EM[j]
    if not c.terminates:
        return  # (every episode runs to max_steps, where the flight ends: there is no step for a late mask to add)
    # the alive mask one step late adds the row behind the episode -- the reset's state and observation, u = the last action:
    # the observation sums (the affected quantity of the stats form) and the metric it moves most
    print(f"TEETH {name} late mask: the metrics moved {[round(bars(late, j)) for j in (0, 1, 2, 3, 4)]} bars")
    assert max(bars(late, j) for j in (0, 1, 2, 3)) > 100
    obs = flat("observation_all")
    s1, s2 = fo.obs_sums_of(obs, f64["shift"], L, np.float64)
    assert np.array_equal(s1, flat("sum_d")) and np.array_equal(s2, flat("sum_d2"))
    l1, l2 = fo.obs_sums_of(obs, f64["shift"], np.minimum(L + 1, T), np.float64)
    shown = []
    for k, x, y in (("part_sum_d", l1, s1), ("part_sum_d2", l2, s2)):
        d = float(np.abs(fo.part_sums(x) - fo.part_sums(y)).max())
        print(f"TEETH {name} late mask: {k} moved {d:.3e} = {d / (BAR_UNITS * units[k]):.0f} bars")
        shown.append(d / (BAR_UNITS * units[k]))
    assert max(shown) > 100, shown  # (one row too many is in both sums: the one that shows it fails the launch)


# ---- the history stack ---------------------------------------------------------------------------------------------------------
GOLDEN = [("hover", 1), ("hover", 4), ("circle", 4), ("circle", 6), ("takeoff", 8), ("hover", 2)]


@pytest.mark.parametrize("task,H", GOLDEN, ids=[f"{t}_h{h}" for t, h in GOLDEN])
def test_history_stack_against_the_reference_trajectories(task, H):
    """the six float64 trajectories of the reference env with observation_history_size = H (tests/golden/history.npz: reset,
    recorded actions, a reset() behind every termination -- the file holds terminations only, no truncation) against
    flight_oracle's stack rule on the float64 oracle's H = 2 row, at the default limit of 500.  The bar: 8 float64 roundings of
    the trajectory's largest value -- the oracle restates the reference's arithmetic in the same precision and order
    (tests/test_oracle_golden.py holds its own rows to 1e-12 relative); rewards, costs and flags come from the oracle's step."""
    from oracle import oracle
    g = np.load(os.path.join(eo.GOLD, "history.npz"))
    k = f"{task}_h{H}_"
    assert not g[k + "truncated"].any()
    env = oracle.OracleEnv(task, "f64", observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0.0, enable_reset_distribution=0)
    stack = fo.stack_reset(env.reset()[None, :], H)
    bar = 8 * 2.0 ** -52 * max(float(np.abs(g[k + "obs"]).max()), 1.0)
    assert stack.shape[1] == g[k + "obs0"].shape[0]
    worst = float(np.abs(stack[0] - g[k + "obs0"]).max())
    resets = 0
    for t in range(g[k + "actions"].shape[0]):
        row, r, term, trunc, cost = env.step(g[k + "actions"][t])
        assert term == bool(g[k + "terminated"][t]) and not trunc and cost == g[k + "cost"][t], t
        stack = fo.stack_advance(stack, row[None, :], np.zeros(1, bool), H)
        worst = max(worst, float(np.abs(stack[0] - g[k + "obs"][t]).max()), abs(r - g[k + "reward"][t]))
        if term:
            resets += 1
            stack = fo.stack_reset(env.reset()[None, :], H)
            worst = max(worst, float(np.abs(stack[0] - g[k + "reset_obs"][t]).max()))
    print(f"{task} H = {H}: max distance {worst:.3e}, bar {bar:.3e}, {resets} restarts")
    assert resets == int(g[k + "terminated"].sum())
    assert worst <= bar, (worst, bar)


def test_a_history_flight_by_hand_with_truncations():
    """flight_oracle.fly with a history against the same flight written env by env: per env a Python list of halves for the
    history, one matrix-vector product per layer, a per-step log, and a plain loop that adds up to and including the env's first
    finished step.  Hover lean, H = 3, limit 6 under 15 steps: envs are truncated (and some terminate), their history restarts
    from the reset row, and the flight goes on into second and third episodes.  (The two networks round differently -- einsum
    against matrix-vector products -- so a float32 action may differ in its last bit: 1e-9, not equality.)"""
    from oracle import oracle
    c = fo.HistoryCase("by_hand_h3", eo.HOVER, eo.LEAN, 3, (17, 33), "tanh", 6, True, P=2, E=8, seed=5, rows_seed=7)
    c.max_steps = 15
    f64 = fo.flight(c, "f64")
    L = f64["length"].astype(int)
    assert (L == 6).any() and (L < 6).any()  # both endings
    d, h1, h2 = c.shape
    half = c.half
    W1, b1, W2, b2, W3, b3 = eo.split_rows(c.rows, d, h1, h2, np.float64)
    env = oracle.OracleBatch("hover", c.N, precision="f64", max_episode_steps=c.limit, **eo.oracle_kwargs(c.kwargs))
    row = env.reset(c.seed, 0).copy()
    hist = [[row[i, :half].copy(), row[i, :half].copy(), row[i, half:].copy()] for i in range(c.N)]
    log, seen, restarts, cuts = [], [], 0, 0
    for s in range(c.max_steps):
        a = np.zeros((c.N, 4), np.float32)
        seen.append(np.stack([np.concatenate(h) for h in hist]))
        for i in range(c.N):
            p = i // c.E
            x = (seen[-1][i] - c.mean[p].astype(np.float64)) / (c.std[p].astype(np.float64) + np.float64(c.eps))
            h = np.tanh(W1[p] @ x + b1[p])
            h = np.tanh(W2[p] @ h + b2[p])
            a[i] = (W3[p] @ h + b3[p]).astype(np.float32)
        o, r, te, tr, co = env.step(a, seed=c.seed, tick=1 + s, auto_reset=True)
        row = o.copy()
        log.append((r.copy(), co.copy(), (te | tr).astype(bool)))
        for i in range(c.N):
            if te[i] or tr[i]:  # the row is the reset's: the history starts again
                hist[i] = [row[i, :half].copy(), row[i, :half].copy(), row[i, half:].copy()]
                restarts += 1
                cuts += int(tr[i] and not te[i])
            else:
                hist[i] = hist[i][1:] + [row[i, half:].copy()]
    assert restarts >= 2 * c.N and cuts >= c.N  # every env was cut at 6 and at 12 at the latest
    seen = np.stack(seen, axis=1).reshape(c.P, c.E, c.max_steps, d)
    assert np.abs(seen - f64["observation_all"]).max() <= 1e-9
    for i in range(c.N):
        ret = cost = 0.0
        n = 0
        for r, co, done in log:
            ret += r[i]; cost += co[i]; n += 1
            if done[i]:
                break
        p, e = divmod(i, c.E)
        assert n == L[p, e] and cost == f64["cost"][p, e] and abs(ret - f64["ret"][p, e]) <= 1e-9 * max(1.0, abs(ret)), (i, n, ret, cost)
        assert np.abs(seen[p, e, :n] - f64["observation"][p, e, :n]).max() <= 1e-9 and not f64["observation"][p, e, n:].any()


@pytest.mark.parametrize("name", fo.HISTORY_CASES)
def test_teeth_of_the_history(name):
    """the stacks rebuilt from the oracle's rows are the flight's; restarted one step late they differ from them by more than
    100 bars of the observation -- in rows behind an env's first finish, which evaluate_population reports nothing of: the restart
    is pinned by the golden trajectories (terminations) and the flight by hand (truncations) above.  What the device CAN show
    wrongly inside a first episode is the shift: a stack that appends the FIRST half of the row, or shifts by a whole row."""
    c = fo.history_case(name)
    f64, units = fo.flight(c, "f64"), fo.units_of(c)
    H, N, T = c.history, c.N, c.max_steps
    assert c.shape[0] == fo.HISTORY_INPUTS[name] == H * c.half
    obs = f64["observation_all"].reshape(N, T, -1).transpose(1, 0, 2)
    right = fo.restack(f64["rows0"], f64["rows_all"], f64["done_all"], H)
    assert np.array_equal(right, obs)
    late = fo.restack(f64["rows0"], f64["rows_all"], f64["done_all"], H, late=True)
    d = float(np.abs(late - right).max())
    print(f"TEETH {name} late restart: the stack moved {d:.3e} = {d / (BAR_UNITS * units['observation']):.0f} bars")
    # (TakeOff never terminates and its limit is max_steps: nothing restarts inside the flight)
    assert d > TEETH * units["observation"] or not f64["done_all"][:-1].any()
    assert f64["done_all"][:-1].any() == c.terminates
    on = _recorded(c, f64).reshape(N, T).T
    assert not np.abs(late - right)[on].any()  # ... and nothing inside a first episode
    first_half = right.copy()
    first_half[1:, :, -c.half:] = f64["rows_all"][:-1, :, :c.half]
    d = float(np.abs(first_half - right)[on].max())
    print(f"TEETH {name} first half appended: {d:.3e} = {d / (BAR_UNITS * units['observation']):.0f} bars")
    assert d > TEETH * units["observation"]
    if c.terminates:
        L = f64["length"]
        assert (L < c.limit).any() and (L == c.limit).any()
