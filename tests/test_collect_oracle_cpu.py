"""tests/collect_oracle.py pinned on the CPU: for every case tests/test_gpu_collect_reference.py flies, the float32 run of the
restated collection loop (float32 oracle, float32 network and exploration rule, float32 running sums -- the arithmetic of the
kernel) against its float64 run.  The distance between the two, per array, is the UNIT of the GPU test's bar; here it is printed
per case, and the conditions the GPU test relies on are asserted on the reference alone: exclusions inside the cap, `done` and
the finished flags identical on the agreeing envs, the endings each task is to show, a second launch that starts in the middle of
episodes, a finished episode in every compared tile."""
import numpy as np
import pytest

import collect_oracle as co
import evaluate_oracle as eo
import sampler_oracle as so


@pytest.mark.parametrize("name", co.CASES)
def test_float32_reference_against_float64_reference(name):
    c = co.case(name)
    r32, r64 = c.reference("f32"), c.reference("f64")
    units, agree, dist = co.units_of(c)
    excluded = int((~agree).sum())
    n_term, n_trunc = int((r64["term"] & ~r64["trunc"]).sum()), int(r64["trunc"].sum())
    tops = {k: float(np.abs(v).max()) if v.size else 0.0
            for k, v in co.float_views(c, r64, co._row_mask(c, agree), agree, co.tiles_compared(c, agree)).items()}
    print(f"{name}: N = {c.N}, K = {c.K}, {excluded} envs excluded (cap {eo.length_cap(c.N)}); {n_term} terminated, {n_trunc} truncated "
          f"transitions; " + "; ".join(f"{k} dist {dist[k]:.3e} unit {units[k]:.3e} max {tops[k]:.3g}" for k in co.FLOAT_ARRAYS))
    assert excluded <= eo.length_cap(c.N)
    # `done` and the finished flags, over ALL steps (not only those the ring still shows), on the agreeing envs
    assert np.array_equal(r32["fin"][:, agree], r64["fin"][:, agree])
    assert np.array_equal(r32["term"][:, agree], r64["term"][:, agree]) and np.array_equal(r32["trunc"][:, agree], r64["trunc"][:, agree])
    rows = co._row_mask(c, agree)
    assert np.array_equal(r32["done"][rows], r64["done"][rows])
    assert np.array_equal(r32["ep_len"][agree], r64["ep_len"][agree])
    for r in (r32, r64):
        # the ring shows the flags: what derived_fin reads off obs2 and the next o is what the loop saw
        fin, known = co.derived_fin(c, r)
        assert known.sum() == min(c.K, c.capacity // c.N) and np.array_equal(fin[known], r["fin"][known])
        assert np.isfinite(r["oa"]).all() and np.isfinite(r["obs2"]).all() and np.isfinite(r["rew"]).all()
        assert np.abs(r["oa"][rows, c.D:]).max() <= c.act_limit
        assert (r["ptr"], r["size"]) == ((c.ptr + c.K * c.N) % c.capacity, min(c.K * c.N, c.capacity))
    # the endings
    assert n_trunc >= 1
    if c.terminates:
        assert n_term >= 1
        # ... and a transition that is terminated AND truncated (the drone tumbles in the step that reaches the TimeLimit): its
        # `done` is 0, so a `done` without `& ~truncated` differs
        assert int((r64["term"] & r64["trunc"]).sum()) >= 1
    else:
        assert n_term == 0 and not r64["term"].any()
    # done = 1 exactly at the terminated-and-not-truncated rows that are still in the ring
    for s in range(c.K):
        if c.survives(s):
            assert np.array_equal(r64["done"][c.block(s):c.block(s) + c.N], (r64["term"][s] & ~r64["trunc"][s]).astype(np.float64))
    # a finished episode in every compared tile of every launch
    ok = co.tiles_compared(c, agree)
    for slab in r64["slabs"]:
        assert (slab[ok, 0] >= 1).all(), slab[:, 0]
    if len(c.launches) > 1:
        assert (r64["ep_len_at"][1] > 0).any() and (r64["ep_len_at"][1] == 0).any()


def test_the_case_table_is_what_the_gpu_test_is_to_fly():
    """five variants, act_limit 0.5, two odd-N cases, two launches and the two ring forms, each in both modes"""
    assert len(co.CASES) == 22
    for name in co.CASES:
        c = co.case(name)
        assert c.K <= 16 and c.N <= 128
        assert c.noise_seed >= 2 ** 32 and c.first_call == 2 ** 33 + 5 and len(set(c.log_std)) == 4
    c = co.case("hover_lean-N67-ddpg")
    assert (c.N * (c.D + 4) * 4) % 16 == 8 and (c.N * c.D * 4) % 16 == 8  # blocks of odd s are 8 bytes off
    c = co.case("hover_lean-wrap-sac")
    assert [c.block(s) for s in range(3)] == [3 * c.N, 0, c.N] and all(c.survives(s) for s in range(3))
    c = co.case("hover_lean-capacity_N-sac")
    assert [c.block(s) for s in range(3)] == [0, 0, 0] and [c.survives(s) for s in range(3)] == [False, False, True]


def test_the_loop_by_hand_env_by_env():
    """collect_reference's batched network, masked sums and tile accumulators against the same loop written env by env: one
    matrix-vector product per env and layer, a plain Python loop over the steps, the log as a list of (step, env, return,
    length) entries reduced per tile at the end.  Flags, lengths and counts are equal; floats agree to 1e-6 of their size: the
    two summation orders of a float64 dot product can round an action to neighbouring float32 values (6e-8 apart), and the env
    carries that on."""
    from oracle import oracle

    def close(x, y, scale=None):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return bool((np.abs(x - y) <= 1e-6 * np.maximum(1.0, np.abs(y) if scale is None else scale)).all())

    for name in ("hover_full-N67-limit0.5-ddpg", "hover_full-N67-limit0.5-sac"):
        c = co.case(name)
        assert c.task == "hover" and c.activation == "tanh" and len(c.launches) == 1  # what the loop below writes out
        ref = c.reference("f64")
        W1, b1, W2, b2, W3, b3 = (w.astype(np.float64) for w in c.actor)
        env = oracle.OracleBatch("hover", c.N, precision="f64", max_episode_steps=c.limit, **eo.oracle_kwargs(c.kwargs))
        o = env.reset(c.env_seed, 0).copy()
        ret, length, log = [0.0] * c.N, [0] * c.N, []
        sig = [float(np.exp(np.float32(v))) for v in c.log_std]
        for s in range(c.K):
            z = so.normals64(c.N, 4, c.noise_seed, c.first_call + s)
            a = np.zeros((c.N, 4), np.float32)
            for i in range(c.N):
                y = W3 @ np.tanh(W2 @ np.tanh(W1 @ o[i] + b1) + b2) + b3
                for j in range(4):
                    if c.mode == co.DDPG:
                        v = min(max(c.act_limit * np.tanh(y[j]) + sig[j] * z[i, j], -c.act_limit), c.act_limit)
                    else:
                        v = c.act_limit * np.tanh(y[j] + np.exp(min(max(y[4 + j], -20.0), 2.0)) * z[i, j])
                    a[i, j] = v
            o2, r, te, tr, _ = env.step(a, seed=c.env_seed, tick=1 + s, auto_reset=True)
            for i in range(c.N):
                row = c.block(s) + i
                assert close(ref["oa"][row], np.concatenate([o[i], a[i].astype(np.float64)])), (name, s, i)
                assert close(ref["obs2"][row], env.final_obs[i] if (te[i] or tr[i]) else o2[i]), (name, s, i)
                assert close(ref["rew"][row], r[i]) and ref["done"][row] == (1.0 if te[i] and not tr[i] else 0.0)
                assert ref["fin"][s, i] == bool(te[i] or tr[i])
                ret[i] += r[i]; length[i] += 1
                if te[i] or tr[i]:
                    log.append((s, i, ret[i], length[i]))
                    ret[i], length[i] = 0.0, 0
            o = o2.copy()
        assert close(ref["obs"], o) and np.array_equal(ref["ep_len"], np.array(length, np.float64))
        assert close(ref["ep_ret"], np.array(ret))
        assert len(log) >= c.N  # every env met the TimeLimit of 4 within the 5 steps
        for t in range(c.tiles):
            mine = [(rt, ln) for _, i, rt, ln in log if i // co.TILE == t]
            rets, lens = np.array([m[0] for m in mine]), np.array([m[1] for m in mine], np.float64)
            got = ref["slabs"][0][t]
            assert got[0] == len(mine) and got[5] == lens.sum() and got[6] == lens.min() and got[7] == lens.max()
            assert close(got[3], rets.min()) and close(got[4], rets.max())
            assert close(got[1], rets.sum(), np.abs(rets).sum()) and close(got[2], (rets * rets).sum(), (rets * rets).sum())
