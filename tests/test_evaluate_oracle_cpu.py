"""tests/evaluate_oracle.py pinned on the CPU: for every case tests/test_gpu_evaluate_reference.py flies, the float32 run of the
reference loop (float32 oracle, float32 network, float32 running sums -- the arithmetic of the kernel) against its float64 run.
The distance between the two in the return is the UNIT of the GPU test's bar; here it is printed per case, and the properties
the GPU test relies on are asserted on the reference alone: lengths agree inside the cap, costs are equal where they do, the
population's rows differ visibly, both endings occur, some cost is nonzero."""
import numpy as np
import pytest

import evaluate_oracle as eo


def _case(kind, name):
    return {"reference": eo.reference_case, "edge": eo.edge_case, "shape": eo.shape_case}[kind](name)


ALL = [("reference", n) for n in eo.REFERENCE_CASES] + [("edge", n) for n in eo.EDGE_CASES] + [("shape", n) for n in eo.SHAPE_CASES]


@pytest.mark.parametrize("kind,name", ALL, ids=[f"{k}-{n}" for k, n in ALL])
def test_float32_reference_against_float64_reference(kind, name):
    c = _case(kind, name)
    r32, l32, c32 = c.reference("f32")
    r64, l64, c64 = c.reference("f64")
    unit, agree, top = eo.unit_of(c)
    excluded = int((~agree).sum())
    print(f"{name}: N = {c.N}, {excluded} envs excluded (cap {eo.length_cap(c.N)}); max |ret32 - ret64| = "
          f"{float(np.abs(r32 - r64)[agree].max()):.3e}, unit {unit:.3e}, max |ret| {top:.3f} (relative {unit / max(top, 1e-30):.2e}); "
          f"lengths {int(l64.min())} .. {int(l64.max())}, median {float(np.median(l64)):.0f}; cost sums up to {float(c64.max()):.0f}")
    assert r64.shape == l64.shape == c64.shape == (c.P, c.E)
    assert excluded <= eo.length_cap(c.N)
    assert np.array_equal(c32[agree], c64[agree])
    assert np.isfinite(r64).all() and l64.min() >= 1 and l64.max() <= min(c.max_steps, c.limit)
    if c.has_cost:
        assert (c64[agree] > 0).any()
    else:
        assert not c64.any()


@pytest.mark.parametrize("name", eo.REFERENCE_CASES)
def test_reference_cases_have_teeth_and_both_endings(name):
    c = eo.reference_case(name)
    r64, l64, _ = c.reference("f64")
    unit, agree, _ = eo.unit_of(c)
    if c.terminates:
        assert (l64 < c.limit).any() and (l64 == c.limit).any()
        # a tile that staged another policy's row: the per-policy mean lengths of two policies differ by more than
        # the length cap could move a mean (cap envs x limit steps / E)
        spread = float(l64.mean(axis=1).max() - l64.mean(axis=1).min())
        assert spread > eo.length_cap(c.N) * c.limit / c.E, spread
    else:
        assert (l64 == c.limit).all()
    # ... and by more than the bar (4 units) could hide in the return
    rspread = float(r64.mean(axis=1).max() - r64.mean(axis=1).min())
    assert rspread > 100 * 4 * unit, (rspread, unit)


def test_edges_are_what_their_names_say():
    for env in ("hover_lean", "hover_default"):
        _, l, _ = eo.edge_case(f"{env}-max_steps_1").reference("f64")
        assert (l == 1).all()
        c = eo.edge_case(f"{env}-max_steps_7_limit_40")
        _, l, _ = c.reference("f64")
        assert (l == 7).any() and (l < 7).any()  # still flying at the last step flown / fallen before: nobody truncated at 40
        c = eo.edge_case(f"{env}-max_steps_40_limit_25")
        _, l, _ = c.reference("f64")
        assert l.max() == 25 and (l == 25).any() and (l < 25).any()
        c = eo.edge_case(f"{env}-one_tile_ends_by_step_3")
        _, l, _ = c.reference("f64")
        assert l[0].max() <= 3, l[0].max()          # tile 0 (policy 0, E = 64): every episode over by step 3
        assert (l[1:].max(axis=1) == c.limit).any()  # another tile flies to the limit


def test_the_loop_by_hand_on_one_env():
    """evaluate_reference's batched einsum network and masked sums against the same evaluation written env by env: one
    matrix-vector product per env and layer, a per-step log, and for each env a plain loop that adds up to and including its
    first finished step"""
    from oracle import oracle
    c = eo.shape_case("17x33-tanh")
    r64, l64, c64 = c.reference("f64")
    d, h1, h2 = c.shape
    W1, b1, W2, b2, W3, b3 = eo.split_rows(c.rows, d, h1, h2, np.float64)
    env = oracle.OracleBatch("hover", c.N, precision="f64", max_episode_steps=c.limit, **eo.oracle_kwargs(c.kwargs))
    obs = env.reset(c.seed, 0).copy()
    log = []
    for s in range(c.max_steps):
        a = np.zeros((c.N, 4), np.float32)
        for i in range(c.N):
            p = i // c.E
            h = np.tanh(W1[p] @ obs[i] + b1[p])
            h = np.tanh(W2[p] @ h + b2[p])
            a[i] = (W3[p] @ h + b3[p]).astype(np.float32)
        o, r, te, tr, co = env.step(a, seed=c.seed, tick=1 + s, auto_reset=True)
        obs = o.copy()
        log.append((r.copy(), co.copy(), (te | tr).astype(bool)))
    for i in range(c.N):
        ret = cost = 0.0
        n = 0
        for r, co, done in log:
            ret += r[i]; cost += co[i]; n += 1
            if done[i]:
                break
        p, e = divmod(i, c.E)
        assert n == l64[p, e] and cost == c64[p, e] and abs(ret - r64[p, e]) <= 1e-12 * max(1.0, abs(ret)), (i, n, ret, cost)
