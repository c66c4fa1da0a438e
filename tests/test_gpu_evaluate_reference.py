"""pds_evaluate_policies (csrc/pds_evaluate.h) and the composed path of evaluation.evaluate_population against an INDEPENDENT
reference: tests/evaluate_oracle.py -- the float64 CPU oracle behind a numpy float64 MLP, the evaluation loop restated from the
reference's text.  tests/test_gpu_evaluate.py compares the two device paths with each other; both were written together and could
be wrong together (the freeze at the first `terminated | truncated`, the step cost that arrives one iteration late, the trailing
`ep_cost +=`, the length as a float).  Here an off-by-one in `length` or one dropped last-step cost fails.

The rule (one statement, check() below):
  length  equal to the float64 reference, except for at most max(1, N // 1000) envs whose termination decision flipped on one
          rounding (the cap of test_lockstep_autoreset_vs_f32_oracle); they are counted and printed.
  cost    exactly equal on the agreeing envs; on Hover (the one task with a cost) some agreeing env has a nonzero sum.
  return  within 4 UNITS on the agreeing envs.  The unit is measured, not chosen: the float32 oracle's own max |ret32 - ret64| on
          the same case (tests/test_evaluate_oracle_cpu.py prints it), floored at the rounding of a float32 running sum,
          max_steps 2^-24 max |ret|.  4 is the margin of test_losses_against_the_reference (tests/test_gpu_simopt.py): the device's
          FMA contraction and its own sincos sit about as far from libm float32 as libm float32 sits from float64.
Each comparison prints `MARGIN <case> <path> unit=... ratio=... excluded=...`; profiles/evaluate_parity_margins.txt keeps a run."""
import numpy as np
import pytest
import torch

import evaluate_oracle as eo

pytestmark = pytest.mark.gpu
BAR_UNITS = 4.0


def _run(case, fused):
    """evaluate_population on a fresh env of the case -> ((ret, length, cost) CPU tensors, the env's tick afterwards)"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import PolicyPopulation, evaluate_population
    d, h1, h2 = case.shape
    pop = PolicyPopulation.from_flat(torch.from_numpy(case.rows.copy()), d, (h1, h2), case.activation,
                                     None if case.mean is None else torch.from_numpy(case.mean.copy()),
                                     None if case.std is None else torch.from_numpy(case.std.copy()), case.eps)
    env = pds.make(case.env_id, num_envs=case.N, seed=case.seed, max_episode_steps=case.limit, **case.kwargs)
    assert env.obs_dim == d
    out = evaluate_population(env, pop, fused=fused, max_steps=case.max_steps)
    tick = env.sync_tick()
    assert tick == env.tick == 1 + case.max_steps  # the reset + max_steps steps, wherever the tiles stopped
    env.close()
    return out, tick


def check(case, out, path):
    """the rule of the module docstring for one device result; -> (ratio, excluded)"""
    ret, length, cost = (x.numpy().astype(np.float64) for x in out)
    r64, l64, c64 = case.reference("f64")
    unit, _, _ = eo.unit_of(case)
    assert ret.shape == r64.shape == (case.P, case.E)
    agree = length == l64
    excluded = int((~agree).sum())
    err = float(np.abs(ret - r64)[agree].max())
    ratio = err / unit
    print(f"MARGIN {case.name} {path} unit={unit:.3e} err={err:.3e} ratio={ratio:.3f} excluded={excluded} of {case.N}")
    assert excluded <= eo.length_cap(case.N), (case.name, path, excluded, np.argwhere(~agree)[:8].tolist(),
                                               length[~agree][:8].tolist(), l64[~agree][:8].tolist())
    bad = agree & (cost != c64)
    assert not bad.any(), (case.name, path, int(bad.sum()), cost[bad][:8].tolist(), c64[bad][:8].tolist())
    if case.has_cost:
        assert (cost[agree] > 0).any()
    else:
        assert not cost.any()
    assert ratio <= BAR_UNITS, (case.name, path, err, unit, ratio)
    return ratio, excluded


def _both_paths(case, bitwise):
    from test_gpu_evaluate import _equal
    fused, tick_f = _run(case, True)
    composed, tick_c = _run(case, False)
    check(case, fused, "fused")
    check(case, composed, "composed")
    assert tick_f == tick_c
    if bitwise:
        assert _equal(fused, composed), [float((a - b).abs().max()) for a, b in zip(fused, composed)]
    return fused


@pytest.mark.parametrize("name", eo.REFERENCE_CASES)
def test_population_evaluation_against_the_float64_reference(name):
    """P = 8 policies x E = 128 episodes (two tiles per policy, 16 tiles), limit 40-60: the kernel and the composed path, each
    against the float64 reference.  The population has teeth -- on the reference's output the per-policy mean lengths of two
    policies differ by more than the excluded envs could move a mean, and the mean returns by more than 100 bars -- so a tile that
    staged another policy's row fails; where the task terminates the case holds both endings."""
    case = eo.reference_case(name)
    r64, l64, _ = case.reference("f64")
    unit, _, _ = eo.unit_of(case)
    per_policy = l64.mean(axis=1)
    if case.terminates:
        assert (l64 < case.limit).any() and (l64 == case.limit).any()
        assert per_policy.max() - per_policy.min() > eo.length_cap(case.N) * case.limit / case.E
    else:
        assert (l64 == case.limit).all()
    assert r64.mean(axis=1).max() - r64.mean(axis=1).min() > 100 * BAR_UNITS * unit
    fused = _both_paths(case, bitwise=True)
    length = fused[1].numpy()
    if case.terminates:
        assert (length < case.limit).any() and (length == case.limit).any()
    else:
        assert (length == case.limit).all()


@pytest.mark.parametrize("name", eo.EDGE_CASES)
def test_edges_against_the_reference_and_bitwise_against_composed(name):
    """P = 4, E = 64 on Hover lean and Hover at the reference's defaults: max_steps = 1; max_steps = 7 under a limit of 40 (nobody
    is truncated, an env still flying has length 7 and its seventh step's cost -- the one that is still on its way back from the
    sink row when the loop ends); max_steps = 40 over a limit of 25 (the sums freeze at or before 25, the env flies on into its
    next episode); one tile whose 64 episodes all end by step 3 next to tiles that fly to the limit."""
    case = eo.edge_case(name)
    fused = _both_paths(case, bitwise=True)
    length, cost = fused[1].numpy(), fused[2].numpy()
    edge = name.split("-", 1)[1]
    if edge == "max_steps_1":
        assert (length == 1).all() and set(np.unique(cost)) <= {0.0, 1.0}
    elif edge == "max_steps_7_limit_40":
        flying = length == 7
        assert flying.any() and (length < 7).any() and length.max() == 7
        _, l64, c64 = case.reference("f64")
        both = flying & (l64 == 7)
        # a Hover env outside its cost-free box at every one of its seven steps has cost 7: the last step's cost is in the sum
        assert (c64[both] == 7).any() and np.array_equal(cost[both], c64[both])
    elif edge == "max_steps_40_limit_25":
        assert length.max() == 25 and (length == 25).any() and (length < 25).any()
    else:
        assert length[0].max() <= 3 and (length[1:].max(axis=1) == case.limit).any()


@pytest.mark.parametrize("name", eo.SHAPE_CASES)
def test_hidden_shapes_against_the_reference_and_bitwise_against_composed(name):
    """the hidden sizes at which forward16_shape (csrc/pds_mlp_fwd.h) takes another instantiation -- 1, 2, 3, 16, 17, 33, 49, 64
    units: the number of data steps in the last 16-wide tile -- with relu and tanh, on Hover lean (42 inputs), P = 2, E = 64,
    limit 20.  (17, 33) has 1461 parameters: policy 1's row starts at an odd float, so none of its six tensors is 8- or 16-byte
    aligned."""
    case = eo.shape_case(name)
    if case.shape[1:] == (17, 33):
        assert case.rows.shape[1] % 2 == 1
    _both_paths(case, bitwise=True)
