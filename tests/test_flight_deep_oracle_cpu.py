"""tests/flight_deep_oracle.py pinned on the CPU, for the six cases tests/test_gpu_evaluate_deep.py flies: its float32 run against
its float64 run (the distance is the UNIT of the GPU test's bar, printed here; the envs whose lengths disagree inside
evaluate_oracle.length_cap), its numpy actor against a float64 torch Sequential built from the same row, and TEETH: on the float64
reference alone, each mistake a kernel for three or four hidden layers could make -- a hidden layer dropped, two layers swapped,
an activation on the output, another policy's row in a tile -- moves a result by more than 100 bars (a bar is BAR_UNITS = 4
units), so a device result inside the bar cannot hold it."""
import numpy as np
import pytest
import torch

import evaluate_oracle as eo
import flight_deep_oracle as fdo
import flight_oracle as fo

BAR_UNITS = 4.0
TEETH = 100 * BAR_UNITS


@pytest.mark.parametrize("name", fdo.DEEP_CASES)
def test_float32_flight_against_float64_flight(name):
    """the units, printed; lengths and integer metrics agree inside length_cap; the cases hold what they are meant to: both
    endings where the task terminates, saturated steps for the saturation metric to count, finite values"""
    c = fdo.deep_case(name)
    assert (c.P, c.E, c.limit, c.max_steps, c.seed) == (8, 128, 40, 40, 11) and len(c.hidden) in (3, 4)
    f32, f64 = fdo.flight(c, "f32"), fdo.flight(c, "f64")
    agree = fo.agreeing(c)
    excluded = int((~agree).sum())
    units = fdo.units_of(c)
    print(f"{name}: N = {c.N}, T = {c.max_steps}, {excluded} envs excluded (cap {eo.length_cap(c.N)})")
    for k, v in units.items():
        print(f"UNIT {name} {k} {v:.3e}")
        assert np.isfinite(v) and v > 0, k
    unit, _, top = eo.unit_of(c)
    print(f"UNIT {name} return {unit:.3e} (max |return| {top:.3e})")
    assert excluded <= eo.length_cap(c.N)
    wrong = agree & (f32["metrics"][..., list(fo.EM_INTEGER)] != f64["metrics"][..., list(fo.EM_INTEGER)]).any(axis=-1)
    assert int(wrong.sum()) <= eo.length_cap(c.N)
    for fl in (f32, f64):
        for k in ("ret", "length", "cost", "metrics", "state", "action", "observation", "sum_d", "sum_d2"):
            assert np.isfinite(fl[k]).all(), k
    L = f64["length"]
    print(f"{name}: lengths {int(L.min())} .. {int(L.max())}, saturated first-episode steps {int(f64['metrics'][..., 5].sum())}")
    if c.terminates:
        assert (L < c.limit).any() and (L == c.limit).any()
    else:
        assert (L == c.limit).all()
    assert f64["metrics"][..., 5].sum() >= 9000
    assert f64["observation"].shape == (c.P, c.E, c.max_steps, c.shape[0])
    if c.has_cost:
        assert (f64["cost"] > 0).any()
    else:
        assert not f64["cost"].any()


def _sequential(case, p):
    """policy p of the case as a float64 torch Sequential(Linear, act, ..., Linear), its parameters cut from the row in torch order"""
    sizes = case.shape + (4,)
    row, k, mods = torch.from_numpy(case.rows[p].astype(np.float64)), 0, []
    for j, (n_in, n_out) in enumerate(zip(sizes[:-1], sizes[1:])):
        lin = torch.nn.Linear(n_in, n_out).double()
        with torch.no_grad():
            lin.weight.copy_(row[k:k + n_out * n_in].reshape(n_out, n_in)); k += n_out * n_in
            lin.bias.copy_(row[k:k + n_out]); k += n_out
        mods.append(lin)
        if j < len(sizes) - 2:
            mods.append({"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh}[case.activation]())
    assert k == row.numel() == sum(p.numel() for m in mods for p in m.parameters())
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("name", fdo.DEEP_CASES)
def test_the_numpy_actor_is_the_torch_sequentials(name):
    """every recorded action of the float64 flight = float32(Sequential(standardised observation)) of the env's policy, on the
    observation recorded with it: the actor, the row layout and the tile -> policy rule in one"""
    c = fdo.deep_case(name)
    f64 = fdo.flight(c, "f64")
    T = c.max_steps
    for p in range(c.P):
        o = torch.from_numpy(f64["observation_all"][p].reshape(c.E * T, -1).copy())
        if c.mean is not None:
            o = (o - torch.from_numpy(c.mean[p].astype(np.float64))) / (torch.from_numpy(c.std[p].astype(np.float64)) + np.float64(np.float32(c.eps)))
        with torch.no_grad():
            want = _sequential(c, p)(o).numpy().reshape(c.E, T, 4)
        got = f64["action_all"][p]  # (the float32 rounding of the numpy float64 output: within 2^-24 |v| of it; 2^-23 leaves the two float64 sums' own distance room)
        assert np.abs(got - want).max() <= 2.0 ** -23 * max(1.0, float(np.abs(want).max())), (name, p)


def _slipped(case, **kw):
    return fdo.fly(eo.TASK_OF[case.env_id], case.kwargs, case.rows, case.shape, case.activation, case.mean, case.std, case.eps, case.E,
                   case.max_steps, case.limit, case.seed, "f64", **kw)


def _bars(case, fl):
    """how far a slipped float64 flight is from the case's float64 flight, in bars, at its best: the return over every env, the
    first action and the four metric sums"""
    f64, units = fdo.flight(case, "f64"), fdo.units_of(case)
    unit, _, _ = eo.unit_of(case)
    out = {"return": float(np.abs(fl["ret"] - f64["ret"]).max()) / (BAR_UNITS * unit),
           "action(0)": float(np.abs(fl["action_all"][:, :, 0] - f64["action_all"][:, :, 0]).max()) / (BAR_UNITS * units["action"])}
    for j in fo.EM_SUMS:
        out[fo.EM[j]] = float(np.abs(fl["metrics"][..., j] - f64["metrics"][..., j]).max()) / (BAR_UNITS * units[fo.EM[j]])
    return out


def _drop_layer(l):
    def net(layers, x, act):
        return fdo.actor(layers[:l] + layers[l + 1:], x, act)
    return net


def _swap_layers(i, j):
    def net(layers, x, act):
        layers = list(layers)
        layers[i], layers[j] = layers[j], layers[i]
        return fdo.actor(layers, x, act)
    return net


def _act_on_output(layers, x, act):
    return act(fdo.actor(layers, x, act))


# (equal widths, so that a dropped and a swapped layer still multiply: one case per depth)
@pytest.mark.parametrize("name", ["circle_lean_motor", "hover_default"])
def test_teeth_of_the_deep_actor(name):
    c = fdo.deep_case(name)
    assert len(set(c.hidden)) == 1
    tiles = c.N // 64
    per = c.E // 64
    wrong_row = np.arange(tiles) // per
    wrong_row[per] = 0  # the first tile of policy 1 flies policy 0's row
    slips = {"hidden layer 2 dropped": dict(net=_drop_layer(1)),
             "the last hidden layer dropped": dict(net=_drop_layer(len(c.hidden) - 1)),
             "hidden layers 2 and 3 swapped": dict(net=_swap_layers(1, 2)),
             "an activation on the output": dict(net=_act_on_output),
             "policy 0's row in a tile of policy 1": dict(tile_policy=wrong_row)}
    same = _slipped(c)
    assert all(np.array_equal(same[k], fdo.flight(c, "f64")[k]) for k in ("ret", "length", "metrics", "action_all"))
    for what, kw in slips.items():
        bars = _bars(c, _slipped(c, **kw))
        print(f"TEETH {name} {what}: " + ", ".join(f"{k} {v:.0f}" for k, v in bars.items()) + " bars")
        assert bars["return"] > 100 and bars["action(0)"] > 100, (name, what, bars)
        assert max(bars[fo.EM[j]] for j in fo.EM_SUMS) > 100, (name, what, bars)
