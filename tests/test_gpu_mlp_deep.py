"""csrc/pds_mlp_deep.hip (include/pds_mlp_deep.h) through fused.FusedMLP: forward, PPO-clip policy gradient and value-regression
gradient of networks with three and four hidden layers against float64 torch autograd on a copy of the same Sequential, over
the table of tests/mlp_deep_cases.py; value edges; the Adam step that rides on a gradient call; hipGraph capture; the refusals
of everything that takes a struct pds_mlp; and that networks with two hidden layers go the way they went.

Every table case runs its kernel twice (equal bits), checks the shape and the bar of mlp_deep_cases (the two-hidden-layer bar or
the 4-unit rule, see there) and records the ratio to the bar that applied as `margin` (+ `bar`: which side)."""
import copy
import ctypes as C
import math
import zlib

import pytest
import torch

import mlp_cases as mc
import mlp_deep_cases as dc

pytestmark = pytest.mark.gpu

CLIP = dc.CLIP


def _seed(c):
    return zlib.crc32(dc.case_id(c).encode()) % 10007


def _fused(c, seed):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = dc.make_net(c.d_in, c.hidden, c.d_out, c.act, seed)
    fm = FusedMLP(net, c.act)
    assert fm.deep and fm.n_hidden == len(c.hidden) and not hasattr(fm, "m")
    return net, fm


def _rows(c):
    return c.B if c.index is None else c.B + c.B // 2 + 1


def _record(record_property, worst, side):
    record_property("margin", worst)
    record_property("bar", side)


# ---- the case table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in dc.CASES if c.kind == "fwd"], ids=dc.case_id)
def test_forward_against_float64(c, record_property):
    s = _seed(c)
    net, fm = _fused(c, s)
    g = torch.Generator(device="cuda").manual_seed(s)
    x = 2 * torch.randn(_rows(c), c.d_in, device="cuda", generator=g)
    idx = mc.make_index(c.index, x.shape[0], c.B, s) if c.index else None
    mean = torch.randn(c.d_in, device="cuda", generator=g) if c.std else None
    std = torch.rand(c.d_in, device="cuda", generator=g) + 0.5 if c.std else None
    y = fm.forward(x, index=idx, mean=mean, std=std, eps=1e-5).clone()
    assert torch.equal(y, fm.forward(x, index=idx, mean=mean, std=std, eps=1e-5))
    assert y.shape == (c.B, c.d_out)
    want = dc.ref_forward(net, x, idx, mean, std, 1e-5)
    f32 = dc.ref_forward(net, x, idx, mean, std, 1e-5, dtype=torch.float32)
    _record(record_property, *dc.check_all([("y", y, want, f32, 1e-5, 5e-6 if c.std else 2e-6)]))


@pytest.mark.parametrize("c", [c for c in dc.CASES if c.kind == "ppo"], ids=dc.case_id)
def test_policy_gradient_against_float64(c, record_property):
    s = _seed(c)
    net, fm = _fused(c, s)
    x, act, adv, logp_old, log_std = dc.ppo_inputs(net, c.B, s)
    st = fm.ppo_grad(x, act, adv, logp_old, log_std, CLIP).clone()
    got = fm.flat_grad.clone()
    st2 = fm.ppo_grad(x, act, adv, logp_old, log_std, CLIP).clone()
    assert torch.equal(got, fm.flat_grad) and torch.equal(st, st2)
    assert got.shape == (sum(p.numel() for p in net.parameters()),) and st.shape == (4,)
    want, wst = dc.ref_ppo(net, x, act, adv, logp_old, log_std)
    fgrad, fst = dc.ref_ppo(net, x, act, adv, logp_old, log_std, dtype=torch.float32)
    _record(record_property, *dc.check_all(dc.ppo_parts(got, st, want, wst, fgrad, fst, c.B)))


@pytest.mark.parametrize("c", [c for c in dc.CASES if c.kind == "mse"], ids=dc.case_id)
def test_value_gradient_against_float64(c, record_property):
    s = _seed(c)
    net, fm = _fused(c, s)
    g = torch.Generator(device="cuda").manual_seed(s)
    rows = _rows(c)
    x = torch.randn(rows, c.d_in, device="cuda", generator=g)
    target = torch.randn(rows, device="cuda", generator=g)
    idx = mc.make_index(c.index, rows, c.B, s) if c.index else None
    st = fm.value_grad(x, target, idx).clone()
    got = fm.flat_grad.clone()
    st2 = fm.value_grad(x, target, idx).clone()
    assert torch.equal(got, fm.flat_grad) and torch.equal(st, st2)
    assert got.shape == (sum(p.numel() for p in net.parameters()),) and st.shape == (4,) and float(st[3]) == c.B
    want, sse = dc.ref_mse(net, x, target, idx)
    fgrad, fsse = dc.ref_mse(net, x, target, idx, dtype=torch.float32)
    _record(record_property, *dc.check_all(dc.mse_parts(got, st, want, sse, fgrad, fsse, c.B)))


# ---- value edges --------------------------------------------------------------------------------------------------------
_EDGE_SHAPES = [(34, (50, 30, 20), "3"), (34, (32, 32, 32, 32), "4")]
_DEAD = 1  # the hidden layer whose weights and bias are zeroed (0-based)


def _kill(net, j):
    lin = [l for l in net if isinstance(l, torch.nn.Linear)]
    with torch.no_grad():
        lin[j].weight.zero_()
        lin[j].bias.zero_()
    return lin


def _zero_span(lin, j):
    """flat-layout length of what must be exactly zero with hidden layer j dead in a relu network: H(j+1) = 0 and act'(0) = 0, so
    dZ(j+1) = 0 -- every parameter of layers 0 .. j -- and dW(j+1) = dZ(j+2)^T H(j+1) = 0.  The biases from layer j + 1 on and the
    weights behind it see relu(b(j+1)) and the loss: they are not zero and are held to the bar."""
    return sum(l.weight.numel() + l.bias.numel() for l in lin[:j + 1]) + lin[j + 1].weight.numel()


@pytest.mark.parametrize("d_in,hidden,_id", _EDGE_SHAPES, ids=[s[2] for s in _EDGE_SHAPES])
def test_policy_gradient_value_edges(d_in, hidden, _id, record_property):
    """a relu network dead past hidden layer 1 (all-zero weights and bias: exact zeros, see _zero_span), adv = 0 on every sample
    (the whole gradient is exactly zero), and log_std at -3 and +1 on the live network"""
    from phoenix_drone_simulation_amd.fused import FusedMLP
    B, worst, sides = 999, 0.0, set()
    net = dc.make_net(d_in, hidden, 4, "relu", 77)
    x, act, adv, logp_old, _ = dc.ppo_inputs(net, B, 5)
    fm = FusedMLP(net, "relu")
    for ls in (-3.0, 1.0):
        log_std = torch.full((4,), ls, device="cuda")
        with torch.no_grad():
            mu = net(x)
            a = mu + math.exp(ls) * torch.randn(B, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)).clamp(-3, 3)
            lp = torch.distributions.Normal(mu, torch.exp(log_std)).log_prob(a).sum(-1) + 0.3 * torch.sin(torch.arange(B, device="cuda") * 1.7)
        st = fm.ppo_grad(x, a, adv, lp, log_std, CLIP).clone()
        got = fm.flat_grad.clone()
        want, wst = dc.ref_ppo(net, x, a, adv, lp, log_std)
        fgrad, fst = dc.ref_ppo(net, x, a, adv, lp, log_std, dtype=torch.float32)
        w, s = dc.check_all(dc.ppo_parts(got, st, want, wst, fgrad, fst, B))
        worst, sides = max(worst, w), sides | {s}
    log_std = torch.full((4,), math.log(0.3), device="cuda")
    st = fm.ppo_grad(x, act, torch.zeros_like(adv), logp_old, log_std, CLIP).clone()
    assert not bool(fm.flat_grad.any()) and float(st[0]) == 0.0 and float(st[3]) == B
    lin = _kill(net, _DEAD)
    st = fm.ppo_grad(x, act, adv, logp_old, log_std, CLIP).clone()
    got = fm.flat_grad.clone()
    want, wst = dc.ref_ppo(net, x, act, adv, logp_old, log_std)
    fgrad, fst = dc.ref_ppo(net, x, act, adv, logp_old, log_std, dtype=torch.float32)
    nz = _zero_span(lin, _DEAD)
    assert not bool(want[:nz].any()) and bool(want[nz:].any())
    assert not bool(got[:nz].any())
    w, s = dc.check_all(dc.ppo_parts(got, st, want, wst, fgrad, fst, B))
    _record(record_property, max(worst, w), "4-unit" if "4-unit" in sides | {s} else "two-layer")


@pytest.mark.parametrize("d_in,hidden,_id", _EDGE_SHAPES, ids=[s[2] for s in _EDGE_SHAPES])
def test_value_gradient_value_edges(d_in, hidden, _id, record_property):
    """targets 30 away from the prediction on every seventh sample and equal to the float32 prediction on every ninth, through a
    row index; then the relu network dead past hidden layer 1 (exact zeros, see _zero_span)"""
    from phoenix_drone_simulation_amd.fused import FusedMLP
    B, rows = 999, 1500
    net = dc.make_net(d_in, hidden, 1, "relu", 78)
    fm = FusedMLP(net, "relu")
    g = torch.Generator(device="cuda").manual_seed(10)
    x = 2 * torch.randn(rows, d_in, device="cuda", generator=g)
    with torch.no_grad():
        pred = net(x).squeeze(-1)
    r = torch.arange(rows, device="cuda")
    target = torch.randn(rows, device="cuda", generator=g)
    target = torch.where(r % 7 == 3, pred + 30.0 * torch.sign(target), target)
    target = torch.where(r % 9 == 2, pred, target)
    idx = mc.make_index("perm", rows, B, 12)
    worst, sides = 0.0, set()
    for dead in (False, True):
        if dead:
            lin = _kill(net, _DEAD)
        st = fm.value_grad(x, target, idx).clone()
        got = fm.flat_grad.clone()
        want, sse = dc.ref_mse(net, x, target, idx)
        fgrad, fsse = dc.ref_mse(net, x, target, idx, dtype=torch.float32)
        if dead:
            nz = _zero_span(lin, _DEAD)
            assert not bool(want[:nz].any()) and bool(want[nz:].any())
            assert not bool(got[:nz].any())
        w, s = dc.check_all(dc.mse_parts(got, st, want, sse, fgrad, fsse, B))
        worst, sides = max(worst, w), sides | {s}
    _record(record_property, worst, "4-unit" if "4-unit" in sides else "two-layer")


# ---- Adam ---------------------------------------------------------------------------------------------------------------
_ADAM_SHAPES = {3: (34, (50, 30, 20)), 4: (34, (32, 32, 32, 32))}


def _adam_call(kind, fm, data, lr):
    if kind == "ppo":
        return fm.ppo_grad(*data, CLIP, adam_lr=lr).clone()
    return fm.value_grad(*data, adam_lr=lr).clone()


@pytest.mark.parametrize("kind", ["ppo", "mse"])
@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("ragged", [False, True], ids=["B17", "ragged"])
def test_gradient_call_with_adam_step_equals_gradient_then_adam_step_bitwise(kind, depth, ragged):
    """parameters, moments, flat_grad and stats of `grad(adam_lr=lr)` against `grad()` + `adam_step(lr)` over three steps, bit for
    bit; and three consecutive adam_step calls against torch.optim.Adam, both ON the float32 autograd gradient of the same loss
    (rtol 1e-5, with the atol 1e-7 of test_adam_step_matches_torch_adam for parameters near zero).

    Both optimisers take the SAME gradient on purpose.  Driving torch.optim.Adam with the autograd gradient and the kernels with
    their own is not a well-posed comparison at this bar: the first step moves a parameter by lr g / (|g| + 1e-8), so an entry
    with |g| near 1e-8 (a relu unit that few samples reach, a mean over 33 000 samples that nearly cancels) turns an absolute
    difference d between two float32 gradients into lr d / 1e-8 -- 3e-6 for d = 1e-10, far inside the gradient bar and thirty
    times this one.  Run that way the first time, six of the eight cases met the bar and the two depth-4 policy cases missed it
    by 2.1e-6 (B = 17) and 7.6e-6 (the ragged batch) on parameters of order 0.1.  The kernels' gradient is held to float64 by
    the case table above; what this test pins is the arithmetic of the step."""
    from phoenix_drone_simulation_amd.fused import FusedMLP
    d_in, hidden = _ADAM_SHAPES[depth]
    B = dc.tail(kind, depth, 1) if ragged else 17
    act, d_out = ("relu", 4) if kind == "ppo" else ("tanh", 1)
    net_a = dc.make_net(d_in, hidden, d_out, act, 21)
    net_b, net_c, ref = copy.deepcopy(net_a), copy.deepcopy(net_a), dc.net_as(net_a, torch.float32)
    fa, fb, fc = FusedMLP(net_a, act), FusedMLP(net_b, act), FusedMLP(net_c, act)
    opt = torch.optim.Adam(ref.parameters(), lr=3e-4)
    if kind == "ppo":
        data = dc.ppo_inputs(net_a, B, 4)
    else:
        g = torch.Generator(device="cuda").manual_seed(4)
        data = (torch.randn(B, d_in, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g))
    for _ in range(3):
        sa = _adam_call(kind, fa, data, 3e-4)
        sb = _adam_call(kind, fb, data, None)
        fb.adam_step(3e-4)
        assert torch.equal(sa, sb) and torch.equal(fa.flat_grad, fb.flat_grad)
        assert torch.equal(fa.exp_avg, fb.exp_avg) and torch.equal(fa.exp_avg_sq, fb.exp_avg_sq)
        for p, q in zip(net_a.parameters(), net_b.parameters()):
            assert torch.equal(p, q)
        opt.zero_grad()
        if kind == "ppo":
            x, a, adv, lp, ls = data
            d = torch.distributions.Normal(ref(x), torch.exp(ls))
            ratio = torch.exp(d.log_prob(a).sum(-1) - lp)
            (-torch.min(ratio * adv, adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP))).mean().backward()
        else:
            ((ref(data[0]).squeeze(-1) - data[1]) ** 2).mean().backward()
        fc.flat_grad.copy_(torch.cat([p.grad.reshape(-1) for p in ref.parameters()]))
        fc.adam_step(3e-4)
        opt.step()
    for p, q in zip(net_c.parameters(), ref.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), float((p - q).abs().max())


# ---- capture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [3, 4])
def test_forward_inside_a_captured_graph_equals_the_eager_call(depth):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    d_in, hidden = _ADAM_SHAPES[depth]
    net = dc.make_net(d_in, hidden, 4, "relu", 5)
    fm = FusedMLP(net, "relu")
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(1000, d_in, device="cuda", generator=g)
    mean, std = torch.randn(d_in, device="cuda", generator=g), torch.rand(d_in, device="cuda", generator=g) + 0.5
    y = torch.empty(1000, 4, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fm.forward(x, mean=mean, std=std, out=y)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fm.forward(x, mean=mean, std=std, out=y)
    for k in range(2):
        x.copy_(torch.randn(1000, d_in, device="cuda", generator=g) * (k + 1))
        graph.replay()
        assert torch.equal(y, fm.forward(x, mean=mean, std=std))


# ---- refusals through Python, and the shallow path ------------------------------------------------------------------------
class _Env:
    """stands where an env would: the refusal comes before anything reads it"""
    _handle = None
    lib = None
    num_envs = 64


def test_what_takes_a_struct_pds_mlp_refuses_a_deep_network():
    from phoenix_drone_simulation_amd import fused, native
    net = dc.make_net(34, (50, 30, 20), 4, "relu", 1)
    fm = fused.FusedMLP(net, "relu")
    shallow = fused.FusedMLP(dc.make_net(38, (64, 64), 1, "relu", 2), "relu")
    t = torch.zeros(64, 34, device="cuda")
    v = torch.zeros_like(fm.flat_grad)
    ls = torch.zeros(4, device="cuda")
    env = _Env()
    calls = [lambda: fm.fisher_vector_product(t, v, ls, 0.1),
             lambda: fm.surrogate_kl(v, torch.ones(2, device="cuda"), t, t, t, t, t, ls),
             lambda: fm._npg_workspace(0),
             lambda: fm.ddpg_policy_grad(shallow, t, None, 1.0),
             lambda: fm.sac_policy_grad(shallow, shallow, t, None, 0.2, 1.0, 0, 0),
             lambda: fused.fused_rollout(env, fm, shallow, 2, *([None] * 20)),
             lambda: fused.fused_rollout(env, shallow, fm, 2, *([None] * 20)),
             lambda: fused.fused_rollout_history(env, fm, 2, 4, *([None] * 19)),
             lambda: fused.fused_collect(env, fm, 0, 2, 1.0, *([None] * 12)),
             lambda: fused.collect_supported(env, fm, 0),
             lambda: fused.collect_control_supported(env, fm, 0),
             lambda: fused.ddpg_supported(fm, shallow),
             lambda: fused.ddpg_supported(shallow, fm),
             lambda: fused.sac_supported(fm, shallow, shallow),
             lambda: fused.ddpg_target(fm, shallow, t, None, t, t, 0.99, 1.0, t),
             lambda: fused.sac_target(fm, shallow, shallow, t, None, t, t, 0.99, 0.2, 1.0, 0, 0, t),
             lambda: fused.polyak(fm, fm, 0.995),
             lambda: native.call("pds_mlp_forward", fm, t, None, 64, None, None, 0.0, t, on=t)]
    for f in calls:
        with pytest.raises(NotImplementedError, match="2 hidden layers"):
            f()
    with pytest.raises(NotImplementedError):  # more than 64 inputs at depth 3: a valid network the deep kernels do not cover
        fused.FusedMLP(dc.make_net(68, (50, 30, 20), 4, "relu", 1), "relu")
    with pytest.raises(ValueError, match="3 or 4 hidden layers"):
        fused.FusedMLP(dc.make_net(34, (50, 65, 20), 4, "relu", 1), "relu")
    with pytest.raises(NotImplementedError):
        fused.FusedMLP(dc.make_net(34, (8, 8, 8, 8, 8), 4, "relu", 1), "relu")


def test_two_hidden_layers_go_the_way_they_went():
    """deep is False, and forward / ppo_grad give the bits of pds_mlp_forward / pds_ppo_policy_grad_step entered directly"""
    from phoenix_drone_simulation_amd import fused, native
    net = mc.make_net(34, 50, 50, 4, "relu", 3)
    fm = fused.FusedMLP(net, "relu")
    assert fm.deep is False and isinstance(fm.m, native.Mlp) and fm.n_hidden == 2
    x, act, adv, logp_old, log_std = dc.ppo_inputs(net, 3000, 8)
    y = torch.empty(3000, 4, device="cuda")
    native.call("pds_mlp_forward", fm, x, None, 3000, None, None, 1e-5, y, on=x)
    assert torch.equal(y, fm.forward(x))
    grads, stats = torch.empty_like(fm.flat_grad), torch.empty(4, device="cuda")
    ws = torch.empty(native.load().pds_mlp_workspace_floats(C.byref(fm.m)), device="cuda")
    native.call("pds_ppo_policy_grad_step", fm, x, act, adv, logp_old, log_std, 3000, CLIP, grads, stats, ws, None, on=x)
    st = fm.ppo_grad(x, act, adv, logp_old, log_std, CLIP)
    assert torch.equal(grads, fm.flat_grad) and torch.equal(stats, st)
