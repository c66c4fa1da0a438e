"""csrc/pds_mlp.hip and csrc/pds_mlp_wide.hip across their whole dispatch table, against float64 autograd.

tests/mlp_cases.py restates the host predicates that pick an instantiation and holds the case table; the CPU test
test_mlp_dispatch_cpu.py checks that the table reaches every launch site of the two files.  Here every case runs its kernel
twice (bitwise-equal results: determinism) and compares with float64.

Bars come from float64 and are never looser than those of tests/test_gpu_fused_mlp.py for the same quantity: gradients
rtol 2e-4, atol 2e-6 of the largest entry (+ 10 / B from 20 000 samples on, _ppo_grad_case's allowance for a random batch
that puts a sample within float32 rounding of a relu or clip kink); loss and ratio sums 2e-5 relative, the kl sum 1e-5, the
sample count exact; the value loss 1e-5; the forward rtol 1e-5 with atol 2e-6 (5e-6 with the input standardisation).  The
value-edge tests build their inputs away from every kink and so drop the 10 / B allowance."""
import math
import zlib

import pytest
import torch

import mlp_cases as mc

pytestmark = pytest.mark.gpu

CLIP = 0.2


def _seed(c):
    return zlib.crc32(mc.case_id(c).encode()) % 10007


def _ppo_inputs(net, B, seed):
    d_in, A = net[0].in_features, net[4].out_features
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, d_in, device="cuda", generator=g)
    log_std = math.log(0.3) + 0.1 * torch.randn(A, device="cuda", generator=g)
    with torch.no_grad():
        mu0 = net(x)
        act = mu0 + torch.exp(log_std) * torch.randn(B, A, device="cuda", generator=g)
        logp_old = torch.distributions.Normal(mu0, torch.exp(log_std)).log_prob(act).sum(-1)
        logp_old = logp_old + 0.3 * torch.randn(B, device="cuda", generator=g)  # ratios on both sides of the clip range
    adv = torch.randn(B, device="cuda", generator=g)
    return x, act, adv, logp_old, log_std


def _check_ppo(got, st, want, wst, B, atol=None):
    atol = mc.grad_atol(want, B) if atol is None else atol
    err = float((got.double() - want).abs().max())
    assert torch.allclose(got.double(), want, rtol=2e-4, atol=atol), (err, atol)
    loss, ratio, kl = float(wst[0]) / B, float(wst[1]) / B, float(wst[2])
    assert abs(float(st[0]) / B - loss) < 2e-5 * max(1.0, abs(loss)), (float(st[0]) / B, loss)
    assert abs(float(st[1]) / B - ratio) < 2e-5 * ratio, (float(st[1]) / B, ratio)
    assert abs(float(st[2]) - kl) < 1e-5 * kl, (float(st[2]), kl)
    assert float(st[3]) == B
    return err / atol


def _check_mse(got, st, want, sse, n, atol=None):
    atol = mc.grad_atol(want, n) if atol is None else atol
    err = float((got.double() - want).abs().max())
    assert torch.allclose(got.double(), want, rtol=2e-4, atol=atol), (err, atol)
    loss = float(sse) / n
    assert abs(float(st[0]) / n - loss) < 1e-5 * max(1.0, loss), (float(st[0]) / n, loss)
    return err / atol


def _fused(c, seed):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = mc.make_net(c.d_in, c.h1, c.h2, c.d_out, c.act, seed)
    return net, FusedMLP(net, c.act)


def _rows(c):
    return c.B if c.index is None else c.B + c.B // 2 + 1


# ---- the case table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in mc.CASES if c.kind == "fwd"], ids=mc.case_id)
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
    want = mc.ref_forward(net, x, idx, mean, std, 1e-5)
    atol = 5e-6 if c.std else 2e-6
    assert y.shape == (c.B, c.d_out)
    assert torch.allclose(y.double(), want, rtol=1e-5, atol=atol), float((y.double() - want).abs().max())
    record_property("member", mc.case_member(c))
    record_property("margin", float(((y.double() - want).abs() / (atol + 1e-5 * want.abs())).max()))


@pytest.mark.parametrize("c", [c for c in mc.CASES if c.kind == "ppo"], ids=mc.case_id)
def test_policy_gradient_against_float64(c, record_property):
    s = _seed(c)
    net, fm = _fused(c, s)
    x, act, adv, logp_old, log_std = _ppo_inputs(net, c.B, s)
    st = fm.ppo_grad(x, act, adv, logp_old, log_std, CLIP).clone()
    got = fm.flat_grad.clone()
    st2 = fm.ppo_grad(x, act, adv, logp_old, log_std, CLIP).clone()
    assert torch.equal(got, fm.flat_grad) and torch.equal(st, st2)
    want, wst = mc.ref_ppo(net, x, act, adv, logp_old, log_std, CLIP)
    record_property("member", mc.case_member(c))
    record_property("margin", _check_ppo(got, st, want, wst, c.B))


@pytest.mark.parametrize("c", [c for c in mc.CASES if c.kind == "mse"], ids=mc.case_id)
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
    want, sse = mc.ref_mse(net, x, target, idx)
    record_property("member", mc.case_member(c))
    record_property("margin", _check_mse(got, st, want, sse, c.B))


# ---- value edges --------------------------------------------------------------------------------------------------------
_LOG_RATIOS = (-2.5, -0.6, -0.1, 0.0, 0.1, 0.6, 2.5)


def _edge_inputs(net, act, B, seed, saturate=True):
    """x with every fifth row pushed to an edge: |x| = 40 x N(0, 1) for tanh (every unit of layer 1 saturated), x = 0 for relu
    together with b1, b2 < 0 (every unit of both layers dead on those rows: the output is b3).  Then the relu kinks are
    stepped around: rows whose float64 pre-activation of any hidden unit lies within 1e-3 of 0 are dropped (float32 puts
    ~1e-6 on a pre-activation of these sizes)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = B + B // 3 + 64
    x = torch.randn(n, net[0].in_features, device="cuda", generator=g) * 2
    edge = torch.arange(n, device="cuda") % 5 == 1
    if act == "tanh":
        if saturate:
            x[edge] *= 20.0
        return x[:B].contiguous()
    with torch.no_grad():
        net[0].bias.copy_(-net[0].bias.abs() - 0.05)
        net[2].bias.copy_(-net[2].bias.abs() - 0.05)
    x[edge] = 0.0
    n64 = mc.net64(net)
    with torch.no_grad():
        z1 = n64[0](x.double())
        z2 = n64[2](torch.relu(z1))
    keep = (z1.abs().min(-1).values > 1e-3) & (z2.abs().min(-1).values > 1e-3)
    x = x[keep][:B].contiguous()
    assert x.shape[0] == B and int((x.abs().sum(-1) == 0).sum()) > B // 8
    return x


@pytest.mark.parametrize("shape,act,log_std,B", [
    ((34, 50, 50, 4), "relu", -5.0, 5000), ((34, 50, 50, 4), "relu", 1.0, 5000), ((34, 50, 50, 4), "relu", -5.0, 70001),
    ((34, 50, 50, 4), "relu", 1.0, 70001), ((136, 64, 64, 4), "relu", -5.0, 5000), ((136, 64, 64, 4), "relu", 1.0, 40001),
    ((34, 64, 64, 4), "tanh", -5.0, 5000), ((34, 64, 64, 4), "tanh", 1.0, 40001), ((136, 64, 64, 4), "tanh", 1.0, 5000)])
def test_policy_gradient_value_edges(shape, act, log_std, B, record_property):
    """ratios far outside [1 - clip, 1 + clip] under both signs of the advantage, advantages of exactly 0, saturated tanh,
    dead relu rows, log_std of -5 and 1.  Every sample is kept off every kink: its log-ratio is set to one of
    -2.5, -0.6, -0.1, 0, 0.1, 0.6, 2.5 (by logp_old = float64 log-prob - log-ratio), at least 0.08 from log(0.8) and log(1.2);
    its action is mu + sigma z with |z| <= 3, so the float32 log-prob is off by at most |dz| |z| A ~ 4e-3 even at
    sigma = e^-5 (|dz| = |d mu| / sigma ~ 1e-6 / 6.7e-3); the advantage is +(0.5 + |N|), -(0.5 + |N|) or 0 (periods 3 and 11,
    coprime with the 7 log-ratios); relu pre-activations stay 1e-3 from 0 (_edge_inputs).  So no 10 / B allowance.

    At sigma = e^-5 the gradient weighs an error of the policy mean by 1 / sigma^2 = 2.2e4 (d logp / d mu = z / sigma): a
    float32 mean -- in any float32 implementation -- puts more than 2e-6 of the largest entry on the gradient.  The bar adds
    64 F, F = how far the float64 gradient moves when only mu is rounded to float32 on its way into the loss (mu correctly
    rounded, the best a float32 forward can do).  The kernels' mu also carries the rounding of three dot products of up to
    136 + 64 + 64 terms; measured: 7.4 F (34-50-50 relu), 9.5 F (34-64-64 tanh), 28 F (136-64-64 relu) at sigma = e^-5, where
    F is 1e-5 .. 4e-5 against a largest entry of 5 .. 15; at sigma = e^1, F ~ 1e-10 and the bar is the plain 2e-6 one."""
    d_in, h1, h2, A = shape
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = mc.make_net(d_in, h1, h2, A, act, 31 + B % 97)
    x = _edge_inputs(net, act, B, 5)
    fm = FusedMLP(net, act)
    g = torch.Generator(device="cuda").manual_seed(9)
    ls = torch.full((A,), log_std, device="cuda")
    with torch.no_grad():
        mu = mc.net64(net)(x.double())
    z = torch.randn(B, A, device="cuda", generator=g, dtype=torch.float64).clamp(-3, 3)
    act_t = (mu + math.exp(log_std) * z).float()
    d = torch.distributions.Normal(mu, torch.exp(ls.double()))
    u = torch.tensor(_LOG_RATIOS, device="cuda", dtype=torch.float64)[torch.arange(B, device="cuda") % 7]
    logp_old = (d.log_prob(act_t.double()).sum(-1) - u).float()
    r = torch.arange(B, device="cuda")
    mag = 0.5 + torch.randn(B, device="cuda", generator=g).abs()
    adv = torch.where(r % 3 == 0, mag, -mag)
    adv = torch.where(r % 11 == 4, torch.zeros_like(adv), adv)
    st = fm.ppo_grad(x, act_t, adv, logp_old, ls, CLIP).clone()
    got = fm.flat_grad.clone()
    want, wst = mc.ref_ppo(net, x, act_t, adv, logp_old, ls, CLIP)
    ratio = torch.exp(torch.distributions.Normal(mc.net64(net)(x.double()), torch.exp(ls.double())).log_prob(act_t.double()).sum(-1) - logp_old.double())
    lr = torch.log(ratio).detach()
    assert float(torch.minimum((lr - math.log(1 - CLIP)).abs(), (lr - math.log(1 + CLIP)).abs()).min()) > 0.05
    assert bool(((ratio > 10) & (adv > 0)).any() and ((ratio > 10) & (adv < 0)).any() and ((ratio < 0.1) & (adv > 0)).any()
                and ((ratio < 0.1) & (adv < 0)).any() and (adv == 0).any())
    # the float32 rounding of the policy mean alone (see the docstring)
    floor = float((mc.ref_ppo(net, x, act_t, adv, logp_old, ls, CLIP, round_mu=True)[0] - want).abs().max())
    record_property("floor_ratio", float((got.double() - want).abs().max()) / max(floor, 1e-30))
    record_property("margin", _check_ppo(got, st, want, wst, B, atol=2e-6 * max(float(want.abs().max()), 1.0) + 64 * floor))


@pytest.mark.parametrize("shape,act,B,use_index", [
    ((34, 64, 64), "tanh", 5000, True), ((34, 64, 64), "tanh", 40001, False), ((136, 64, 64), "tanh", 40001, True),
    ((34, 50, 50), "relu", 5000, True), ((136, 50, 50), "relu", 40001, False)])
def test_value_gradient_value_edges(shape, act, B, use_index, record_property):
    """saturated tanh rows and dead relu rows (_edge_inputs), targets 30 away from the prediction on every seventh sample
    and equal to the float32 prediction on every ninth (MSE has no kink: the relu rows are the only ones kept off one)"""
    d_in, h1, h2 = shape
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = mc.make_net(d_in, h1, h2, 1, act, 41 + B % 89)
    rows = B + B // 2 if use_index else B
    x = _edge_inputs(net, act, rows, 6)
    fm = FusedMLP(net, act)
    g = torch.Generator(device="cuda").manual_seed(10)
    with torch.no_grad():
        pred = net(x).squeeze(-1)
    r = torch.arange(rows, device="cuda")
    target = torch.randn(rows, device="cuda", generator=g)
    target = torch.where(r % 7 == 3, pred + 30.0 * torch.sign(target), target)
    target = torch.where(r % 9 == 2, pred, target)
    idx = mc.make_index("perm", rows, B, 12) if use_index else None
    st = fm.value_grad(x, target, idx).clone()
    got = fm.flat_grad.clone()
    want, sse = mc.ref_mse(net, x, target, idx)
    record_property("margin", _check_mse(got, st, want, sse, B, atol=2e-6 * max(float(want.abs().max()), 1.0)))


# ---- guard bands --------------------------------------------------------------------------------------------------------
_GUARD = 4096
_SENTINEL = -1.2345e33


def _in_slab(t, fill=float("nan")):
    """a contiguous copy of t inside a slab whose memory before and after it holds `fill`"""
    slab = torch.full((t.numel() + 2 * _GUARD,), fill, device=t.device, dtype=t.dtype)
    v = slab[_GUARD:_GUARD + t.numel()].view(t.shape)
    v.copy_(t)
    return v, slab


def _bands_intact(slab, n):
    bits = slab.view(torch.int32)
    want = torch.tensor([_SENTINEL], device=slab.device).view(torch.int32)
    return bool((bits[:_GUARD] == want).all() and (bits[_GUARD + n:] == want).all())


def _out_slab(n):
    slab = torch.full((n + 2 * _GUARD,), _SENTINEL, device="cuda")
    return slab[_GUARD:_GUARD + n], slab


def _swap_outputs(fm):
    """flat_grad, stats and workspace of `fm` as views into sentinel-banded slabs (p.grad rebound to the new flat_grad)"""
    slabs = {}
    for name in ("flat_grad", "stats", "workspace"):
        n = getattr(fm, name).numel()
        v, slab = _out_slab(n)
        v.fill_(0.0)
        setattr(fm, name, v)
        slabs[name] = (slab, n)
    off = 0
    for p in fm.params:
        p.grad = fm.flat_grad[off:off + p.numel()].view_as(p)
        off += p.numel()
    return slabs


_GUARD_CASES = [
    mc.Case("fwd", 34, 50, 50, 4, "relu", 1001, "perm", True), mc.Case("fwd", 63, 64, 33, 8, "tanh", 70003, None, False),
    mc.Case("fwd", 136, 64, 64, 4, "tanh", 33001, "rep", True), mc.Case("fwd", 191, 17, 49, 3, "relu", 17, None, False),
    mc.Case("ppo", 34, 50, 50, 4, "relu", 3001, None, False), mc.Case("ppo", 34, 50, 50, 4, "relu", 70001, None, False),
    mc.Case("ppo", 42, 50, 50, 4, "relu", 65537, None, False), mc.Case("ppo", 17, 33, 49, 5, "tanh", 1001, None, False),
    mc.Case("ppo", 49, 64, 64, 8, "relu", 65557, None, False), mc.Case("ppo", 161, 64, 64, 8, "relu", 40001, None, False),
    mc.Case("ppo", 97, 49, 17, 3, "tanh", 15, None, False),
    mc.Case("mse", 34, 64, 64, 1, "tanh", 20001, "perm", False), mc.Case("mse", 49, 50, 50, 1, "relu", 65553, None, False),
    mc.Case("mse", 97, 64, 64, 1, "tanh", 33003, "rep", False), mc.Case("mse", 192, 33, 17, 1, "relu", 1, None, False)]


@pytest.mark.parametrize("c", _GUARD_CASES, ids=mc.case_id)
def test_guard_bands(c):
    """inputs as contiguous views into NaN-banded slabs (rows of x that the index does not name NaN as well): the kernels
    may read clamped rows and columns (load_x) but nothing past the batch may reach a result -- finite and bitwise equal
    to the call on clean tensors.  Outputs (y via out=, flat_grad, stats, workspace) inside sentinel bands that must
    come back unchanged."""
    s = _seed(c)
    net, fm = _fused(c, s)
    g = torch.Generator(device="cuda").manual_seed(s)
    if c.kind == "fwd":
        x = 2 * torch.randn(_rows(c), c.d_in, device="cuda", generator=g)
        idx = mc.make_index(c.index, x.shape[0], c.B, s) if c.index else None
        mean = torch.randn(c.d_in, device="cuda", generator=g) if c.std else None
        std = torch.rand(c.d_in, device="cuda", generator=g) + 0.5 if c.std else None
        clean = fm.forward(x, index=idx, mean=mean, std=std).clone()
        xg, _ = _in_slab(x)
        if idx is not None:
            unused = torch.ones(x.shape[0], dtype=torch.bool, device="cuda")
            unused[idx] = False
            xg[unused] = float("nan")
        y, yslab = _out_slab(c.B * c.d_out)
        got = fm.forward(xg, index=idx, mean=mean, std=std, out=y.view(c.B, c.d_out))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)
        assert _bands_intact(yslab, c.B * c.d_out)
        return
    if c.kind == "ppo":
        args = _ppo_inputs(net, c.B, s)
        st = fm.ppo_grad(*args, CLIP).clone()
        clean = fm.flat_grad.clone()
        slabs = _swap_outputs(fm)
        guarded = [_in_slab(t)[0] for t in args[:4]] + [args[4]]
        st_g = fm.ppo_grad(*guarded, CLIP)
    else:
        rows = _rows(c)
        x = torch.randn(rows, c.d_in, device="cuda", generator=g)
        target = torch.randn(rows, device="cuda", generator=g)
        idx = mc.make_index(c.index, rows, c.B, s) if c.index else None
        st = fm.value_grad(x, target, idx).clone()
        clean = fm.flat_grad.clone()
        slabs = _swap_outputs(fm)
        xg, tg = _in_slab(x)[0], _in_slab(target)[0]
        if idx is not None:
            unused = torch.ones(rows, dtype=torch.bool, device="cuda")
            unused[idx] = False
            xg[unused] = float("nan")
            tg[unused] = float("nan")
        st_g = fm.value_grad(xg, tg, idx)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(fm.flat_grad).all()) and bool(torch.isfinite(st_g).all())
    assert torch.equal(fm.flat_grad, clean) and torch.equal(st_g, st)
    for name, (slab, n) in slabs.items():
        assert _bands_intact(slab, n), name
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in fm.params]), clean)


# ---- fused Adam ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,act,B", [("ppo", (136, 64, 64, 4), "relu", 40001), ("mse", (136, 64, 64, 1), "tanh", 40001),
                                              ("ppo", (47, 33, 63, 5), "tanh", 40001), ("mse", (161, 17, 49, 1), "relu", 17)])
def test_gradient_call_with_adam_step_equals_gradient_then_adam_step_bitwise_over_wide_partials(kind, shape, act, B):
    """the optimiser step of reduce_kernel over the wide kernels' one partial per WAVE (1 024 of them) and over a narrow
    non-default shape: after 4 steps the parameters, both moment buffers (themselves in sentinel bands) and the gradient
    equal the route through pds_adam_step bit for bit"""
    import copy
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net_a = mc.make_net(*shape, act, 23)
    net_b = copy.deepcopy(net_a)
    fa, fb = FusedMLP(net_a, act), FusedMLP(net_b, act)
    bands = []
    for f in (fa, fb):
        f.exp_avg, s1 = _out_slab(f.flat_grad.numel())
        f.exp_avg_sq, s2 = _out_slab(f.flat_grad.numel())
        f.exp_avg.zero_(); f.exp_avg_sq.zero_(); f.adam_steps = 0
        bands += [s1, s2]
    g = torch.Generator(device="cuda").manual_seed(4)
    if kind == "ppo":
        args = _ppo_inputs(net_a, B, 4)
    else:
        x = torch.randn(2 * B, shape[0], device="cuda", generator=g)
        tgt = torch.randn(2 * B, device="cuda", generator=g)
        idx = mc.make_index("perm", 2 * B, B, 4)
    before = net_a[0].weight.detach().clone()
    for it in range(4):
        lr = 3e-4 * (it + 1)
        if kind == "ppo":
            fa.ppo_grad(*args, CLIP); fa.adam_step(lr)
            fb.ppo_grad(*args, CLIP, adam_lr=lr)
        else:
            fa.value_grad(x, tgt, idx); fa.adam_step(lr)
            fb.value_grad(x, tgt, idx, adam_lr=lr)
        assert torch.equal(fa.flat_grad, fb.flat_grad), it
    for pa, pb in zip(net_a.parameters(), net_b.parameters()):
        assert torch.equal(pa, pb)
    assert torch.equal(fa.exp_avg, fb.exp_avg) and torch.equal(fa.exp_avg_sq, fb.exp_avg_sq)
    assert fa.adam_steps == fb.adam_steps == 4
    assert not torch.equal(net_a[0].weight, before)
    n = fa.flat_grad.numel()
    assert all(_bands_intact(s, n) for s in bands)
