"""Helpers for tests/test_gpu_mlp_deep.py and tests/test_mlp_deep_cpu.py: the case table of the kernels for networks with three
and four hidden layers (csrc/pds_mlp_deep.hip, include/pds_mlp_deep.h), the three references -- forward, PPO-clip policy gradient,
value-regression gradient -- as torch autograd on a copy of the same Sequential in a chosen dtype (float64: the reference;
float32: the restatement that measures the unit of the 4-unit rule), and the bar.

The bar (BAR_UNITS = 4): a result passes if it meets the bar of the two-hidden-layer kernels (tests/test_gpu_mlp_dispatch.py:
forward rtol 1e-5 with atol 2e-6, 5e-6 with the standardisation; gradients rtol 2e-4 with atol mlp_cases.grad_atol; the
statistics bars of _check_ppo / _check_mse), or if its largest absolute error is within 4 units, a unit being the largest
absolute distance of float32 torch on the same device, the same network and the same inputs from the float64 reference.  The unit
is measured against the float32 restatement of the reference, never against the kernel."""
import copy
from collections import namedtuple

import mlp_cases as mc

TILE = mc.TILE
MAX_BLOCKS = 256          # kDeepMaxBlocks
BAR_UNITS = 4
CLIP = 0.2

Case = namedtuple("Case", "kind d_in hidden d_out act B index std")


def waves(kind, depth):
    """deep_waves<L, LOSS>: the gradient forms at depth 4 run three waves per block (LDS), everything else four"""
    return 3 if depth == 4 and kind != "fwd" else 4


def grid_round(kind, depth):
    """samples one persistent grid covers before its waves stride into their second tile"""
    return MAX_BLOCKS * waves(kind, depth) * TILE


def tail(kind, depth, k):
    """a ragged batch past the second full round of the grid"""
    return 2 * grid_round(kind, depth) + TILE * (3 + k) + 5 + 2 * k


# distinct widths per layer (a swapped dimension shows), both sides of every 16-boundary, the padded extremes
SHAPES3 = [(1, (1, 16, 17), 1), (15, (17, 33, 48), 3), (16, (64, 49, 63), 5), (17, (63, 1, 50), 8), (34, (50, 30, 20), 4),
           (34, (40, 40, 40), 4), (34, (30, 30, 30), 4), (48, (16, 64, 33), 2), (49, (33, 17, 64), 4), (64, (64, 64, 64), 8)]
SHAPES4 = [(1, (16, 1, 17, 1), 1), (16, (17, 33, 49, 64), 8), (34, (32, 32, 32, 32), 4), (34, (25, 25, 25, 25), 4),
           (40, (50, 30, 20, 10), 4), (63, (64, 48, 33, 17), 3), (64, (64, 64, 64, 64), 8)]
CRITICS = [(34, (64, 64, 64), 1), (40, (64, 64, 64, 64), 1)]
SMALL = (1, 15, 16, 17)
INDEX = (None, "perm", "rep")


def _case_table():
    cases = []
    for i, (d, hid, o) in enumerate(SHAPES3 + SHAPES4 + CRITICS):
        L, act = len(hid), ("relu", "tanh")[i % 2]
        cases.append(Case("fwd", d, hid, o, act, SMALL[i % 4], None, i % 2 == 1))
        cases.append(Case("fwd", d, hid, o, act, tail("fwd", L, i), INDEX[i % 3], i % 2 == 0))
        cases.append(Case("ppo", d, hid, o, act, SMALL[(i + 1) % 4], None, False))
        cases.append(Case("ppo", d, hid, o, ("tanh", "relu")[i % 2] if i % 3 == 0 else act, tail("ppo", L, i), None, False))
        cases.append(Case("mse", d, hid, 1, ("tanh", "relu")[i % 2], SMALL[(i + 2) % 4], INDEX[i % 3], False))
        cases.append(Case("mse", d, hid, 1, ("tanh", "relu")[i % 2], tail("mse", L, i), INDEX[(i + 1) % 3], False))
    # what the trainer runs at its largest
    cases += [Case("ppo", 34, (50, 30, 20), 4, "relu", 524288, None, False),
              Case("mse", 34, (64, 64, 64), 1, "tanh", 524288, "perm", False),
              Case("mse", 34, (64, 64, 64), 1, "tanh", 524288, "rep", False),
              Case("fwd", 34, (50, 30, 20), 4, "relu", 1 << 20, None, True)]
    return cases


CASES = _case_table()


def case_id(c):
    return (f"{c.kind}-{c.d_in}x{'x'.join(map(str, c.hidden))}x{c.d_out}-{c.act}-B{c.B}" + (f"-{c.index}" if c.index else "") +
            ("-std" if c.std else ""))


# ---- networks and references (torch is imported lazily: the CPU test imports this module without a device) ----------------
def make_net(d_in, hidden, d_out, act, seed, device="cuda"):
    import torch
    from phoenix_drone_simulation_amd.ppo import _mlp
    torch.manual_seed(seed)
    return _mlp([d_in] + list(hidden) + [d_out], act).to(device)


def net_as(net, dtype):
    """a copy of the Sequential in `dtype` (its own parameters and .grad: a FusedMLP ties the original's .grad to its flat buffer)"""
    n = copy.deepcopy(net).to(dtype)
    for p in n.parameters():
        p.grad = None
    return n


def ref_forward(net, x, index=None, mean=None, std=None, eps=1e-5, dtype=None):
    import torch
    dtype = dtype or torch.float64
    xs = x.to(dtype) if index is None else x.to(dtype)[index]
    if mean is not None:
        xs = (xs - mean.to(dtype)) / (std.to(dtype) + eps)
    with torch.no_grad():
        return net_as(net, dtype)(xs)


def ref_ppo(net, x, act, adv, logp_old, log_std, clip=CLIP, dtype=None):
    """compute_loss_pi (algs/ppo/ppo.py:22-40) through autograd -> (flat gradient, [loss sum, ratio sum, kl sum, count])"""
    import torch
    dtype = dtype or torch.float64
    n = net_as(net, dtype)
    d = torch.distributions.Normal(n(x.to(dtype)), torch.exp(log_std.to(dtype)))
    ratio = torch.exp(d.log_prob(act.to(dtype)).sum(-1) - logp_old.to(dtype))
    a = adv.to(dtype)
    per = -torch.min(ratio * a, a * torch.clamp(ratio, 1 - clip, 1 + clip))
    per.mean().backward()
    grad = torch.cat([p.grad.reshape(-1) for p in n.parameters()])
    kl = (0.5 * (d.mean - act.to(dtype)) ** 2 / d.stddev ** 2).sum()
    B = torch.tensor(float(x.shape[0]), device=x.device, dtype=dtype)
    return grad.double(), torch.stack([per.sum().detach(), ratio.sum().detach(), kl.detach(), B]).double()


def ref_mse(net, x, target, index=None, dtype=None):
    """compute_loss_v (algs/iwpg/iwpg.py:272-275) through autograd -> (flat gradient, sum of squared errors)"""
    import torch
    dtype = dtype or torch.float64
    n = net_as(net, dtype)
    xs, ts = (x.to(dtype), target.to(dtype)) if index is None else (x.to(dtype)[index], target.to(dtype)[index])
    err = (n(xs).squeeze(-1) - ts) ** 2
    err.mean().backward()
    return torch.cat([p.grad.reshape(-1) for p in n.parameters()]).double(), err.sum().detach().double()


def ppo_inputs(net, B, seed):
    import math
    import torch
    d_in = net[0].in_features
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, d_in, device="cuda", generator=g)
    with torch.no_grad():
        mu0 = net(x)
        A = mu0.shape[1]
        log_std = math.log(0.3) + 0.1 * torch.randn(A, device="cuda", generator=g)
        act = mu0 + torch.exp(log_std) * torch.randn(B, A, device="cuda", generator=g)
        logp_old = torch.distributions.Normal(mu0, torch.exp(log_std)).log_prob(act).sum(-1)
        logp_old = logp_old + 0.3 * torch.randn(B, device="cuda", generator=g)  # ratios on both sides of the clip range
    adv = torch.randn(B, device="cuda", generator=g)
    return x, act, adv, logp_old, log_std


# ---- the bar ------------------------------------------------------------------------------------------------------------------
def within(got, want, f32, rtol, atol):
    """-> (passes, ratio to the bar that applied, which side: "two-layer" or "4-unit").  got / want / f32: the kernel's result,
    the float64 reference and its float32 restatement (tensors or floats)."""
    import torch
    got, want, f32 = (torch.as_tensor(t, dtype=torch.float64).reshape(-1).cpu() for t in (got, want, f32))
    err = (got - want).abs()
    two = float((err / (atol + rtol * want.abs())).max())
    if two <= 1.0:
        return True, two, "two-layer"
    unit = float((f32 - want).abs().max())
    four = float(err.max()) / (BAR_UNITS * unit) if unit > 0 else float("inf")
    return four <= 1.0, four, "4-unit"


def check_all(parts):
    """parts: (name, got, want, f32, rtol, atol) -> (the largest ratio to the bar that applied, the sides that applied); asserts
    every part"""
    worst, sides = 0.0, set()
    for name, got, want, f32, rtol, atol in parts:
        ok, ratio, side = within(got, want, f32, rtol, atol)
        print(f"{name}: {ratio:.3f} of the {side} bar")
        assert ok, (name, ratio, side)
        worst, sides = max(worst, ratio), sides | {side}
    return worst, "4-unit" if "4-unit" in sides else "two-layer"


def ppo_parts(got, st, want, wst, fgrad, fst, B):
    """the bars of _check_ppo (tests/test_gpu_mlp_dispatch.py) as parts of check_all; the sample count is exact"""
    assert float(st[3]) == B
    loss, ratio, kl = float(wst[0]) / B, float(wst[1]) / B, float(wst[2])
    return [("grad", got, want, fgrad, 2e-4, mc.grad_atol(want, B)),
            ("loss", float(st[0]) / B, loss, float(fst[0]) / B, 0.0, 2e-5 * max(1.0, abs(loss))),
            ("ratio", float(st[1]) / B, ratio, float(fst[1]) / B, 0.0, 2e-5 * ratio),
            ("kl", float(st[2]), kl, float(fst[2]), 0.0, 1e-5 * kl)]


def mse_parts(got, st, want, sse, fgrad, fsse, n):
    """the bars of _check_mse as parts of check_all"""
    loss = float(sse) / n
    return [("grad", got, want, fgrad, 2e-4, mc.grad_atol(want, n)),
            ("loss", float(st[0]) / n, loss, float(fsse) / n, 0.0, 1e-5 * max(1.0, loss))]
