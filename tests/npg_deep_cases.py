"""Helpers for tests/test_gpu_npg_deep.py and its CPU companion tests/test_npg_deep_cpu.py: the case table of the natural-gradient
kernels for actors with three and four hidden layers (csrc/pds_npg_deep.hip: fvp_deep_kernel<ACT, L>, surrogate_deep_kernel<ACT, L>),
the float64 references and the bars.  Everything that works on any nn.Sequential is tests/npg_cases.py's and used as it is
(fvp_autograd, ref_fvp, jacobian64, ref_fvp_dense, ref_ls, ls_merged_bars, LS_FRACS and the constants of the Fisher bar); what is
restated here for L layers: the networks, near_kink, cancel_depth, the slices of the flat layout and the per-tensor bar by the
tensor's POSITION in the network.  torch is imported lazily.

Flat parameter layout everywhere: W1 [h1, d_in], b1, ..., W(L+1) [d_out, hL], b(L+1) (torch parameter order)."""
import math
import os
import re
from collections import namedtuple

import mlp_cases as mc
import mlp_deep_cases as dc
import npg_cases as nc

NPG_DEEP_SOURCE = os.path.join(mc.CSRC, "pds_npg_deep.hip")
TILE = mc.TILE
MAX_BLOCKS = 256  # kNpgDeepMaxBlocks
MAX_WAVES = 4     # kNpgDeepMaxWaves


def source_constants():
    """(kNpgDeepMaxBlocks, kNpgDeepMaxWaves, waves of the Fisher kernel at L = 4) from the text of csrc/pds_npg_deep.hip"""
    with open(NPG_DEEP_SOURCE) as f:
        text = f.read()
    blocks = int(re.search(r"constexpr int kNpgDeepMaxBlocks = (\d+);", text).group(1))
    waves = int(re.search(r"constexpr int kNpgDeepMaxWaves = (\d+);", text).group(1))
    w4 = int(re.search(r"constexpr int fvp_deep_waves\(\) \{ return L == 4 \? (\d+) : kNpgDeepMaxWaves; \}", text).group(1))
    return blocks, waves, w4


def waves(kind, depth):
    """the Fisher kernel at depth 4 runs three waves per block (LDS), everything else four"""
    return 3 if kind == "fvp" and depth == 4 else MAX_WAVES


def tail(kind, depth):
    """a ragged batch past the second round of the persistent grid"""
    return 2 * MAX_BLOCKS * waves(kind, depth) * TILE + 53


# kind: "fvp" | "ls"; index (fvp): None | "perm" | "rep" over rows = 2 B + 3, the rows that are not indexed hold NaN
Case = namedtuple("Case", "kind d_in hidden d_out act B index")
SHAPES = [dc.SHAPES3[0], dc.SHAPES3[3], dc.SHAPES3[4], dc.SHAPES3[7], dc.SHAPES3[9],
          dc.SHAPES4[0], dc.SHAPES4[2], dc.SHAPES4[4], dc.SHAPES4[6]]
TINY = nc.TINY            # (1, 15, 16, 17, 65)
DENSE_MAX = nc.DENSE_MAX  # ref_fvp_dense up to here
INDEX = (None, "perm", "rep")
ACTS = ("relu", "tanh")
N_FVP_CASES, N_LS_CASES = 22, 13  # literal: the table cannot shrink unnoticed


def _case_table():
    cases = []
    for i, (d, hid, o) in enumerate(SHAPES):  # every shape under both activations, at two of the tiny batches
        cases.append(Case("fvp", d, hid, o, ACTS[i % 2], TINY[i % 5], INDEX[i % 3]))
        cases.append(Case("fvp", d, hid, o, ACTS[(i + 1) % 2], TINY[(i + 2) % 5], INDEX[(i + 1) % 3]))
    # past the second round of the grid, per depth: the architecture search's two actors, the other activation and an index each
    cases += [Case("fvp", 34, (50, 30, 20), 4, "relu", tail("fvp", 3), "rep"), Case("fvp", 34, (32, 32, 32, 32), 4, "tanh", tail("fvp", 4), None),
              Case("fvp", 48, (16, 64, 33), 2, "tanh", tail("fvp", 3), "perm"), Case("fvp", 40, (50, 30, 20, 10), 4, "relu", tail("fvp", 4), "perm")]
    for i, (d, hid, o) in enumerate(SHAPES):
        cases.append(Case("ls", d, hid, o, ACTS[(i + 1) % 2], TINY[(i + 3) % 5], None))
    cases += [Case("ls", 34, (50, 30, 20), 4, "relu", tail("ls", 3), None), Case("ls", 34, (32, 32, 32, 32), 4, "tanh", tail("ls", 4), None),
              Case("ls", 64, (64, 64, 64), 8, "tanh", tail("ls", 3), None), Case("ls", 40, (50, 30, 20, 10), 4, "relu", tail("ls", 4), None)]
    return cases


CASES = _case_table()
FVP_CASES = [c for c in CASES if c.kind == "fvp"]
LS_CASES = [c for c in CASES if c.kind == "ls"]
LS_FRACS = nc.LS_FRACS


def case_id(c):
    return f"{c.kind}-{c.d_in}x{'x'.join(map(str, c.hidden))}x{c.d_out}-{c.act}-B{c.B}" + (f"-{c.index}" if c.index else "")


def case_seed(c):
    return 300 + CASES.index(c)


def dims(c):
    return [c.d_in] + list(c.hidden) + [c.d_out]


def param_count(c):
    d = dims(c)
    return sum(d[j + 1] * d[j] + d[j + 1] for j in range(len(d) - 1))


def tensors(c):
    return [n for j in range(len(c.hidden) + 1) for n in (f"W{j + 1}", f"b{j + 1}")]


def slices(c):
    """name -> slice of the flat layout"""
    out, off, d = {}, 0, dims(c)
    for j in range(len(d) - 1):
        for name, n in ((f"W{j + 1}", d[j + 1] * d[j]), (f"b{j + 1}", d[j + 1])):
            out[name] = slice(off, off + n)
            off += n
    return out


def position(name, c):
    """a tensor's position in the network: first / inner / out weight or bias"""
    j = int(name[1:])
    return name[0] + ("_first" if j == 1 else "_out" if j == len(c.hidden) + 1 else "_inner")


# ---- networks and inputs (the recipe of npg_cases.make_net / make_inputs, for L hidden layers) ---------------------------------
def make_net(c, seed, device):
    """nn.Sequential(Linear, act, ..., Linear, Identity) with the reference's layer initialisation"""
    import torch
    from torch import nn
    g = torch.Generator().manual_seed(seed)
    act = {"relu": nn.ReLU, "tanh": nn.Tanh}[c.act]
    sizes, layers = dims(c), []
    for j in range(len(sizes) - 1):
        lin = nn.Linear(sizes[j], sizes[j + 1])
        bound = 1.0 / math.sqrt(sizes[j])  # kaiming_uniform_(a = sqrt 5) and the bias range of nn.Linear
        with torch.no_grad():
            lin.weight.copy_((torch.rand(lin.weight.shape, generator=g) * 2 - 1) * bound)
            lin.bias.copy_((torch.rand(lin.bias.shape, generator=g) * 2 - 1) * bound)
        layers += [lin, act() if j < len(sizes) - 2 else nn.Identity()]
    return nn.Sequential(*layers).to(device)


KINK = nc.KINK  # 2^-18


def near_kink(net, xs):
    """bool [B]: samples of xs with a hidden pre-activation |z| < KINK in float64, at any of the L hidden layers"""
    import torch
    n64 = nc.net64(net)
    lin = [m for m in n64 if isinstance(m, torch.nn.Linear)]
    bad = torch.zeros(xs.shape[0], dtype=torch.bool)
    with torch.no_grad():
        h = xs.double()
        for j, l in enumerate(lin[:-1]):
            z = l(h)
            bad |= (z.abs() < KINK).any(-1)
            h = n64[2 * j + 1](z)
    return bad


def make_inputs(c, device):
    """-> dict(net, x, index, xs, log_std, v [fvp] | s, act, adv, logp_old, mu_old, theta [ls], kink_redraws, kink_left).  xs: the B
    rows the operation sees.  Drawn on the CPU from the case's seed, so that a device and a CPU run see the same numbers.  For a relu
    net the rows that land near a kink are drawn again, up to 20 rounds (kink_left: how many were still near one, asserted zero by
    the CPU test): the table holds no such sample and the Fisher bars need no kink allowance."""
    import torch
    seed = case_seed(c)
    net = make_net(c, seed, "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    xs = torch.randn(c.B, c.d_in, generator=g)
    redraws = left = 0
    if c.act == "relu":
        for _ in range(20):
            bad = near_kink(net, xs)
            nb = int(bad.sum())
            if nb == 0:
                break
            redraws += nb
            xs[bad] = torch.randn(nb, c.d_in, generator=g)
        left = int(near_kink(net, xs).sum())
    P = param_count(c)
    log_std = torch.linspace(-1.2, -0.4, c.d_out, device=device)  # every output its own sigma
    out = dict(net=net, log_std=log_std, kink_redraws=redraws, kink_left=left)
    if c.kind == "fvp":
        v = torch.randn(P, generator=g)
        if c.index is None:
            x, index = xs, None
        else:
            rows = 2 * c.B + 3
            index = nc.make_index(c.index, rows, c.B, seed + 2, "cpu")
            x = torch.full((rows, c.d_in), float("nan"))
            if c.index == "rep":  # repeated entries: the rows are the samples, xs follows from them
                uniq = torch.unique(index)
                x[uniq] = xs[:uniq.numel()]
                xs = x[index]
            else:
                x[index] = xs
            index = index.to(device)
        out.update(x=x.to(device), index=index, xs=xs.to(device), v=v.to(device))
    else:
        A = c.d_out
        theta = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).to(device)
        s = 0.05 * torch.randn(P, generator=g)
        with torch.no_grad():
            mu_old = net(xs).to(device)
        sigma = torch.exp(log_std)
        act_t = mu_old + sigma * torch.randn(c.B, A, generator=g).to(device)
        adv = torch.randn(c.B, generator=g).to(device)
        logp_old = torch.distributions.Normal(mu_old, sigma).log_prob(act_t).sum(-1) + 0.01
        out.update(x=xs.to(device), xs=xs.to(device), index=None, theta=theta, s=s.to(device), act=act_t.contiguous(),
                   adv=adv, logp_old=logp_old.contiguous(), mu_old=mu_old.contiguous())
    net.to(device)
    return out


# ---- references ---------------------------------------------------------------------------------------------------------------
def cancel_depth(c):
    """summation depth of one inner product J_ij . v as the kernel forms it: the tangent pass adds d_in + 1 terms in layer 1
    (V x + vb), 2 h_(l-1) + 1 in every later hidden layer and 2 h_L + 1 in the output layer (V h + W t + vb), one chain after the
    other"""
    return (c.d_in + 1) + sum(2 * h + 1 for h in c.hidden)


def gn_fvp(net, x, log_std, v, slip=None):
    """F v in float64 by the recurrence the kernel runs, written out: per hidden layer z = W_l h_(l-1), dz = W_l t_(l-1) +
    V_l h_(l-1) + vb_l (t_0 = 0), h_l = act(z + b_l), t_l = act'(h_l) dz; dmu = W_o t_L + V_o h_L + vb_o; u = dmu exp(-2 log_std);
    J^T u by one backward pass; scale 1 / (B d_out).  slip: a deliberate mistake, for the teeth of the reference --
    ("drop", l): no W_l t_(l-1) term at hidden layer l (1-based, l >= 2); ("act", l): act' of layer l - 1 at layer l (equal widths);
    "sigma": exp(-log_std); "scale": 1 / B."""
    import torch
    n64 = nc.net64(net)
    lin = [m for m in n64 if isinstance(m, torch.nn.Linear)]
    L = len(lin) - 1
    relu = isinstance(n64[1], torch.nn.ReLU)
    act = torch.relu if relu else torch.tanh
    dact = (lambda h: (h > 0).double()) if relu else (lambda h: 1 - h * h)
    v = v.double()
    Vs, off = [], 0
    for l in lin:
        nw, nb = l.weight.numel(), l.bias.numel()
        Vs.append((v[off:off + nw].view_as(l.weight), v[off + nw:off + nw + nb]))
        off += nw + nb
    with torch.no_grad():
        h = x.double()
        t = torch.zeros_like(h)
        prev_d = None
        for j in range(L):
            W, b = lin[j].weight, lin[j].bias
            V, vb = Vs[j]
            dz = h @ V.t() + vb
            if j > 0 and slip != ("drop", j + 1):
                dz = dz + t @ W.t()
            h = act(h @ W.t() + b)
            d = dact(h)
            t = (prev_d if slip == ("act", j + 1) else d) * dz
            prev_d = d
        dmu = t @ lin[L].weight.t() + h @ Vs[L][0].t() + Vs[L][1]
        u = dmu * torch.exp((-1.0 if slip == "sigma" else -2.0) * log_std.double())
    mu = n64(x.double())
    jtu = torch.autograd.grad((mu * u).sum(), list(n64.parameters()))
    B, A = mu.shape
    return torch.cat([g.reshape(-1) for g in jtu]) / (B if slip == "scale" else B * A)


# ---- bars ---------------------------------------------------------------------------------------------------------------------
FVP_REL, TENSOR_FACTOR, TENSOR_FLOOR = nc.FVP_REL, nc.TENSOR_FACTOR, nc.TENSOR_FLOOR  # 2e-5, 8, 2^-21: the project's own

# The largest rho = |f32 autograd - ref_fvp| / |ref_fvp| per tensor position over the table above: torch's float32 double backward
# (the operation npg.py runs without deep_fused) on the same inputs, measured on the MI355X by profiles/tools/npg_deep_margins.py
# (profiles/npg_deep_parity_margins.txt).  The rank-one cases (B = 1, d_out = 1), whose error is the cancellation term's, are left
# out of the maxima, as in npg_cases.F32_AUTOGRAD_RHO.
F32_AUTOGRAD_RHO = {"W_first": 1.138e-06, "b_first": 1.985e-07, "W_inner": 2.342e-06, "b_inner": 2.446e-07, "W_out": 1.186e-06, "b_out": 1.563e-07}
# The kernel's own maxima per position, for the record (same run): 5.8e-07, 5.7e-07, 5.3e-07, 5.1e-07, 7.2e-07, 4.4e-07 -- 0.03 to 0.36
# of the bars these maxima give, so no family needs an override.
# families whose measured kernel rho exceeds TENSOR_FACTOR x the float32-autograd rho, with the excess accounted for in
# profiles/npg_deep_parity_margins.txt: (position, predicate on the case, twice the measured value); never above FVP_REL
TENSOR_OVERRIDES = []


def cancel_applies(c):
    """npg_cases.cancel_applies: the cancellation term is added for the rank-one case (one sample, one output) and nowhere else"""
    return c.B * c.d_out == 1


def fvp_tensor_rel(name, c, live=None):
    """relative bar of one parameter tensor (npg_cases.fvp_tensor_rel's rule): 8 x the larger of float32 autograd's rho on this
    case's inputs (`live`) and the table-wide maximum for the tensor's position, within [2^-21, 2e-5]"""
    pos = position(name, c)
    for pname, pred, rel in TENSOR_OVERRIDES:
        if pname == pos and pred(c):
            return min(rel, FVP_REL)
    rho = max(F32_AUTOGRAD_RHO[pos], live[name] if live else 0.0)
    return min(max(TENSOR_FACTOR * rho, TENSOR_FLOOR), FVP_REL)


def fvp_bars(c, want, cancel=None, live=None):
    """-> (whole-vector absolute bar, {tensor: absolute bar}).  cancel: the element-wise cancellation term of ref_fvp_dense; live:
    float32 autograd's rho per tensor on this case's inputs.  A tensor whose float64 value is exactly zero has a bar of zero."""
    import torch
    use = cancel is not None and cancel_applies(c)
    whole = FVP_REL * float(torch.norm(want)) + (float(torch.norm(cancel)) if use else 0.0)
    per = {}
    for name, sl in slices(c).items():
        per[name] = fvp_tensor_rel(name, c, live) * float(torch.norm(want[sl])) + (float(torch.norm(cancel[sl])) if use else 0.0)
    return whole, per


def tensor_rho(got, want, c):
    """{tensor: |got - want| / |want|}; 0 where both are exactly zero, inf where only want is"""
    import torch
    out = {}
    for name, sl in slices(c).items():
        e, w = float(torch.norm(got[sl].double() - want[sl])), float(torch.norm(want[sl]))
        out[name] = e / w if w > 0 else (0.0 if e == 0 else float("inf"))
    return out


def fvp_margins(c, got, want, cancel, live):
    """error / bar over the whole vector and per tensor (comparisons are <=: 0 / 0 counts as 0, e / 0 as inf)"""
    import torch
    whole, per = fvp_bars(c, want, cancel, live)

    def ratio(e, b):
        return e / b if b > 0 else (0.0 if e == 0 else float("inf"))

    out = {"whole": ratio(float(torch.norm(got.double() - want)), whole)}
    for name, sl in slices(c).items():
        out[name] = ratio(float(torch.norm(got[sl].double() - want[sl])), per[name])
    return out


def cg64(avp, b, nsteps, residual_tol=1e-10, eps=1e-6):
    """conjugate_gradients (algs/utils.py:5-38) in the dtype of b, from x = 0"""
    x = b * 0
    r = b.clone()
    p = r.clone()
    rdotr = r @ r
    for _ in range(nsteps):
        z = avp(p)
        alpha = rdotr / (p @ z + eps)
        x = x + alpha * p
        r = r - alpha * z
        new = r @ r
        if math.sqrt(float(new)) < residual_tol:
            break
        p = r + new / (rdotr + eps) * p
        rdotr = new
    return x
