"""Helpers for tests/test_gpu_npg_kernels.py and its CPU companion tests/test_npg_oracle_cpu.py: the case table of the
natural-gradient kernels of csrc/pds_npg.hip (fvp_kernel<ACT, NIN>, surrogate_kernel<ACT, NIN>, cg_kernel and the two reduce
kernels), a Python restatement of the host predicate that picks NIN, float64 references of the three operations, and the
bars the kernels are held to, each with its derivation.  torch is imported lazily (the table and the mirror need none).

Flat parameter layout everywhere: W1 [h1, d_in], b1, W2 [h2, h1], b2, W3 [d_out, h2], b3 (torch parameter order)."""
import math
import os
import re
from collections import namedtuple

import mlp_cases as mc

NPG_SOURCE = os.path.join(mc.CSRC, "pds_npg.hip")
EPS32 = 2.0 ** -24  # unit roundoff of float32

# ---- dispatch mirror: launch_fvp / launch_surrogate --------------------------------------------------------------------
NIN_THRESHOLDS = (2, 4, 8)  # `nin <= 2`, `nin <= 4`, `nin <= 8`, else 12
NINS = (2, 4, 8, 12)


def nin_of(d_in):
    """the NIN template argument launch_fvp / launch_surrogate pick: nin = ceil(d_in / 16) against the `<=` chain"""
    nin = (d_in + mc.TILE - 1) // mc.TILE
    for t in NIN_THRESHOLDS:
        if nin <= t:
            return t
    return 12


def source_thresholds():
    """per launcher of pds_npg.hip: the (`nin <= T`, NIN launched) pairs and the NIN of the final else, from the source text"""
    with open(NPG_SOURCE) as f:
        text = f.read()
    out = {}
    for name, kernel in (("launch_fvp", "fvp_kernel"), ("launch_surrogate", "surrogate_kernel")):
        body = text[text.index(f"static void {name}("):]
        body = body[:body.index("\n}\n")]
        pairs = [(int(a), int(b)) for a, b in re.findall(rf"if \(nin <= (\d+)\) hipLaunchKernelGGL\(\({kernel}<ACT, (\d+)>\)", body)]
        last = re.findall(rf"else hipLaunchKernelGGL\(\({kernel}<ACT, (\d+)>\)", body)
        out[name] = (pairs, [int(v) for v in last])
    return out


# ---- the case table -----------------------------------------------------------------------------------------------------
# kind: "fvp" | "ls"; index (fvp): None | "perm" | "rep" over rows = 2 B + 3, the rows that are not indexed hold NaN
Case = namedtuple("Case", "kind d_in h1 h2 d_out act B index")
TAIL = 2 * mc.WIDE_ROUND + 53  # a ragged batch past two rounds of the persistent grid (256 blocks x 4 waves x 16 samples)
TINY = (1, 15, 16, 17, 65)     # 65: five tiles, two blocks, three waves of the second block without a tile
BIG = 131072                   # exactly eight rounds
DENSE_MAX = 65                 # ref_fvp_dense (one Jacobian row per sample and output) up to here

FVP_SHAPES = [  # (d_in, h1, h2, d_out, act): per NIN both orders of h1 != h2 and both activations; then the trainer's shapes
    (1, 16, 17, 1, "relu"), (16, 63, 33, 2, "tanh"), (17, 49, 48, 3, "relu"), (32, 17, 64, 5, "tanh"),     # NIN 2
    (33, 50, 49, 6, "relu"), (47, 33, 63, 7, "tanh"), (64, 64, 1, 8, "relu"),                               # NIN 4
    (65, 48, 16, 3, "tanh"), (128, 1, 50, 4, "relu"),                                                       # NIN 8
    (129, 17, 48, 8, "relu"), (191, 64, 63, 2, "tanh"), (192, 16, 33, 5, "tanh"),                           # NIN 12
    (34, 50, 50, 4, "relu"), (42, 50, 50, 4, "tanh"), (40, 50, 50, 4, "relu"), (48, 50, 50, 4, "tanh"),
    (34, 64, 64, 4, "tanh")]
LS_SHAPES = [
    (16, 16, 17, 1, "relu"), (32, 33, 63, 2, "tanh"), (33, 49, 33, 5, "tanh"), (42, 50, 50, 4, "relu"),
    (65, 63, 48, 8, "relu"), (128, 17, 64, 6, "tanh"), (129, 48, 16, 3, "relu"), (192, 64, 50, 7, "tanh")]
N_FVP_CASES, N_LS_CASES = 36, 16  # literal: the table cannot shrink unnoticed


def _case_table():
    cases = []
    for i, (d, h1, h2, o, act) in enumerate(FVP_SHAPES):
        cases.append(Case("fvp", d, h1, h2, o, act, TINY[i % 5], (None, "perm", "rep")[i % 3]))
        cases.append(Case("fvp", d, h1, h2, o, act, TAIL, (None, "perm", "rep")[(i + 1) % 3]))
    cases += [Case("fvp", 68, 16, 16, 1, "tanh", BIG, None), Case("fvp", 42, 50, 50, 4, "relu", BIG, None)]
    for i, (d, h1, h2, o, act) in enumerate(LS_SHAPES):
        cases.append(Case("ls", d, h1, h2, o, act, TINY[(i + 2) % 5], None))
        cases.append(Case("ls", d, h1, h2, o, act, TAIL, None))
    return cases


CASES = _case_table()
FVP_CASES = [c for c in CASES if c.kind == "fvp"]
LS_CASES = [c for c in CASES if c.kind == "ls"]
LS_FRACS = [0.0, 1.0, 0.8, 0.8 ** 7, -0.5, float("inf")]
CG_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 5000, 16968)  # 16968: the largest parameter count (192 x 64 x 64 x 8)
TENSORS = ("W1", "b1", "W2", "b2", "W3", "b3")


def case_id(c):
    return f"{c.kind}-{c.d_in}x{c.h1}x{c.h2}x{c.d_out}-{c.act}-B{c.B}" + (f"-{c.index}" if c.index else "")


def case_seed(c):
    return 100 + CASES.index(c)


def param_count(c):
    return c.h1 * c.d_in + c.h1 + c.h2 * c.h1 + c.h2 + c.d_out * c.h2 + c.d_out


def slices(c):
    """name -> slice of the flat layout"""
    out, off = {}, 0
    for name, n in zip(TENSORS, (c.h1 * c.d_in, c.h1, c.h2 * c.h1, c.h2, c.d_out * c.h2, c.d_out)):
        out[name] = slice(off, off + n)
        off += n
    return out


# ---- networks and inputs ------------------------------------------------------------------------------------------------
def make_net(c, seed, device):
    """nn.Sequential(Linear, act, Linear, act, Linear, Identity) with the reference's layer initialisation"""
    import torch
    from torch import nn
    g = torch.Generator().manual_seed(seed)
    act = {"relu": nn.ReLU, "tanh": nn.Tanh}[c.act]
    sizes, layers = [c.d_in, c.h1, c.h2, c.d_out], []
    for j in range(3):
        lin = nn.Linear(sizes[j], sizes[j + 1])
        bound = 1.0 / math.sqrt(sizes[j])  # kaiming_uniform_(a = sqrt 5) and the bias range of nn.Linear
        with torch.no_grad():
            lin.weight.copy_((torch.rand(lin.weight.shape, generator=g) * 2 - 1) * bound)
            lin.bias.copy_((torch.rand(lin.bias.shape, generator=g) * 2 - 1) * bound)
        layers += [lin, act() if j < 2 else nn.Identity()]
    return nn.Sequential(*layers).to(device)


def net64(net):
    import copy
    return copy.deepcopy(net).double()


def log_std_of(c, device):
    import torch
    return torch.linspace(-1.2, -0.4, c.d_out, device=device)  # every output its own sigma


KINK = 2.0 ** -18  # a sample is near a relu kink when a hidden pre-activation of the float64 reference is below this


def near_kink(net, xs):
    """bool [B]: samples of xs with a hidden pre-activation |z| < KINK in float64"""
    import torch
    n64 = net64(net)
    with torch.no_grad():
        z1 = n64[0](xs.double())
        z2 = n64[2](n64[1](z1))
    return (z1.abs() < KINK).any(-1) | (z2.abs() < KINK).any(-1)


def make_index(kind, rows, B, seed, device):
    """mlp_cases.make_index on any device: a permutation slice of `rows`, or B entries with repeats from the first rows"""
    import torch
    if str(device).startswith("cuda"):
        return mc.make_index(kind, rows, B, seed)
    g = torch.Generator().manual_seed(seed)
    if kind == "perm":
        return torch.randperm(rows, generator=g)[:B]
    return torch.randint(0, max(rows // 2, 1), (B,), generator=g)


def make_inputs(c, device):
    """-> dict(net, x, index, xs, log_std, v [fvp] | s, act, adv, logp_old, mu_old, theta [ls]).  xs: the B rows the
    operation sees.  Drawn on the CPU from the case's seed, so that a device and a CPU run see the same numbers.  For a
    relu net the rows that land near a kink are drawn again (kink_redraws of them): the table holds no such sample, which is
    the cap of the issue at its strictest, and fvp_bars needs no kink allowance."""
    import torch
    seed = case_seed(c)
    net = make_net(c, seed, "cpu")
    g = torch.Generator().manual_seed(seed + 1)
    xs = torch.randn(c.B, c.d_in, generator=g)
    redraws = 0
    if c.act == "relu":
        for _ in range(20):
            bad = near_kink(net, xs)
            nb = int(bad.sum())
            if nb == 0:
                break
            redraws += nb
            xs[bad] = torch.randn(nb, c.d_in, generator=g)
    P = param_count(c)
    out = dict(net=net, log_std=log_std_of(c, device), kink_redraws=redraws)
    if c.kind == "fvp":
        v = torch.randn(P, generator=g)
        if c.index is None:
            x, index = xs, None
        else:
            rows = 2 * c.B + 3
            index = make_index(c.index, rows, c.B, seed + 2, "cpu")
            x = torch.full((rows, c.d_in), float("nan"))
            if c.index == "rep":  # repeated entries: the rows are the samples, xs follows from them
                uniq = torch.unique(index)
                x[uniq] = xs[:uniq.numel()]
                xs = x[index]
                if c.act == "relu":
                    assert not bool(near_kink(net, xs).any())
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
        sigma = torch.exp(out["log_std"])
        act_t = mu_old + sigma * torch.randn(c.B, A, generator=g).to(device)
        adv = torch.randn(c.B, generator=g).to(device)
        logp_old = torch.distributions.Normal(mu_old, sigma).log_prob(act_t).sum(-1) + 0.01
        out.update(x=xs.to(device), xs=xs.to(device), index=None, theta=theta, s=s.to(device), act=act_t.contiguous(),
                   adv=adv, logp_old=logp_old.contiguous(), mu_old=mu_old.contiguous())
    net.to(device)
    return out


# ---- references ---------------------------------------------------------------------------------------------------------
def fvp_autograd(net, x, log_std, v, dtype):
    """NaturalPolicyGradientAlgorithm.Fvp (algs/npg/npg.py:52-77) without the damping, in `dtype`: the double backward of
    KL(p_old || p_theta).mean() at theta = theta_old"""
    import copy
    import torch
    n = copy.deepcopy(net).to(dtype)
    ps = list(n.parameters())
    std = torch.exp(log_std.to(dtype))
    q = torch.distributions.Normal(n(x.to(dtype)), std)
    with torch.no_grad():
        p = torch.distributions.Normal(n(x.to(dtype)), std)
    kl = torch.distributions.kl.kl_divergence(p, q).mean()
    g = torch.cat([t.reshape(-1) for t in torch.autograd.grad(kl, ps, create_graph=True)])
    return torch.cat([t.reshape(-1) for t in torch.autograd.grad((g * v.to(dtype)).sum(), ps)])


def ref_fvp(net, x, log_std, v):
    import torch
    return fvp_autograd(net, x, log_std, v, torch.float64)


def jacobian64(net, x):
    """J [B * A, P]: row i A + j = d mu_j(x_i) / d theta in float64 autograd"""
    import torch
    n64 = net64(net)
    ps = list(n64.parameters())
    mu = n64(x.double()).reshape(-1)
    rows = []
    for k in range(mu.numel()):
        gr = torch.autograd.grad(mu[k], ps, retain_graph=True)
        rows.append(torch.cat([t.reshape(-1) for t in gr]))
    return torch.stack(rows)


def cancel_depth(c):
    """summation depth of one inner product J_ij . v as the kernel forms it: the tangent pass adds d_in + 1, h1 + h1 + 1 and
    h2 + h2 + 1 terms in its three layers (V x + vb; V h + W t + vb), one chain after the other"""
    return (c.d_in + 1) + (2 * c.h1 + 1) + (2 * c.h2 + 1)


def ref_fvp_dense(net, x, log_std, v, depth):
    """the Gauss-Newton form written out, 1 / (B A) sum_i J_i^T diag(exp(-2 log_std)) J_i v, from jacobian64; B <= DENSE_MAX.
    -> (F v, cancellation term).  The cancellation term is element-wise: float32 forms J_ij . v with an error of at most
    depth eps sum_k |J_ijk v_k| (first order), and that error goes through 1 / sigma_j^2, J_ij^T and the 1 / (B A) scale like
    the value itself: e = 1 / (B A) sum_ij |J_ij| exp(-2 log_std_j) depth eps (|J_ij| . |v|).  For one sample and one output
    its norm is the allowance the one-sample test has always had, depth eps sum |j v| |j| / sigma^2, with the kernel's own
    summation depth (cancel_depth) in place of the parameter count."""
    import torch
    B = x.shape[0]
    assert B <= DENSE_MAX
    J = jacobian64(net, x)
    A = J.shape[0] // B
    w = torch.exp(-2 * log_std.double()).repeat(B)
    fv = J.t() @ (w * (J @ v.double())) / (B * A)
    e = J.abs().t() @ (w * (depth * EPS32) * (J.abs() @ v.double().abs())) / (B * A)
    return fv, e


def set_flat64(n64, theta):
    import torch
    off = 0
    with torch.no_grad():
        for p in n64.parameters():
            p.copy_(theta[off:off + p.numel()].view_as(p).double())
            off += p.numel()


def ref_ls(net, theta_c, x, act, adv, logp_old, mu_old, log_std, sigma_of=None):
    """one line-search candidate in float64 at the float32 parameters theta_c -> dict(ra = sum ratio adv, kl = sum of
    KL(Normal(mu_old, sigma) || Normal(mu, sigma)) over samples x outputs, rs = sum ratio, scale = sum |ratio adv|)"""
    import torch
    n64 = net64(net)
    set_flat64(n64, theta_c)
    with torch.no_grad():
        mu = n64(x.double())
        std = torch.exp(log_std.double())
        lp = torch.distributions.Normal(mu, std).log_prob(act.double()).sum(-1)
        ratio = torch.exp(lp - logp_old.double())
        kl = torch.distributions.kl.kl_divergence(torch.distributions.Normal(mu_old.double(), std),
                                                  torch.distributions.Normal(mu, std)).sum()
        ra = ratio * adv.double()
    return dict(ra=float(ra.sum()), kl=float(kl), rs=float(ratio.sum()), scale=float(ra.abs().sum()))


def ref_cg_step(x, r, p, z, st, eps, tol, init):
    """ONE launch of cg_kernel in float64 from the float32 state it is given (tensors or arrays; z = A p, or b when init)
    -> dict(x, r, p, st = [r.r, stopped]) and the intermediate alpha, mu, pz, nr the bars are built from"""
    import numpy as np
    x, r, p, z = (np.asarray(t.detach().cpu() if hasattr(t, "detach") else t, dtype=np.float64) for t in (x, r, p, z))
    st = np.asarray(st.detach().cpu() if hasattr(st, "detach") else st, dtype=np.float64)
    if init:
        return dict(x=np.zeros_like(z), r=z.copy(), p=z.copy(), st=np.array([z @ z, 0.0]), stopped_now=False)
    if st[1] != 0.0:
        return dict(x=x.copy(), r=r.copy(), p=p.copy(), st=st.copy(), frozen=True, stopped_now=False)
    pz = p @ z
    alpha = st[0] / (pz + eps)
    xn, rn = x + alpha * p, r - alpha * z
    nr = rn @ rn
    out = dict(x=xn, r=rn, alpha=alpha, pz=pz, nr=nr, p_in=p, z_in=z, eps=eps)
    if math.sqrt(nr) < tol:
        out.update(p=p.copy(), st=np.array([st[0], 1.0]), stopped_now=True)
        return out
    mu = nr / (st[0] + eps)
    out.update(p=rn + mu * p, st=np.array([nr, 0.0]), mu=mu, stopped_now=False)
    return out


# ---- bars ---------------------------------------------------------------------------------------------------------------
FVP_REL = 2e-5  # the whole-vector bar the kernels were merged with

# The largest rho = |f32 autograd - ref_fvp| / |ref_fvp| per tensor kind over the table: torch's float32 double backward (the
# operation npg.py runs with fused=False) on the same inputs, measured on the MI355X (profiles/npg_parity_margins.txt;
# tiny batches are also evaluated inside the GPU test).  The rank-one case (B = 1, d_out = 1), whose error is the
# cancellation term's, is left out of the maxima.
F32_AUTOGRAD_RHO = {"W1": 2.545e-06, "b1": 1.101e-06, "W2": 1.537e-06, "b2": 6.519e-07, "W3": 1.598e-05, "b3": 5.816e-07}
TENSOR_FACTOR = 8.0     # other summation trees: torch's blocked GEMMs against MFMA chains of four plus up to 1024 per-wave
                        # partials added in a fixed order.  A margin over the reference side's number, not the kernel's
TENSOR_FLOOR = 2.0 ** -21
# families whose measured kernel rho exceeds TENSOR_FACTOR x the float32-autograd rho, with the excess accounted for in
# profiles/npg_parity_margins.txt: (tensor, predicate on the case) -> twice the measured value
TENSOR_OVERRIDES = []


def fvp_tensor_rel(name, c=None, live=None):
    """relative bar of one parameter tensor: 8 x the largest float32-autograd rho of its kind -- the table's recorded maximum
    and, where the test evaluated it on the spot (tiny batches), that value `live` too -- within [2^-21, 2e-5]"""
    for tname, pred, rel in TENSOR_OVERRIDES:
        if tname == name and c is not None and pred(c):
            return min(rel, FVP_REL)
    rho = max(F32_AUTOGRAD_RHO[name], live[name] if live else 0.0)
    return min(max(TENSOR_FACTOR * rho, TENSOR_FLOOR), FVP_REL)


def cancel_applies(c):
    """The cancellation term is a worst-case bound: depth eps times a sum of ABSOLUTE values, where F v itself is a sum of
    signed ones.  Measured over the tiny cases it is 2e-4 to 3e-3 of |F v| (profiles/npg_parity_margins.txt), far looser than
    2e-5, and it does not shrink with B; float32 needs it only where F v is a single inner product, F = j j^T / sigma^2 (one
    sample, one output: rank one), the case the allowance was introduced for.  So it is added there and nowhere else: for
    every other case, B >= 4096 included, the allowance is exactly zero and the bars are the 2e-5 and per-tensor terms alone."""
    return c.B * c.d_out == 1


def fvp_bars(c, want, cancel=None, live=None):
    """-> (whole-vector absolute bar, {tensor: absolute bar}).  cancel: the element-wise cancellation term of ref_fvp_dense;
    live: float32 autograd's rho per tensor on this case's inputs"""
    import torch
    use = cancel is not None and cancel_applies(c)
    whole = FVP_REL * float(torch.norm(want)) + (float(torch.norm(cancel)) if use else 0.0)
    per = {}
    for name, sl in slices(c).items():
        per[name] = fvp_tensor_rel(name, c, live) * float(torch.norm(want[sl])) + (float(torch.norm(cancel[sl])) if use else 0.0)
    return whole, per


def tensor_rho(got, want, c):
    import torch
    return {name: float(torch.norm(got[sl].double() - want[sl]) / torch.norm(want[sl])) for name, sl in slices(c).items()}


# line search: the expressions the kernels were merged with -- 1e-5 of sum |ratio adv| (+ 1e-6), 1e-4 of the KL sum plus its
# floor, 1e-5 of the ratio sum -- each times twice the worst error / bar measured over the table on the MI355X: 0.0179, 0.0393
# and 0.0277 (profiles/npg_parity_margins.txt), all more than ten times below the merged bars
LS_TIGHTEN = (2 * 0.0179, 2 * 0.0393, 2 * 0.0277)


def ls_merged_bars(ref, B, A):
    """absolute bars of (sum ratio adv, sum kl, sum ratio) as the kernels were merged with them"""
    return (1e-5 * ref["scale"] + 1e-6, 1e-4 * ref["kl"] + 1e-5 * B * A * 1e-7 + 1e-6, 1e-5 * ref["rs"])


def ls_bars(ref, B, A):
    return tuple(t * b for t, b in zip(LS_TIGHTEN, ls_merged_bars(ref, B, A)))


def cg_dot_depth(n):
    """additions one product goes through in cg_dot: the thread's chain, six butterfly stages, sixteen waves"""
    return -(-n // 1024) + 22


def cg_dot_bar(a, b):
    """first-order bound of cg_dot(a, b): depth eps sum |a_i b_i| (every product rounded once, then `depth` additions)"""
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return cg_dot_depth(a.size) * EPS32 * float(np.abs(a * b).sum())


CG_SLACK = 1.0 + 2.0 ** -10  # the second-order terms of the first-order bounds below


def cg_step_bars(ref):
    """element-wise absolute bars (x, r, p) and the bar of st[0] for one non-init launch, from ref_cg_step's record.
    alpha = rr / (pz + eps): pz within its dot bar, one rounding for the sum and one for the quotient.  x + alpha p and
    r - alpha z: alpha's error times the vector, one rounding of the product (__fmul_rn), one of the sum (__fadd_rn).  nr is the
    dot of the DEVICE's r with itself: its dot bar plus 2 sum |r_i| dr_i.  mu = nr / (rr + eps) and p = r + mu p likewise."""
    import numpy as np
    u = EPS32
    p, z, alpha = ref["p_in"], ref["z_in"], ref["alpha"]
    d_pz = cg_dot_bar(p, z)
    d_alpha = abs(alpha) * (d_pz / abs(ref["pz"] + ref["eps"]) + 3 * u)
    bx = (d_alpha * np.abs(p) + u * np.abs(alpha * p) + u * np.abs(ref["x"])) * CG_SLACK
    br = (d_alpha * np.abs(z) + u * np.abs(alpha * z) + u * np.abs(ref["r"])) * CG_SLACK
    d_nr = (cg_dot_bar(ref["r"], ref["r"]) + 2.0 * float((np.abs(ref["r"]) * br).sum()) + u * ref["nr"]) * CG_SLACK
    out = dict(x=bx, r=br, nr=d_nr)
    if "mu" in ref:
        mu = ref["mu"]
        d_mu = abs(mu) * (d_nr / ref["nr"] + 3 * u)
        out["p"] = (br + d_mu * np.abs(p) + u * np.abs(mu * p) + u * np.abs(ref["p"])) * CG_SLACK
    return out


def cg_problem(n, seed=11):
    """a diagonal SPD operator with O(1) entries and a right-hand side whose last element is not small (so that the last
    element of every dot carries about 1 / n of it) -> (diag, b) float32 arrays"""
    import numpy as np
    rs = np.random.RandomState(seed + n)
    d = rs.uniform(0.5, 2.0, n).astype(np.float32)
    b = rs.standard_normal(n).astype(np.float32)
    b[-1] = np.float32(math.copysign(1.0 + abs(float(b[-1])), float(b[-1])))
    return d, b
