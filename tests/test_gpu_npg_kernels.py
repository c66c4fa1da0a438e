"""The natural-gradient kernels of csrc/pds_npg.hip on the device: the Fisher-vector product against float64 autograd
double backward of KL.mean(), the conjugate-gradient step against the reference restated in float64, the line-search
candidates against a float64 evaluation, and the policy gradient with an infinite clip ratio against autograd of the
unclipped loss.  The case table, the float64 references and the bars of the table-driven tests are tests/npg_cases.py
(checked on the CPU by tests/test_npg_oracle_cpu.py); the margins recorded on the MI355X are
profiles/npg_parity_margins.txt."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import npg_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _net(d_in, h, d_out, act, seed=0):
    from phoenix_drone_simulation_amd.ppo import _mlp
    torch.manual_seed(seed)
    return _mlp([d_in, h, h, d_out], act).to(DEV)


def _fvp64(net, x, log_std, v, damping):
    """NaturalPolicyGradientAlgorithm.Fvp (algs/npg/npg.py:52-77) in float64"""
    return nc.ref_fvp(net, x, log_std, v) + damping * v.double()


CASES = [(16, 16, 1, "relu", 1), (42, 50, 4, "relu", 17), (42, 50, 4, "tanh", 4096), (68, 64, 8, "relu", 4096),
         (192, 64, 8, "tanh", 4096), (192, 50, 4, "relu", 17), (16, 64, 8, "tanh", 1), (68, 16, 1, "tanh", 131072),
         (42, 50, 4, "relu", 131072)]


@pytest.mark.parametrize("d_in,h,d_out,act,B", CASES)
@pytest.mark.parametrize("indexed", [False, True])
def test_fisher_vector_product_matches_float64_double_backward(d_in, h, d_out, act, B, indexed):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = _net(d_in, h, d_out, act)
    fm = FusedMLP(net, act)
    g = torch.Generator(device=DEV).manual_seed(1)
    rows = 4 * B if indexed else B
    x = torch.randn(rows, d_in, device=DEV, generator=g)
    index = torch.arange(0, rows, 4, device=DEV) if indexed else None
    log_std = torch.linspace(-1.2, -0.4, d_out, device=DEV)
    P = fm.flat_grad.numel()
    v = torch.randn(P, device=DEV, generator=g)
    fm._npg_workspace(0).fill_(NAN)  # every wave, idle or not, writes its partial
    got = fm.fisher_vector_product(x, v, log_std, 0.0, index=index)  # F v alone: the bar is relative to |F v|
    want = _fvp64(net, x[::4] if indexed else x, log_std, v, 0.0)
    bar = 2e-5 * float(torch.norm(want))
    if B * d_out == 1:
        # one sample, one output: F = j j^T / sigma^2 and F v is the single dot product j.v, which cancels -- float32 meets
        # it to the dot product's own bound, P eps sum |j_i v_i|, not to 2e-5 of its (small) value
        n64 = torch.nn.Sequential(*[m.double() if isinstance(m, torch.nn.Linear) else m for m in __import__("copy").deepcopy(net)])
        j = torch.cat([t.reshape(-1) for t in torch.autograd.grad(n64((x[::4] if indexed else x).double()).sum(),
                                                                   list(n64.parameters()))])
        cond = float((j * v.double()).abs().sum()) * float(torch.norm(j)) * float(torch.exp(-2 * log_std.double()).max())
        bar += P * 2 ** -24 * cond
    err = float(torch.norm(got.double() - want))
    assert err < bar, (err, bar, float(torch.norm(want)))
    damped = fm.fisher_vector_product(x, v, log_std, 0.1, index=index)
    assert torch.equal(damped, got + v * 0.1)  # two products, one sum: to the bit
    again = fm.fisher_vector_product(x, v, log_std, 0.0, index=index)
    assert torch.equal(got, again)  # bitwise repeatable: fixed-order sums, no atomics


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_fisher_vector_product_is_symmetric_and_positive(act):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = _net(42, 50, 4, act)
    fm = FusedMLP(net, act)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(8192, 42, device=DEV, generator=g)
    log_std = torch.full((4,), math.log(0.5), device=DEV)
    u, v = (torch.randn(fm.flat_grad.numel(), device=DEV, generator=g) for _ in range(2))
    fu = fm.fisher_vector_product(x, u, log_std, 0.0).double()
    fv = fm.fisher_vector_product(x, v, log_std, 0.0).double()
    a, b = float(u.double() @ fv), float(v.double() @ fu)
    assert abs(a - b) <= 1e-5 * (float(torch.norm(u)) * float(torch.norm(fv)))
    assert float(v.double() @ fv) >= 0 and float(u.double() @ fu) >= 0


def _cg64(avp, b, nsteps, residual_tol=1e-10, eps=1e-6):
    x = torch.zeros_like(b)
    r = b.clone()
    p = r.clone()
    rdotr = r @ r
    for _ in range(nsteps):
        z = avp(p)
        alpha = rdotr / (p @ z + eps)
        x += alpha * p
        r -= alpha * z
        new = r @ r
        if math.sqrt(float(new)) < residual_tol:
            break
        p = r + new / (rdotr + eps) * p
        rdotr = new
    return x


@pytest.mark.parametrize("case", ["spd", "breaks_early"])
def test_cg_kernel_matches_the_reference_restated_in_float64(case):
    from phoenix_drone_simulation_amd.fused import conjugate_gradients
    rs = np.random.RandomState(4)
    n = 5000
    if case == "spd":
        d = rs.uniform(0.1, 2.0, n)
        b = rs.standard_normal(n)
    else:
        d = np.full(n, 2.0)
        b = rs.standard_normal(n) * 1e6 / math.sqrt(n)
    A = torch.as_tensor(d, device=DEV)
    want = _cg64(lambda p: A * p, torch.as_tensor(b, device=DEV), 10)
    A32 = A.float()
    got, st = conjugate_gradients(lambda p, out: torch.mul(A32, p, out=out), torch.as_tensor(b, device=DEV, dtype=torch.float32), 10)
    assert float(torch.norm(got.double() - want) / torch.norm(want)) < 1e-5
    assert float(st[1]) == (1.0 if case == "breaks_early" else 0.0)


def test_cg_kernel_with_the_fisher_operator_matches_float64():
    from phoenix_drone_simulation_amd.fused import FusedMLP, conjugate_gradients
    net = _net(42, 50, 4, "relu")
    fm = FusedMLP(net, "relu")
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4096, 42, device=DEV, generator=g)
    log_std = torch.full((4,), math.log(0.3), device=DEV)
    b = torch.randn(fm.flat_grad.numel(), device=DEV, generator=g)
    got, _ = conjugate_gradients(lambda p, out: fm.fisher_vector_product(x, p, log_std, 0.1, out=out), b, 10)
    want = _cg64(lambda p: _fvp64(net, x, log_std, p, 0.1), b.double(), 10)
    assert float(torch.norm(got.double() - want) / torch.norm(want)) < 1e-3


@pytest.mark.parametrize("d_in,h,act,B", [(42, 50, "relu", 20000), (192, 64, "tanh", 4097), (16, 16, "relu", 1)])
def test_line_search_candidates_match_float64(d_in, h, act, B):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    A = 4
    net = _net(d_in, h, A, act)
    fm = FusedMLP(net, act)
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.randn(B, d_in, device=DEV, generator=g)
    log_std = torch.full((A,), math.log(0.4), device=DEV)
    theta = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    s = 0.05 * torch.randn(theta.numel(), device=DEV, generator=g)
    with torch.no_grad():
        mu_old = net(x)
    act_t = mu_old + 0.4 * torch.randn(B, A, device=DEV, generator=g)
    adv = torch.randn(B, device=DEV, generator=g)
    logp_old = torch.distributions.Normal(mu_old, torch.exp(log_std)).log_prob(act_t).sum(-1) + 0.01
    fr = [0.8 ** j for j in range(15)] + [float("inf")]  # the last candidate has non-finite parameters
    fracs = torch.tensor(fr, dtype=torch.float32, device=DEV)
    thetas = torch.empty(len(fr), theta.numel(), device=DEV)
    fm._npg_workspace(len(fr)).fill_(NAN)
    out = fm.surrogate_kl(s, fracs, x, act_t, adv, logp_old, mu_old, log_std, theta_out=thetas).cpu()
    n64 = torch.nn.Sequential(*[m.double() if isinstance(m, torch.nn.Linear) else m for m in __import__("copy").deepcopy(net)])
    for j, f in enumerate(fr):
        want_theta = theta + f * s  # torch's expression: f rounded to float32, product and sum rounded separately
        assert torch.equal(thetas[j], want_theta), j
        if not math.isfinite(f):
            assert out[j, 2] == 1.0
            continue
        assert out[j, 2] == 0.0
        off = 0
        with torch.no_grad():
            for p in n64.parameters():
                p.copy_(want_theta[off:off + p.numel()].view_as(p).double())
                off += p.numel()
            mu = n64(x.double())
            std = torch.exp(log_std.double())
            lp = torch.distributions.Normal(mu, std).log_prob(act_t.double()).sum(-1)
            ra = float((torch.exp(lp - logp_old.double()) * adv.double()).sum())
            kl = float(torch.distributions.kl.kl_divergence(torch.distributions.Normal(mu_old.double(), std),
                                                             torch.distributions.Normal(mu, std)).sum())
        scale = float((torch.exp(lp - logp_old.double()) * adv.double()).abs().sum())
        assert abs(float(out[j, 0]) - ra) <= 1e-5 * scale + 1e-6, (j, float(out[j, 0]), ra)
        assert abs(float(out[j, 1]) - kl) <= 1e-4 * kl + 1e-5 * B * A * 1e-7 + 1e-6, (j, float(out[j, 1]), kl)
        rsum = float(torch.exp(lp - logp_old.double()).sum())
        assert abs(float(out[j, 3]) - rsum) <= 1e-5 * rsum, (j, float(out[j, 3]), rsum)


@pytest.mark.parametrize("B", [4096, 131072])
def test_policy_grad_with_infinite_clip_is_the_unclipped_gradient(B):
    """pds_ppo_policy_grad with clip_ratio = inf: min(r A, clip(r) A) = r A, so the gradient of -(r A).mean() -- on the f32
    kernels (4096) and the split-bf16 ones (131072 >= 65 536)."""
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = _net(42, 50, 4, "relu")
    fm = FusedMLP(net, "relu")
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(B, 42, device=DEV, generator=g)
    log_std = torch.full((4,), math.log(0.5), device=DEV)
    with torch.no_grad():
        mu = net(x)
    act_t = mu + 0.5 * torch.randn(B, 4, device=DEV, generator=g)
    adv = torch.randn(B, device=DEV, generator=g)
    logp_old = torch.distributions.Normal(mu, torch.exp(log_std)).log_prob(act_t).sum(-1) - 0.3 * torch.rand(B, device=DEV, generator=g)
    stats = fm.ppo_grad(x, act_t, adv, logp_old, log_std, math.inf)
    got = fm.flat_grad.clone().double()
    n64 = torch.nn.Sequential(*[m.double() if isinstance(m, torch.nn.Linear) else m for m in __import__("copy").deepcopy(net)])
    lp = torch.distributions.Normal(n64(x.double()), torch.exp(log_std.double())).log_prob(act_t.double()).sum(-1)
    ratio = torch.exp(lp - logp_old.double())
    loss = -(ratio * adv.double()).mean()
    want = torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss, list(n64.parameters()))])
    assert float(torch.norm(got - want) / torch.norm(want)) < 2e-5
    assert abs(float(stats[0]) / B - float(loss)) < 1e-5 * max(1.0, abs(float(loss)))
    assert bool((ratio > 1.2).any())  # the clip of PPO (0.2) would have cut these samples


def test_argument_checks_return_einval_and_leave_outputs():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.fused import FusedMLP, _ptr
    net = _net(42, 50, 4, "relu")
    fm = FusedMLP(net, "relu")
    lib = pds.native.load()
    P = fm.flat_grad.numel()
    x = torch.zeros(16, 42, device=DEV)
    ls = torch.zeros(4, device=DEV)
    v = torch.ones(P, device=DEV)
    out = torch.full((P,), 7.0, device=DEV)
    ws = torch.empty(lib.pds_npg_workspace_floats(C.byref(fm.m), 15), device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.pds_npg_fisher_vector_product(None, _ptr(x), None, 16, _ptr(ls), _ptr(v), 0.1, _ptr(out), _ptr(ws), s) == pds.native.EINVAL
    assert lib.pds_npg_fisher_vector_product(C.byref(fm.m), None, None, 16, _ptr(ls), _ptr(v), 0.1, _ptr(out), _ptr(ws), s) == pds.native.EINVAL
    assert lib.pds_npg_fisher_vector_product(C.byref(fm.m), _ptr(x), None, 0, _ptr(ls), _ptr(v), 0.1, _ptr(out), _ptr(ws), s) == pds.native.EINVAL
    bad = pds.native.Mlp.from_buffer_copy(fm.m)
    for field, val in (("d_in", 193), ("h1", 65), ("h2", 0), ("d_out", 9), ("activation", 2)):
        bad = pds.native.Mlp.from_buffer_copy(fm.m)
        setattr(bad, field, val)
        assert lib.pds_npg_fisher_vector_product(C.byref(bad), _ptr(x), None, 16, _ptr(ls), _ptr(v), 0.1, _ptr(out), _ptr(ws), s) == pds.native.EINVAL
        assert lib.pds_npg_workspace_floats(C.byref(bad), 1) == pds.native.EINVAL
        res = torch.full((4,), 7.0, device=DEV)
        assert lib.pds_npg_surrogate_kl(C.byref(bad), _ptr(v), _ptr(ls), 1, _ptr(x), _ptr(x), _ptr(ls), _ptr(ls), _ptr(x), _ptr(ls),
                                        16, _ptr(res), None, _ptr(ws), s) == pds.native.EINVAL
        assert torch.all(res == 7.0)
    assert lib.pds_npg_surrogate_kl(C.byref(fm.m), _ptr(v), _ptr(ls), 0, _ptr(x), _ptr(x), _ptr(ls), _ptr(ls), _ptr(x), _ptr(ls),
                                    16, _ptr(out), None, _ptr(ws), s) == pds.native.EINVAL
    assert lib.pds_npg_cg_step(0, _ptr(v), _ptr(v), _ptr(v), _ptr(v), _ptr(ls), 1e-6, 1e-10, 0, s) == pds.native.EINVAL
    assert lib.pds_npg_cg_step(P, None, _ptr(v), _ptr(v), _ptr(v), _ptr(ls), 1e-6, 1e-10, 0, s) == pds.native.EINVAL
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(v == 1.0)


# ---- the table of tests/npg_cases.py ---------------------------------------------------------------------------------------
def _fvp_margin(c, got, want, cancel, live):
    """worst error / bar over the whole vector and the six tensors (the bars of npg_cases.fvp_bars), and the kernel's rho"""
    whole, per = nc.fvp_bars(c, want, cancel, live)
    worst = {"whole": float(torch.norm(got.double() - want)) / whole}
    for name, sl in nc.slices(c).items():
        worst[name] = float(torch.norm(got[sl].double() - want[sl])) / per[name]
    return worst


@pytest.mark.parametrize("c", nc.FVP_CASES, ids=nc.case_id)
def test_fisher_vector_product_over_the_shape_table(c, record_property):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    i = nc.make_inputs(c, DEV)
    net, x, index, xs, log_std, v = (i[k] for k in ("net", "x", "index", "xs", "log_std", "v"))
    fm = FusedMLP(net, c.act)
    assert fm.flat_grad.numel() == nc.param_count(c)
    if index is not None:  # only indexed rows are read: every other row is NaN
        mask = torch.ones(x.shape[0], dtype=torch.bool, device=DEV)
        mask[index] = False
        assert bool(mask.any()) and bool(torch.isnan(x[mask]).all()) and bool(torch.isfinite(x[index]).all())
    fm._npg_workspace(0).fill_(NAN)
    got = fm.fisher_vector_product(x, v, log_std, 0.0, index=index)
    assert bool(torch.isfinite(got).all())
    want = nc.ref_fvp(net, xs, log_std, v)
    dense = cancel = live = None
    if c.B <= nc.DENSE_MAX:
        dense, cancel = nc.ref_fvp_dense(net, xs, log_std, v, nc.cancel_depth(c))
        if not nc.cancel_applies(c):
            live = nc.tensor_rho(nc.fvp_autograd(net, xs, log_std, v, torch.float32), want, c)
    rho = nc.tensor_rho(got, want, c)
    margins = _fvp_margin(c, got, want, cancel, live)
    print("fvp", nc.case_id(c), "rho", " ".join(f"{k} {r:.2e}" for k, r in rho.items()),
          "whole %.2e" % float(torch.norm(got.double() - want) / torch.norm(want)),
          "f32", " ".join(f"{k} {r:.2e}" for k, r in (live or {}).items()), "margin %.3f" % max(margins.values()))
    record_property("margin", max(margins.values()))
    assert max(margins.values()) < 1.0, (margins, rho)
    if dense is not None:
        md = _fvp_margin(c, got, dense, cancel, live)
        assert max(md.values()) < 1.0, md
    fm._npg_workspace(0).fill_(NAN)
    assert torch.equal(got, fm.fisher_vector_product(x, v, log_std, 0.0, index=index))  # fixed-order sums, no atomics
    alias = v.clone()
    assert fm.fisher_vector_product(x, alias, log_std, 0.0, index=index, out=alias) is alias
    assert torch.equal(alias, got)  # out may alias v
    damped = fm.fisher_vector_product(x, v, log_std, 0.1, index=index)
    assert torch.equal(damped, got + v * 0.1)  # flat_grad_grad_kl + v * cg_damping: two products, one sum


@pytest.mark.parametrize("c", nc.LS_CASES, ids=nc.case_id)
def test_line_search_candidates_over_the_shape_table(c, record_property):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    i = nc.make_inputs(c, DEV)
    fm = FusedMLP(i["net"], c.act)
    fr = nc.LS_FRACS
    fracs = torch.tensor(fr, dtype=torch.float32, device=DEV)
    thetas = torch.full((len(fr), i["theta"].numel()), NAN, device=DEV)
    args = (i["x"], i["act"], i["adv"], i["logp_old"], i["mu_old"], i["log_std"])
    fm._npg_workspace(len(fr)).fill_(NAN)
    out_dev = fm.surrogate_kl(i["s"], fracs, *args, theta_out=thetas)
    out = out_dev.cpu()
    worst = [0.0, 0.0, 0.0]
    for j, f in enumerate(fr):
        want_theta = i["theta"] + f * i["s"]  # f rounded to float32, product and sum rounded separately
        assert torch.equal(thetas[j], want_theta), j
        if not math.isfinite(f):
            assert out[j, 2] == 1.0
            continue
        assert out[j, 2] == 0.0
        ref = nc.ref_ls(i["net"], want_theta, *args)
        bars = nc.ls_bars(ref, c.B, c.d_out)
        errs = [abs(float(out[j, 0]) - ref["ra"]), abs(float(out[j, 1]) - ref["kl"]), abs(float(out[j, 3]) - ref["rs"])]
        old = nc.ls_merged_bars(ref, c.B, c.d_out)
        print("ls", nc.case_id(c), "f", f, "err/bar", " ".join("%.3f" % (e / b) for e, b in zip(errs, bars)),
              "err/merged-bar", " ".join("%.4f" % (e / b) for e, b in zip(errs, old)))
        for k in range(3):
            worst[k] = max(worst[k], errs[k] / bars[k])
            assert errs[k] <= bars[k], (j, k, errs[k], bars[k])
    record_property("margin", max(worst))
    for j in (0, 2):  # a candidate's result does not depend on the other candidates of the launch
        fm._npg_workspace(len(fr)).fill_(NAN)
        alone = fm.surrogate_kl(i["s"], fracs[j:j + 1].clone(), *args)
        assert torch.equal(alone[0], out_dev[j]), j


def _cg_launch(n, x, r, p, z, st, eps, tol, init):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.fused import _ptr
    assert all(t.numel() == n and t.dtype == torch.float32 and t.is_contiguous() for t in (x, r, p, z)) and st.numel() == 2
    rc = pds.native.load().pds_npg_cg_step(n, _ptr(x), _ptr(r), _ptr(p), _ptr(z), _ptr(st), float(eps), float(tol), int(init),
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == pds.native.OK
    torch.cuda.synchronize()


def _np(*ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def _cg_init(n):
    d, b = nc.cg_problem(n)
    D, bt = torch.as_tensor(d, device=DEV), torch.as_tensor(b, device=DEV)
    x, r, p = (torch.full((n,), NAN, device=DEV) for _ in range(3))
    st = torch.full((2,), NAN, device=DEV)
    _cg_launch(n, x, r, p, bt, st, 1e-6, 1e-10, True)
    return D, bt, b, x, r, p, st


def _cg_margin(ref, x, r, p, st):
    """worst error / bar of a launch that did not find the state frozen"""
    bars = nc.cg_step_bars(ref)
    xs, rs, ps, sts = _np(x, r, p, st)
    tiny = np.finfo(np.float64).tiny
    worst = max(float(np.max(np.abs(xs - ref["x"]) / (bars["x"] + tiny))), float(np.max(np.abs(rs - ref["r"]) / (bars["r"] + tiny))))
    if not ref["stopped_now"]:
        worst = max(worst, float(np.max(np.abs(ps - ref["p"]) / (bars["p"] + tiny))), abs(float(sts[0]) - ref["st"][0]) / bars["nr"])
    return worst, bars


@pytest.mark.parametrize("n", nc.CG_SIZES)
def test_cg_step_matches_float64_launch_by_launch(n, record_property):
    D, bt, b, x, r, p, st = _cg_init(n)
    # the init launch: x = 0, r = p = b to the bit, st = {b.b within the dot bar, 0}
    assert torch.equal(x, torch.zeros_like(x)) and torch.equal(r, bt) and torch.equal(p, bt)
    b64 = b.astype(np.float64)
    assert abs(float(st[0]) - float(b64 @ b64)) <= nc.cg_dot_bar(b, b) and float(st[1]) == 0.0
    worst = abs(float(st[0]) - float(b64 @ b64)) / nc.cg_dot_bar(b, b)
    for launch in range(6):
        z = D * p
        ref = nc.ref_cg_step(x, r, p, z, st, 1e-6, 1e-10, False)  # from the state the device holds
        assert not ref["stopped_now"]
        _cg_launch(n, x, r, p, z, st, 1e-6, 1e-10, False)
        m, _ = _cg_margin(ref, x, r, p, st)
        print("cg n", n, "launch", launch, "margin %.3f" % m)
        worst = max(worst, m)
        assert m < 1.0, (launch, m)
        assert float(st[1]) == 0.0
    record_property("margin", worst)


def test_cg_break_updates_x_and_r_then_freezes_the_state():
    n, stop_at = 5000, 3
    d, b = nc.cg_problem(n)
    # the tolerance between |r| after launch `stop_at - 1` and after launch `stop_at` of the float64 solve
    x64, r64, p64, st64 = np.zeros(n), b.astype(np.float64), b.astype(np.float64), np.array([float(b.astype(np.float64) @ b), 0.0])
    norms = []
    for _ in range(stop_at + 1):
        s = nc.ref_cg_step(x64, r64, p64, d * p64, st64, 1e-6, 0.0, False)
        x64, r64, p64, st64 = s["x"], s["r"], s["p"], s["st"]
        norms.append(math.sqrt(s["nr"]))
    assert all(a > c for a, c in zip(norms, norms[1:]))
    tol = math.sqrt(norms[stop_at - 1] * norms[stop_at])
    D, bt, b, x, r, p, st = _cg_init(n)
    for launch in range(stop_at + 1):
        z = D * p
        ref = nc.ref_cg_step(x, r, p, z, st, 1e-6, tol, False)
        bars = nc.cg_step_bars(ref)
        assert abs(ref["nr"] - tol * tol) >= 10 * bars["nr"]  # |r| is far from the tolerance on either side, at every launch
        assert ref["stopped_now"] == (launch == stop_at)
        p_before, st_before = p.clone(), st.clone()
        _cg_launch(n, x, r, p, z, st, 1e-6, tol, False)
        m, _ = _cg_margin(ref, x, r, p, st)
        assert m < 1.0, (launch, m)
        if launch == stop_at:  # the reference's break: x and r updated, p kept
            assert torch.equal(p, p_before) and float(st[1]) == 1.0 and torch.equal(st[:1], st_before[:1])
        else:
            assert float(st[1]) == 0.0 and not torch.equal(p, p_before)
    frozen = [t.clone() for t in (x, r, p, st)]
    for _ in range(3):
        _cg_launch(n, x, r, p, D * p, st, 1e-6, tol, False)
        assert all(torch.equal(a, c) for a, c in zip((x, r, p, st), frozen))
