"""The natural-gradient kernels for actors with three and four hidden layers (csrc/pds_npg_deep.hip, include/pds_npg_deep.h) on the
device, through fused.FusedMLP(net, act, npg_deep=True): the Fisher-vector product against the float64 double backward of KL.mean(),
the line-search candidates against a float64 evaluation, conjugate gradients over the deep Fisher operator, and the policy gradient
with an infinite clip ratio.  The case table, the references and the bars are tests/npg_deep_cases.py (checked on the CPU by
tests/test_npg_deep_cpu.py); the margins recorded on the MI355X are profiles/npg_deep_parity_margins.txt."""
import math

import pytest
import torch

import mlp_cases as mc
import mlp_deep_cases as dc
import npg_cases as nc
import npg_deep_cases as ndc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _fm(net, act):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    return FusedMLP(net, act, npg_deep=True)


@pytest.mark.parametrize("c", ndc.FVP_CASES, ids=ndc.case_id)
def test_fisher_vector_product_over_the_shape_table(c, record_property):
    i = ndc.make_inputs(c, DEV)
    net, x, index, xs, log_std, v = (i[k] for k in ("net", "x", "index", "xs", "log_std", "v"))
    fm = _fm(net, c.act)
    assert fm.deep and fm.npg_deep and fm.flat_grad.numel() == ndc.param_count(c)
    if index is not None:  # only indexed rows are read: every other row is NaN
        mask = torch.ones(x.shape[0], dtype=torch.bool, device=DEV)
        mask[index] = False
        assert bool(mask.any()) and bool(torch.isnan(x[mask]).all()) and bool(torch.isfinite(x[index]).all())
    fm._npg_workspace(0).fill_(NAN)  # every wave, idle or not, writes its partial
    got = fm.fisher_vector_product(x, v, log_std, 0.0, index=index)
    assert bool(torch.isfinite(got).all())
    want = nc.ref_fvp(net, xs, log_std, v)
    dense = cancel = None
    if c.B <= ndc.DENSE_MAX:
        dense, cancel = nc.ref_fvp_dense(net, xs, log_std, v, ndc.cancel_depth(c))
    # (a) of the bar: float32 autograd double backward on this case's inputs, on the device; the rank-one case has the cancellation
    # term instead
    live = None if ndc.cancel_applies(c) else ndc.tensor_rho(nc.fvp_autograd(net, xs, log_std, v, torch.float32), want, c)
    if live is not None:
        live = {k: (r if math.isfinite(r) else 0.0) for k, r in live.items()}
    rho = ndc.tensor_rho(got, want, c)
    margins = ndc.fvp_margins(c, got, want, cancel, live)
    print("fvp", ndc.case_id(c), "rho", " ".join(f"{k} {r:.2e}" for k, r in rho.items()),
          "whole %.2e" % float(torch.norm(got.double() - want) / torch.norm(want)),
          "f32", " ".join(f"{k} {r:.2e}" for k, r in (live or {}).items()),
          "err/bar", " ".join(f"{k} {r:.3f}" for k, r in margins.items()), "margin %.3f" % max(margins.values()))
    record_property("margin", max(margins.values()))
    assert max(margins.values()) <= 1.0, (margins, rho)
    for name, sl in ndc.slices(c).items():  # where the float64 tensor is exactly zero the kernel's is too
        if float(torch.norm(want[sl])) == 0.0:
            assert bool((got[sl] == 0).all()), name
    if dense is not None:
        md = ndc.fvp_margins(c, got, dense, cancel, live)
        assert max(md.values()) <= 1.0, md
    fm._npg_workspace(0).fill_(NAN)
    assert torch.equal(got, fm.fisher_vector_product(x, v, log_std, 0.0, index=index))  # fixed-order sums, no atomics
    alias = v.clone()
    assert fm.fisher_vector_product(x, alias, log_std, 0.0, index=index, out=alias) is alias
    assert torch.equal(alias, got)  # out may alias v
    damped = fm.fisher_vector_product(x, v, log_std, 0.1, index=index)
    assert torch.equal(damped, got + v * 0.1)  # flat_grad_grad_kl + v * cg_damping: two products, one sum


@pytest.mark.parametrize("d_in,hidden,act", [(34, (50, 30, 20), "relu"), (48, (16, 64, 33), "tanh"), (34, (32, 32, 32, 32), "tanh"),
                                             (40, (50, 30, 20, 10), "relu")])
def test_fisher_vector_product_is_symmetric_and_positive(d_in, hidden, act):
    net = dc.make_net(d_in, hidden, 4, act, 0)
    fm = _fm(net, act)
    g = torch.Generator(device=DEV).manual_seed(2)
    x = torch.randn(8192, d_in, device=DEV, generator=g)
    log_std = torch.full((4,), math.log(0.5), device=DEV)
    u, v = (torch.randn(fm.flat_grad.numel(), device=DEV, generator=g) for _ in range(2))
    fu = fm.fisher_vector_product(x, u, log_std, 0.0).double()
    fv = fm.fisher_vector_product(x, v, log_std, 0.0).double()
    a, b = float(u.double() @ fv), float(v.double() @ fu)
    assert abs(a - b) <= 1e-5 * (float(torch.norm(u)) * float(torch.norm(fv)))
    assert float(v.double() @ fv) >= 0 and float(u.double() @ fu) >= 0


@pytest.mark.parametrize("c", ndc.LS_CASES, ids=ndc.case_id)
def test_line_search_candidates_over_the_shape_table(c, record_property):
    i = ndc.make_inputs(c, DEV)
    fm = _fm(i["net"], c.act)
    fr = ndc.LS_FRACS
    fracs = torch.tensor(fr, dtype=torch.float32, device=DEV)
    thetas = torch.full((len(fr), i["theta"].numel()), NAN, device=DEV)
    mu_old = fm.forward(i["x"])  # the kernel's own forward: the f = 0 candidate's KL against it is exactly zero
    assert float((mu_old - i["mu_old"]).abs().max()) <= 1e-5 * max(1.0, float(i["mu_old"].abs().max()))
    args = (i["x"], i["act"], i["adv"], i["logp_old"], mu_old, i["log_std"])
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
        if f == 0.0:
            assert float(out[j, 1]) == 0.0  # the forward chain is stated once: pds_mlp_deep_forward's bits
        ref = nc.ref_ls(i["net"], want_theta, *args)
        bars = nc.ls_merged_bars(ref, c.B, c.d_out)
        errs = [abs(float(out[j, 0]) - ref["ra"]), abs(float(out[j, 1]) - ref["kl"]), abs(float(out[j, 3]) - ref["rs"])]
        print("ls", ndc.case_id(c), "f", f, "err/merged-bar", " ".join("%.4f" % (e / b) for e, b in zip(errs, bars)))
        for k in range(3):
            worst[k] = max(worst[k], errs[k] / bars[k])
            assert errs[k] <= bars[k], (j, k, errs[k], bars[k])
    record_property("margin", max(worst))
    for j in (1, 2):  # a candidate's result does not depend on the other candidates of the launch
        fm._npg_workspace(len(fr)).fill_(NAN)
        alone = fm.surrogate_kl(i["s"], fracs[j:j + 1].clone(), *args)
        assert torch.equal(alone[0], out_dev[j]), j


@pytest.mark.parametrize("d_in,hidden,act", [(34, (50, 30, 20), "relu"), (34, (32, 32, 32, 32), "tanh")])
def test_cg_kernel_with_the_deep_fisher_operator_matches_float64(d_in, hidden, act):
    from phoenix_drone_simulation_amd.fused import conjugate_gradients
    net = dc.make_net(d_in, hidden, 4, act, 0)
    fm = _fm(net, act)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(4096, d_in, device=DEV, generator=g)
    log_std = torch.full((4,), math.log(0.3), device=DEV)
    b = torch.randn(fm.flat_grad.numel(), device=DEV, generator=g)
    got, _ = conjugate_gradients(lambda p, out: fm.fisher_vector_product(x, p, log_std, 0.1, out=out), b, 10)
    want = ndc.cg64(lambda p: nc.ref_fvp(net, x, log_std, p) + 0.1 * p, b.double(), 10)
    assert float(torch.norm(got.double() - want) / torch.norm(want)) < 1e-3


@pytest.mark.parametrize("d_in,hidden,act", [(34, (50, 30, 20), "relu"), (34, (32, 32, 32, 32), "tanh")])
def test_policy_grad_with_infinite_clip_is_the_unclipped_gradient(d_in, hidden, act):
    """pds_mlp_deep_ppo_policy_grad_step with clip_ratio = inf: min(r A, clip(r) A) = r A, so the gradient of -(r A).mean(), at the
    gradient bar of tests/mlp_deep_cases.py (the two-hidden-layer bar, or 4 units of float32 torch's own distance)"""
    B = 4096
    net = dc.make_net(d_in, hidden, 4, act, 0)
    fm = _fm(net, act)
    x, act_t, adv, logp_old, log_std = dc.ppo_inputs(net, B, 7)
    stats = fm.ppo_grad(x, act_t, adv, logp_old, log_std, math.inf).clone()
    got = fm.flat_grad.clone().double()

    def unclipped(dtype):
        n = dc.net_as(net, dtype)
        lp = torch.distributions.Normal(n(x.to(dtype)), torch.exp(log_std.to(dtype))).log_prob(act_t.to(dtype)).sum(-1)
        ratio = torch.exp(lp - logp_old.to(dtype))
        loss = -(ratio * adv.to(dtype)).mean()
        return torch.cat([t.reshape(-1) for t in torch.autograd.grad(loss, list(n.parameters()))]).double(), float(loss.detach()), ratio.detach()

    want, loss, ratio = unclipped(torch.float64)
    f32, loss32, _ = unclipped(torch.float32)
    dc.check_all([("grad", got, want, f32, 2e-4, mc.grad_atol(want, B)),
                  ("loss", float(stats[0]) / B, loss, loss32, 0.0, 2e-5 * max(1.0, abs(loss)))])
    assert bool((ratio > 1.2).any())  # the clip of PPO (0.2) would have cut these samples


def test_without_the_keyword_a_deep_network_is_still_refused():
    """the default is pinned by tests/test_gpu_mlp_deep.py; one line of it here, so that this file fails loudly if the default moves"""
    from phoenix_drone_simulation_amd.fused import FusedMLP
    net = dc.make_net(34, (50, 30, 20), 4, "relu", 0)
    fm = FusedMLP(net, "relu")
    x, v, ls = torch.zeros(16, 34, device=DEV), torch.zeros(fm.flat_grad.numel(), device=DEV), torch.zeros(4, device=DEV)
    assert fm.deep and not fm.npg_deep
    with pytest.raises(NotImplementedError, match="2 hidden layers"):
        fm.fisher_vector_product(x, v, ls, 0.1)
    with pytest.raises(NotImplementedError, match="2 hidden layers"):
        fm._npg_workspace(1)
    with pytest.raises(NotImplementedError, match="2 hidden layers"):
        fm.surrogate_kl(v, ls[:1], x, x[:, :4], ls, ls, x[:, :4], ls)
    shallow = FusedMLP(dc.make_net(34, (50, 50), 4, "relu", 0), "relu", npg_deep=True)  # on two hidden layers the keyword changes nothing
    assert not shallow.deep and not shallow.npg_deep and shallow._npg_names[1] == "pds_npg_fisher_vector_product"
