"""The SAC kernels of csrc/pds_sac.hip on the device: the policy gradient against float64 autograd of sac.loss_pi's recipe, the
entropy-regularised backup and the elementwise sampler against float64, the Adam step on the gradient call against
pds_adam_step bit for bit, and the argument checks.  The kernels' own noise is fed to the references: eps is regenerated
through gaussian_sample(mu = 0, log_std = 0), which the noise contract (include/pds.h) names as the same variates.

Bars.  Gradient: rtol 2e-4 + mlp_cases.grad_atol (2e-6 of the largest entry), the project's bar for this MFMA chain.  sum min Q,
sum logp and the backup: the forward bar of tests/test_gpu_mlp_dispatch.py (rtol 1e-5, atol 2e-6 per sample; summed over the
batch for the two sums).  None of these bars was exceeded on an MI355X, so none is widened: the largest gradient error is 0.041
of its bar, the sums stay under 0.02 and the backup under 0.15 of theirs.  Every case also evaluates the same quantity with
TORCH in float32 and prints that error next to the kernel's (the two are of one size: the longer exp / tanh / log1p chain costs
the kernel nothing extra).  What was measured is in profiles/sac_parity_margins.txt; every case records its margin (error / bar)
as a test property.

min(Q1, Q2) has a kink: a sample whose two Q values tie within float32 rounding may legitimately choose either network.  Every
mixed-selection case therefore asserts ON ITS INPUTS that the float64 gap min_g |Q1 - Q2| is at least 1e-4 (its seed was picked
so); no sample is excluded."""
import copy
import ctypes as C
import math

import pytest
import torch

import mlp_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 2 * mc.WIDE_ROUND + 16 * 3 + 5  # a ragged batch past two rounds of either persistent grid (256 blocks x 3 or 4 waves x 16)
SEED, CALL = 0x5AC5EED, 7              # the noise of the gradient and target cases
ALPHA = 0.2
MIN_GAP = 1e-4

# D, actor hidden, Q hidden, actor act, Q act, B, index, act_limit, seed of the nets, variant
#   variant "mixed": independent random q1, q2;  "q1" / "q2": q2 = q1 with its last bias shifted by +1 / -1 (every sample
#   selects q1 / q2, gap 1);  ("ls", v): the log_std rows of the actor's b3 set to v (at v = 1.5 the rows of w3 are scaled by
#   8 as well: the initial weights leave log_std within 0.5 of its bias, and the clamp at 2 is to bind for SOME samples).
#   The seeds are those for which the conditions the test asserts on its inputs hold (gap, and both Qs chosen from B = 15 on).
GRAD_CASES = [
    (12, (16, 17), (64, 50), "relu", "tanh", 1, None, 1.0, 0, "mixed"),
    (13, (1, 16), (17, 1), "tanh", "relu", 15, "perm", 0.5, 6, "mixed"),
    (40, (50, 50), (64, 64), "relu", "relu", 16, "rep", 1.0, 12, "mixed"),
    (42, (64, 64), (64, 64), "relu", "relu", 17, None, 1.0, 12, "mixed"),
    (48, (17, 64), (50, 16), "tanh", "tanh", 17, "perm", 0.5, 9, "mixed"),
    (60, (64, 1), (1, 64), "relu", "tanh", 16, "rep", 1.0, 15, "mixed"),
    (60, (50, 17), (16, 50), "tanh", "relu", 1, None, 0.5, 0, "mixed"),
    (12, (64, 64), (64, 64), "tanh", "tanh", 15, "rep", 1.0, 0, "mixed"),
    (34, (64, 64), (64, 64), "relu", "relu", 128, "rep", 1.0, 12, "mixed"),   # Hover at the trainer's defaults
    (48, (50, 50), (64, 64), "tanh", "relu", 128, "perm", 0.5, 3, "mixed"),
    (40, (16, 50), (50, 64), "relu", "tanh", 4099, "rep", 0.5, 0, "q1"),
    (40, (16, 50), (50, 64), "relu", "tanh", 4099, "rep", 0.5, 0, "q2"),
    (42, (64, 64), (64, 64), "relu", "relu", TAIL, "perm", 1.0, 0, "q1"),
    (42, (64, 64), (64, 64), "relu", "relu", TAIL, "perm", 1.0, 0, "q2"),
    (48, (50, 50), (64, 64), "tanh", "relu", TAIL + 11, None, 0.5, 0, "q1"),
    (48, (50, 50), (64, 64), "tanh", "relu", TAIL + 11, None, 0.5, 0, "q2"),
    (42, (64, 64), (64, 64), "relu", "relu", 17, None, 1.0, 12, ("ls", 30.0)),
    (42, (64, 64), (64, 64), "relu", "relu", 128, "rep", 1.0, 15, ("ls", 30.0)),
    (42, (64, 64), (64, 64), "relu", "relu", 17, None, 1.0, 9, ("ls", -30.0)),
    (42, (64, 64), (64, 64), "relu", "relu", 128, "rep", 1.0, 15, ("ls", -30.0)),
    (42, (64, 64), (64, 64), "relu", "relu", 17, None, 1.0, 12, ("ls", 1.5)),
    (42, (64, 64), (64, 64), "relu", "relu", 128, "rep", 1.0, 15, ("ls", 1.5)),
]


def _id(c):
    v = c[9] if isinstance(c[9], str) else f"ls{c[9][1]:+g}"
    return f"D{c[0]}-pi{c[1][0]}x{c[1][1]}{c[3]}-q{c[2][0]}x{c[2][1]}{c[4]}-B{c[5]}-{c[6]}-lim{c[7]}-{v}"


def _nets(D, ph, qh, pact, qact, seed=0, variant="mixed"):
    """(pi, q1, q2) as torch modules -- the actor is ONE net of d_out = 8, [mu | log_std] -- and their FusedMLP views"""
    from phoenix_drone_simulation_amd.fused import FusedMLP
    pi = mc.make_net(D, ph[0], ph[1], 8, pact, seed)
    q1 = mc.make_net(D + 4, qh[0], qh[1], 1, qact, seed + 1)
    if variant in ("q1", "q2"):
        q2 = copy.deepcopy(q1)
        with torch.no_grad():
            q2[4].bias += 1.0 if variant == "q1" else -1.0
    else:
        q2 = mc.make_net(D + 4, qh[0], qh[1], 1, qact, seed + 2)
    if isinstance(variant, tuple):
        with torch.no_grad():
            pi[4].bias[4:] = variant[1]
            if variant[1] == 1.5:
                pi[4].weight[4:] *= 8.0
    return (pi, q1, q2), (FusedMLP(pi, pact), FusedMLP(q1, qact), FusedMLP(q2, qact))


def _rows(D, B, index, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = B if index is None else 2 * B + 3
    oa = torch.randn(rows, D + 4, device=DEV, generator=g)
    idx = None if index is None else mc.make_index(index, rows, B, seed + 1)
    return oa, idx


def _eps(B, seed=SEED, call=CALL, id_base=0):
    """the four variates of sample ids id_base .. id_base + B - 1: pds_gaussian_sample at mu = 0, log_std = 0"""
    from phoenix_drone_simulation_amd.fused import gaussian_sample
    out, lp = torch.empty(B, 4, device=DEV), torch.empty(B, device=DEV)
    gaussian_sample(torch.zeros(B, 4, device=DEV), torch.zeros(4, device=DEV), out, lp, seed, call, id_base=id_base)
    return out


def _policy_loss(nets, o, eps, limit, alpha, dtype):
    """compute_loss_pi (algs/sac/sac.py:324-337) in `dtype` through torch autograd, by the recipe of sac.loss_pi on the flat
    networks of the kernel tests -> (flat actor gradient, min Q, logp, Q1, Q2, raw log_std)"""
    from phoenix_drone_simulation_amd.sac import squashed_sample
    pi, q1, q2 = (copy.deepcopy(n).to(dtype) for n in nets)
    o = o.to(dtype)
    head = pi(o)
    a, logp = squashed_sample(head, eps.to(dtype), limit)
    oa = torch.cat([o, a], dim=-1)
    v1, v2 = q1(oa).squeeze(-1), q2(oa).squeeze(-1)
    minq = torch.min(v1, v2)
    (alpha * logp - minq).mean().backward()
    grad = torch.cat([p.grad.reshape(-1) for p in pi.parameters()])
    return grad, minq.detach(), logp.detach(), v1.detach(), v2.detach(), head.detach()[:, 4:]


@pytest.mark.parametrize("case", GRAD_CASES, ids=_id)
def test_policy_gradient_matches_float64_autograd(case, record_property):
    D, ph, qh, pact, qact, B, index, limit, seed, variant = case
    nets, (fpi, fq1, fq2) = _nets(D, ph, qh, pact, qact, seed, variant)
    oa, idx = _rows(D, B, index)
    o = (oa if idx is None else oa[idx])[:, :D]
    eps = _eps(B)
    want, minq, logp, v1, v2, raw = _policy_loss(nets, o, eps, limit, ALPHA, torch.float64)
    g32, minq32, logp32, _, _, _ = _policy_loss(nets, o, eps, limit, ALPHA, torch.float32)
    # ---- conditions on the INPUTS -------------------------------------------------------------------------------------------
    gap = float((v1 - v2).abs().min())
    n_first = int((v1 <= v2).sum())
    assert gap >= MIN_GAP, f"the seed of this case leaves a Q gap of {gap:.3e}: pick another"
    if variant not in ("q1", "q2"):
        assert B < 15 or 0 < n_first < B, f"the seed of this case lets every sample choose one network ({n_first} / {B})"
    else:
        assert n_first == (B if variant == "q1" else 0) and abs(gap - 1.0) < 1e-6  # (the shifted bias is rounded to float32)
    open_ = (raw >= -20.0) & (raw <= 2.0)
    if isinstance(variant, tuple):
        assert (not bool(open_.any())) if abs(variant[1]) == 30.0 else (bool(open_.any()) and bool((~open_).any()))
    # ---- the kernel ---------------------------------------------------------------------------------------------------------
    q_before = [p.detach().clone() for q in nets[1:] for p in q.parameters()]
    st = fpi.sac_policy_grad(fq1, fq2, oa, idx, ALPHA, limit, SEED, CALL).clone()
    got = fpi.flat_grad.clone()
    err32 = float((g32.double() - want).abs().max())
    atol = mc.grad_atol(want, B)
    err = float((got.double() - want).abs().max())
    q_bar = 1e-5 * float(minq.abs().sum()) + 2e-6 * B
    q_err = abs(float(st[0].double()) - float(minq.sum()))
    l_bar = 1e-5 * float(logp.abs().sum()) + 2e-6 * B
    l_err = abs(float(st[1].double()) - float(logp.sum()))
    margin = float(((got.double() - want).abs() / (atol + 2e-4 * want.abs())).max())
    print(f"sac-grad {_id(case)}: err {err:.3e} atol {atol:.3e} max|g| {float(want.abs().max()):.3e} margin {margin:.3f} "
          f"f32 err {err32:.3e} | sumQ err {q_err:.3e} bar {q_bar:.3e} f32 err {abs(float(minq32.double().sum()) - float(minq.sum())):.3e} "
          f"| sumlogp err {l_err:.3e} bar {l_bar:.3e} f32 err {abs(float(logp32.double().sum()) - float(logp.sum())):.3e} "
          f"| gap {gap:.3e} chose q1 {n_first}/{B} clamp open {int(open_.sum())}/{open_.numel()}")
    record_property("margin", margin)
    record_property("margin_sumq", q_err / q_bar)
    record_property("margin_sumlogp", l_err / l_bar)
    assert torch.allclose(got.double(), want, rtol=2e-4, atol=atol), (err, atol)
    assert q_err <= q_bar, (q_err, q_bar)
    assert l_err <= l_bar, (l_err, l_bar)
    assert float(st[3]) == B and float(st[2]) == 0.0
    if isinstance(variant, tuple) and abs(variant[1]) == 30.0:  # the clamp binds everywhere: no gradient into the log_std head
        o_ = fpi.lin[0].weight.numel() + fpi.lin[0].bias.numel() + fpi.lin[1].weight.numel() + fpi.lin[1].bias.numel()
        h2 = fpi.m.h2
        assert torch.all(got[o_ + 4 * h2:o_ + 8 * h2] == 0.0) and torch.all(got[o_ + 8 * h2 + 4:] == 0.0)
        assert float(got[o_:o_ + 4 * h2].abs().max()) > 0.0
    # same inputs, same bits; Q1 and Q2 are only read
    st2 = fpi.sac_policy_grad(fq1, fq2, oa, idx, ALPHA, limit, SEED, CALL)
    assert torch.equal(fpi.flat_grad, got) and torch.equal(st2, st)
    assert all(torch.equal(a, b) for a, b in zip(q_before, [p for q in nets[1:] for p in q.parameters()]))


@pytest.mark.parametrize("pact,qact", [("relu", "relu"), ("tanh", "tanh")])
def test_alpha_zero_and_zeroed_action_columns_give_a_gradient_of_exactly_zero(pact, qact):
    D = 42
    nets, (fpi, fq1, fq2) = _nets(D, (50, 50), (64, 64), pact, qact)
    with torch.no_grad():
        nets[1][0].weight[:, D:] = 0.0
        nets[2][0].weight[:, D:] = 0.0
    oa, idx = _rows(D, 1000, "perm")
    fpi.flat_grad.fill_(7.0)
    st = fpi.sac_policy_grad(fq1, fq2, oa, idx, 0.0, 1.0, SEED, CALL)
    assert torch.all(fpi.flat_grad == 0.0) and float(st[3]) == 1000
    fpi.sac_policy_grad(fq1, fq2, oa, idx, ALPHA, 1.0, SEED, CALL)  # (and with the entropy term it is not)
    assert float(fpi.flat_grad.abs().max()) > 0.0


@pytest.mark.parametrize("B", [17, 5000])
def test_the_adam_step_on_the_gradient_call_gives_the_bits_of_pds_adam_step(B):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    D = 42
    (pi_a, q1, q2), (fa, fq1, fq2) = _nets(D, (50, 64), (64, 64), "relu", "relu")
    pi_b = copy.deepcopy(pi_a)
    fb = FusedMLP(pi_b, "relu")
    oa, idx = _rows(D, B, "rep")
    for k in range(3):
        fa.sac_policy_grad(fq1, fq2, oa, idx, ALPHA, 1.0, SEED, CALL + k, adam_lr=1e-3)
        fb.sac_policy_grad(fq1, fq2, oa, idx, ALPHA, 1.0, SEED, CALL + k)
        fb.adam_step(1e-3)
        assert torch.equal(fa.flat_grad, fb.flat_grad)
        for a, b in zip(pi_a.parameters(), pi_b.parameters()):
            assert torch.equal(a, b)
        assert torch.equal(fa.exp_avg, fb.exp_avg) and torch.equal(fa.exp_avg_sq, fb.exp_avg_sq)
    assert float((pi_a[0].weight - mc.make_net(D, 50, 64, 8, "relu", 0)[0].weight).detach().abs().max()) > 0  # (the step moved them)


# ---- the backup -----------------------------------------------------------------------------------------------------------------
TARGET_CASES = [(12, (16, 17), (64, 50), "relu", "tanh", 1, None, 1.0), (42, (64, 64), (64, 64), "relu", "relu", 17, "perm", 1.0),
                (40, (50, 50), (17, 1), "tanh", "relu", 15, "rep", 0.5), (60, (1, 64), (64, 64), "tanh", "tanh", 16, "perm", 0.5),
                (48, (64, 64), (50, 50), "relu", "relu", TAIL, "rep", 1.0)]


def _tid(c):
    return f"D{c[0]}-pi{c[1][0]}x{c[1][1]}{c[3]}-q{c[2][0]}x{c[2][1]}{c[4]}-B{c[5]}-{c[6]}-lim{c[7]}"


def _target_inputs(D, B, index, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = B if index is None else 2 * B + 3
    obs2 = torch.randn(rows, D, device=DEV, generator=g)
    rew = torch.randn(rows, device=DEV, generator=g)
    done = (torch.rand(rows, device=DEV, generator=g) < 0.3).float()
    idx = None if index is None else mc.make_index(index, rows, B, seed + 1)
    return obs2, rew, done, idx


def _backup(nets, obs2, rew, done, pos, eps, gamma, alpha, limit, dtype):
    """the backup of compute_loss_q (algs/sac/sac.py:303-311) per POSITION of the mini-batch, in `dtype`"""
    from phoenix_drone_simulation_amd.sac import squashed_sample
    pi, q1, q2 = (copy.deepcopy(n).to(dtype) for n in nets)
    with torch.no_grad():
        o = obs2[pos].to(dtype)
        a2, logp2 = squashed_sample(pi(o), eps.to(dtype), limit)
        oa = torch.cat([o, a2], dim=-1)
        soft = torch.min(q1(oa).squeeze(-1), q2(oa).squeeze(-1)) - alpha * logp2
        return rew[pos].to(dtype) + gamma * (1 - done[pos].to(dtype)) * soft


@pytest.mark.parametrize("case", TARGET_CASES, ids=_tid)
def test_target_matches_float64_and_leaves_other_rows(case, record_property):
    """The backup is written at the ROW and its noise belongs to the POSITION: a row the index names more than once holds the
    backup of one of its positions (whichever was written last), so the row's error is the smallest over its positions."""
    from phoenix_drone_simulation_amd.fused import sac_target
    D, ph, qh, pact, qact, B, index, limit = case
    nets, (fpi, fq1, fq2) = _nets(D, ph, qh, pact, qact)
    obs2, rew, done, idx = _target_inputs(D, B, index)
    rows = obs2.shape[0]
    pos = torch.arange(B, device=DEV) if idx is None else idx
    gamma = 0.99
    eps = _eps(B)
    out = torch.full((rows,), 7.0, device=DEV)
    sac_target(fpi, fq1, fq2, obs2, idx, rew, done, gamma, ALPHA, limit, SEED, CALL, out)
    want = _backup(nets, obs2, rew, done, pos, eps, gamma, ALPHA, limit, torch.float64)
    w32 = _backup(nets, obs2, rew, done, pos, eps, gamma, ALPHA, limit, torch.float32)
    err32 = float((w32.double() - want).abs().max())
    sel = torch.zeros(rows, dtype=torch.bool, device=DEV).index_fill_(0, pos, True)
    bar = 2e-6 + 1e-5 * want.abs()
    ratio = (out.double()[pos] - want).abs() / bar  # per position; per row: the best of its positions
    per_row = torch.full((rows,), float("inf"), device=DEV, dtype=torch.float64).scatter_reduce(0, pos, ratio, "amin")
    margin = float(per_row[sel].max())
    print(f"sac-target {_tid(case)}: margin {margin:.3f} f32 err {err32:.3e} rows written {int(sel.sum())} of {B} positions")
    record_property("margin", margin)
    assert margin <= 1.0, margin
    assert torch.all(out[~sel] == 7.0)  # rows outside the index are untouched
    # done = 1 or gamma = 0: the backup is the reward, bit for bit
    out1 = torch.full_like(out, 7.0)
    sac_target(fpi, fq1, fq2, obs2, idx, rew, torch.ones_like(done), gamma, ALPHA, limit, SEED, CALL, out1)
    assert torch.equal(out1[sel], rew[sel]) and torch.all(out1[~sel] == 7.0)
    out0 = torch.full_like(out, 7.0)
    sac_target(fpi, fq1, fq2, obs2, idx, rew, done, 0.0, ALPHA, limit, SEED, CALL, out0)
    assert torch.equal(out0[sel], rew[sel])
    if index != "rep":  # every row has one position: same inputs, same bits; another call, another noise
        again = torch.full_like(out, 7.0)
        sac_target(fpi, fq1, fq2, obs2, idx, rew, done, gamma, ALPHA, limit, SEED, CALL, again)
        assert torch.equal(again, out)
        sac_target(fpi, fq1, fq2, obs2, idx, rew, done, gamma, ALPHA, limit, SEED, CALL + 1, again)
        live = sel & (done == 0)
        assert not torch.equal(again[live], out[live]) or int(live.sum()) == 0


@pytest.mark.parametrize("case", TARGET_CASES, ids=_tid)
def test_target_without_entropy_and_with_one_q_is_the_ddpg_target_bit_for_bit(case):
    """alpha = 0, q2_targ = q1_targ, the log_std rows forced to -30 (sigma = e^-20): the backup of pds_ddpg_target on the actor
    built from the mu rows."""
    from phoenix_drone_simulation_amd.fused import FusedMLP, ddpg_target, sac_target
    D, ph, qh, pact, qact, B, index, limit = case
    nets, (fpi, fq1, _) = _nets(D, ph, qh, pact, qact, variant=("ls", -30.0))
    pi = nets[0]
    with torch.no_grad():
        pi[4].weight[4:] = 0.0  # (the rows' weights as well: log_std = -30 for every input)
        pi[4].bias[:4] += torch.tensor([2.5, -2.5, 3.0, -3.0], device=DEV)  # |mu| well above sigma |eps| 2^24
    pi4 = mc.make_net(D, ph[0], ph[1], 4, pact, 0)
    with torch.no_grad():
        for dst, src in zip(pi4.parameters(), pi.parameters()):
            dst.copy_(src if dst.shape == src.shape else src[:4])
    f4 = FusedMLP(pi4, pact)
    obs2, rew, done, idx = _target_inputs(D, B, index)
    pos = torch.arange(B, device=DEV) if idx is None else idx
    # on the inputs: sigma eps does not move u off mu in float32
    with torch.no_grad():
        mu = fpi.forward(obs2[pos])[:, :4]
    sigma = torch.exp(torch.tensor(-20.0, device=DEV))
    assert torch.equal(torch.addcmul(mu, sigma.expand_as(mu), _eps(B)), mu)
    a, b = torch.full((obs2.shape[0],), 7.0, device=DEV), torch.full((obs2.shape[0],), 7.0, device=DEV)
    sac_target(fpi, fq1, fq1, obs2, idx, rew, done, 0.99, 0.0, limit, SEED, CALL, a)
    ddpg_target(f4, fq1, obs2, idx, rew, done, 0.99, limit, b)
    assert torch.equal(a, b)


# ---- the elementwise sampler ----------------------------------------------------------------------------------------------------
def _sample64(head, eps, limit):
    from phoenix_drone_simulation_amd.sac import squashed_sample
    return squashed_sample(head.double(), eps.double(), limit)


def _check_sample(head, limit, seed, call, id_base=0, deterministic=False):
    from phoenix_drone_simulation_amd.fused import sac_sample
    n = head.shape[0]
    act, logp = sac_sample(head, limit, seed, call, id_base=id_base, deterministic=deterministic)
    eps = torch.zeros(n, 4, device=DEV) if deterministic else _eps(n, seed, call, id_base)
    a64, l64 = _sample64(head, eps, limit)
    from phoenix_drone_simulation_amd.sac import squashed_sample
    l32 = squashed_sample(head, eps, limit)[1].double()
    # the action: a few float32 roundings of a value within act_limit, and of u (|d tanh / d u| <= 1)
    u_abs = head[:, :4].abs().double() + torch.exp(torch.clamp(head[:, 4:], -20, 2)).double() * eps.abs().double()
    a_bar = 2.0 ** -22 * (limit + limit * u_abs)
    assert bool((act.double() - a64).abs().le(a_bar).all()), float(((act.double() - a64).abs() / a_bar).max())
    assert float(act.abs().max()) <= limit
    # logp: the bar of tests/test_sac_cpu.py -- 32 float32 roundings of the sum of the terms' magnitudes, plus u's carried over
    # (|d logp / d u| <= 2 per dimension)
    u64 = head[:, :4].double() + torch.exp(torch.clamp(head[:, 4:], -20, 2).double()) * eps.double()
    terms = (0.5 * eps.double() ** 2 + torch.clamp(head[:, 4:], -20, 2).abs().double() + 0.5 * math.log(2 * math.pi)
             + 2 * math.log(2) + 2 * u64.abs() + 2 * torch.nn.functional.softplus(-2 * u64))
    scale = terms.sum(-1) + 2 * 4 * u_abs.sum(-1)
    l_bar = 32 * 2.0 ** -24 * scale
    l_err = (logp.double() - l64).abs()
    print(f"sac-sample n {n} limit {limit} det {deterministic}: act err/bar {float(((act.double() - a64).abs() / a_bar).max()):.3f} "
          f"logp err/bar {float((l_err / l_bar).max()):.3f} (torch float32: {float(((l32 - l64).abs() / l_bar).max()):.3f})")
    assert bool(torch.isfinite(logp).all()) and bool(l_err.le(l_bar).all()), float((l_err / l_bar).max())
    return act, logp


@pytest.mark.parametrize("limit", [1.0, 0.5])
def test_sample_matches_float64(limit):
    g = torch.Generator(device=DEV).manual_seed(11)
    n = 1000
    head = torch.randn(n, 8, device=DEV, generator=g)
    head[:, 4:] = head[:, 4:] * 1.5 - 1.0
    _check_sample(head, limit, 99, 3)
    # u = +-30 (sigma tiny), both clamps of log_std with ordinary means, and rows beyond the clamps
    ends = torch.zeros(6, 8, device=DEV)
    ends[0, :4], ends[1, :4] = 30.0, -30.0
    ends[0:2, 4:] = -25.0
    ends[2, 4:], ends[3, 4:], ends[4, 4:], ends[5, 4:] = -20.0, 2.0, -40.0, 9.0
    ends[2:, :4] = torch.tensor([0.3, -0.2, 1.0, -1.0], device=DEV)
    act, logp = _check_sample(ends, limit, 99, 4)
    from phoenix_drone_simulation_amd.fused import sac_sample
    held = ends.clone()
    held[4, 4:], held[5, 4:] = -20.0, 2.0
    act_h, logp_h = sac_sample(held, limit, 99, 4)
    assert torch.equal(act, act_h) and torch.equal(logp, logp_h)  # the clamp holds the value
    assert torch.equal(act[0], torch.full((4,), limit, device=DEV)) and torch.equal(act[1], torch.full((4,), -limit, device=DEV))


def test_sample_deterministic_ids_and_calls():
    from phoenix_drone_simulation_amd.fused import sac_sample
    g = torch.Generator(device=DEV).manual_seed(12)
    n, k = 300, 37
    head = torch.randn(n + k, 8, device=DEV, generator=g)
    act, _ = _check_sample(head, 0.5, 5, 9, deterministic=True)
    assert torch.allclose(act, 0.5 * torch.tanh(head[:, :4]), rtol=0, atol=2.0 ** -22)  # a = act_limit tanh(mu)
    a0, l0 = sac_sample(head, 1.0, 5, 9)
    a1, l1 = sac_sample(head, 1.0, 5, 10)            # another call
    a2, l2 = sac_sample(head, 1.0, 6, 9)             # another seed
    a3, l3 = sac_sample(head[:n], 1.0, 5, 9, id_base=k)  # another id base
    assert not torch.equal(a0, a1) and not torch.equal(a0, a2) and not torch.equal(a0[:n], a3)
    assert bool((l0 != l1).all()) and bool((l0[:n] != l3).all())  # every row's noise changed
    # row i under id_base = k is row i + k under id_base = 0 (the same head row under both)
    a4, l4 = sac_sample(head[k:].contiguous(), 1.0, 5, 9, id_base=k)
    assert torch.equal(a4, a0[k:]) and torch.equal(l4, l0[k:])
    # no log-probability asked for: the actions are the same
    a5, l5 = sac_sample(head, 1.0, 5, 9, want_logp=False)
    assert l5 is None and torch.equal(a5, a0)


def test_argument_checks():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.fused import _ptr
    nat = pds.native
    lib = nat.load()
    D = 42
    nets, (fpi, fq1, fq2) = _nets(D, (50, 50), (64, 64), "relu", "relu")
    oa = torch.zeros(16, D + 4, device=DEV)
    obs2 = torch.zeros(16, D, device=DEV)
    head = torch.zeros(16, 8, device=DEV)
    r = torch.zeros(16, device=DEV)
    out = torch.full((16,), 7.0, device=DEV)
    act = torch.full((16, 4), 7.0, device=DEV)
    grads = torch.full_like(fpi.flat_grad, 7.0)
    stats = torch.full((4,), 7.0, device=DEV)
    P, Q1, Q2 = C.byref(fpi.m), C.byref(fq1.m), C.byref(fq2.m)
    n = lib.pds_sac_workspace_floats(P, Q1, Q2)
    assert n == 256 * 3 * (fpi.flat_grad.numel() + 4)
    ws = torch.empty(n, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def grad(pi_=P, q1_=Q1, q2_=Q2, oa_=_ptr(oa), B=16, g=_ptr(grads), st=_ptr(stats), w=_ptr(ws)):
        return lib.pds_sac_policy_grad(pi_, q1_, q2_, oa_, None, B, 0.2, 1.0, 1, 1, g, st, w, None, s)

    def target(pi_=P, q1_=Q1, q2_=Q2, o=_ptr(obs2), B=16, rew=_ptr(r), done=_ptr(r), t=_ptr(out)):
        return lib.pds_sac_target(pi_, q1_, q2_, o, None, B, rew, done, 0.99, 0.2, 1.0, 1, 1, t, s)

    def sample(h=_ptr(head), n_=16, a=_ptr(act), id_base=0):
        return lib.pds_sac_sample(h, n_, 1.0, 1, 1, id_base, 0, a, None, s)

    assert lib.pds_sac_supported(P, Q1, Q2) == 1
    for kw in (dict(pi_=None), dict(q1_=None), dict(q2_=None), dict(oa_=None), dict(B=0), dict(g=None), dict(st=None), dict(w=None)):
        assert grad(**kw) == nat.EINVAL, kw
    for kw in (dict(pi_=None), dict(q1_=None), dict(q2_=None), dict(o=None), dict(B=0), dict(rew=None), dict(done=None), dict(t=None)):
        assert target(**kw) == nat.EINVAL, kw
    for kw in (dict(h=None), dict(n_=0), dict(a=None), dict(id_base=(1 << 56) - 15)):
        assert sample(**kw) == nat.EINVAL, kw
    assert lib.pds_sac_supported(None, Q1, Q2) == 0 and lib.pds_sac_workspace_floats(P, None, Q2) == nat.EINVAL
    bad_pi = nat.Mlp.from_buffer_copy(fpi.m); bad_pi.d_out = 4
    bad_q = nat.Mlp.from_buffer_copy(fq1.m); bad_q.d_out = 2
    off_q = nat.Mlp.from_buffer_copy(fq1.m); off_q.d_in = D + 3
    shape_q = nat.Mlp.from_buffer_copy(fq2.m); shape_q.h1 = 63
    act_q = nat.Mlp.from_buffer_copy(fq2.m); act_q.activation = 1
    for kw in (dict(pi_=C.byref(bad_pi)), dict(q1_=C.byref(bad_q)), dict(q2_=C.byref(bad_q)), dict(q1_=C.byref(off_q)),
               dict(q2_=C.byref(off_q)), dict(q2_=C.byref(shape_q)), dict(q2_=C.byref(act_q))):
        assert grad(**kw) == nat.EINVAL and target(**kw) == nat.EINVAL, kw
        assert lib.pds_sac_supported(kw.get("pi_", P), kw.get("q1_", Q1), kw.get("q2_", Q2)) == 0
    # D + 4 = 65: a shape pds_mlp covers, these kernels do not
    wide_pi = nat.Mlp.from_buffer_copy(fpi.m); wide_pi.d_in = 61
    wide_q1 = nat.Mlp.from_buffer_copy(fq1.m); wide_q1.d_in = 65
    wide_q2 = nat.Mlp.from_buffer_copy(fq2.m); wide_q2.d_in = 65
    W = dict(pi_=C.byref(wide_pi), q1_=C.byref(wide_q1), q2_=C.byref(wide_q2))
    assert grad(**W) == nat.EUNSUPPORTED and target(**W) == nat.EUNSUPPORTED
    assert lib.pds_sac_supported(W["pi_"], W["q1_"], W["q2_"]) == 0
    assert lib.pds_sac_workspace_floats(W["pi_"], W["q1_"], W["q2_"]) == nat.EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(grads == 7.0) and torch.all(stats == 7.0) and torch.all(out == 7.0) and torch.all(act == 7.0)
