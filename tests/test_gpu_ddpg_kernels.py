"""The DDPG kernels of csrc/pds_ddpg.hip on the device: the deterministic policy gradient against float64 autograd of
-q(cat(o, limit * tanh(pi(o)))).mean(), the Bellman backup against float64, the polyak step against the two torch in-place
ops bit for bit, and the argument checks.

Bars.  Gradient: mlp_cases.grad_atol (2e-6 of the largest entry) with rtol 2e-4, the project's bar for this MFMA chain
(tests/test_gpu_mlp_dispatch.py _check_mse); the chain here is two networks deep.  sum Q and the backup: the forward bar of
tests/test_gpu_mlp_dispatch.py (rtol 1e-5, atol 2e-6 per sample; summed over the batch for sum Q).  What was measured against
them is in profiles/ddpg_parity_margins.txt; every case also records its margin (error / bar) as a test property."""
import copy
import ctypes as C

import pytest
import torch

import mlp_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAIL = 2 * mc.WIDE_ROUND + 16 * 3 + 5  # a ragged batch past two rounds of the persistent grid (256 blocks x 4 waves x 16)

# D, actor hidden, Q hidden, actor act, Q act, B, index, act_limit
GRAD_CASES = [
    (12, (16, 17), (64, 50), "relu", "tanh", 1, None, 1.0),
    (13, (1, 16), (17, 1), "tanh", "relu", 15, "perm", 0.5),
    (40, (50, 50), (64, 64), "relu", "relu", 16, "rep", 1.0),
    (42, (64, 64), (64, 64), "relu", "relu", 17, None, 1.0),
    (48, (17, 64), (50, 16), "tanh", "tanh", 17, "perm", 0.5),
    (60, (64, 1), (1, 64), "relu", "tanh", 16, "rep", 1.0),
    (60, (50, 17), (16, 50), "tanh", "relu", 1, None, 0.5),
    (12, (64, 64), (64, 64), "tanh", "tanh", 15, "rep", 1.0),
    (34, (64, 64), (64, 64), "relu", "relu", 128, "rep", 1.0),   # Hover at the trainer's defaults
    (40, (16, 50), (50, 64), "relu", "tanh", 4099, "rep", 0.5),
    (42, (64, 64), (64, 64), "relu", "relu", TAIL, "perm", 1.0),
    (48, (50, 50), (64, 64), "tanh", "relu", TAIL + 11, None, 0.5),
]


def _id(c):
    return f"D{c[0]}-pi{c[1][0]}x{c[1][1]}{c[3]}-q{c[2][0]}x{c[2][1]}{c[4]}-B{c[5]}-{c[6]}-lim{c[7]}"


def _nets(D, ph, qh, pact, qact, seed=0):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    pi = mc.make_net(D, ph[0], ph[1], 4, pact, seed)
    q = mc.make_net(D + 4, qh[0], qh[1], 1, qact, seed + 1)
    return pi, q, FusedMLP(pi, pact), FusedMLP(q, qact)


def _rows(D, B, index, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = B if index is None else 2 * B + 3
    oa = torch.randn(rows, D + 4, device=DEV, generator=g)
    idx = None if index is None else mc.make_index(index, rows, B, seed + 1)
    return oa, idx


def _ref_grad(pi, q, oa, idx, D, limit):
    """float64 autograd of compute_loss_pi (algs/ddpg/ddpg.py:336-340) -> (flat actor gradient, Q values)"""
    p64, q64 = mc.net64(pi), mc.net64(q)
    o = (oa if idx is None else oa[idx])[:, :D].double()
    qv = q64(torch.cat([o, limit * torch.tanh(p64(o))], dim=-1)).squeeze(-1)
    (-qv.mean()).backward()
    return torch.cat([p.grad.reshape(-1) for p in p64.parameters()]), qv.detach()


@pytest.mark.parametrize("case", GRAD_CASES, ids=_id)
def test_policy_gradient_matches_float64_autograd(case, record_property):
    D, ph, qh, pact, qact, B, index, limit = case
    pi, q, fpi, fq = _nets(D, ph, qh, pact, qact)
    oa, idx = _rows(D, B, index)
    q_before = [p.detach().clone() for p in q.parameters()]
    st = fpi.ddpg_policy_grad(fq, oa, idx, limit).clone()
    got = fpi.flat_grad.clone()
    want, qv = _ref_grad(pi, q, oa, idx, D, limit)
    atol = mc.grad_atol(want, B)
    err = float((got.double() - want).abs().max())
    q_bar = 1e-5 * float(qv.abs().sum()) + 2e-6 * B
    q_err = abs(float(st[0].double()) - float(qv.sum()))
    print(f"ddpg-grad {_id(case)}: err {err:.3e} atol {atol:.3e} max|g| {float(want.abs().max()):.3e} "
          f"sumQ err {q_err:.3e} bar {q_bar:.3e}")
    record_property("margin", float(((got.double() - want).abs() / (atol + 2e-4 * want.abs())).max()))
    assert torch.allclose(got.double(), want, rtol=2e-4, atol=atol), (err, atol)
    assert q_err <= q_bar, (q_err, q_bar)
    assert float(st[3]) == B and float(st[1]) == 0.0 and float(st[2]) == 0.0
    # same inputs, same bits; Q is only read
    st2 = fpi.ddpg_policy_grad(fq, oa, idx, limit)
    assert torch.equal(fpi.flat_grad, got) and torch.equal(st2, st)
    assert all(torch.equal(a, b) for a, b in zip(q_before, q.parameters()))


@pytest.mark.parametrize("pact,qact", [("relu", "relu"), ("tanh", "tanh")])
def test_zeroed_action_columns_give_a_gradient_of_exactly_zero(pact, qact):
    D = 42
    pi, q, fpi, fq = _nets(D, (50, 50), (64, 64), pact, qact)
    with torch.no_grad():
        q[0].weight[:, D:] = 0.0
    oa, idx = _rows(D, 1000, "perm")
    fpi.flat_grad.fill_(7.0)
    fpi.ddpg_policy_grad(fq, oa, idx, 1.0)
    assert torch.all(fpi.flat_grad == 0.0)


@pytest.mark.parametrize("B", [17, 5000])
def test_the_adam_step_on_the_gradient_call_gives_the_bits_of_pds_adam_step(B):
    D = 42
    pi_a, q, fa, fq = _nets(D, (50, 64), (64, 64), "relu", "relu")
    pi_b = copy.deepcopy(pi_a)
    from phoenix_drone_simulation_amd.fused import FusedMLP
    fb = FusedMLP(pi_b, "relu")
    oa, idx = _rows(D, B, "rep")
    for _ in range(3):
        fa.ddpg_policy_grad(fq, oa, idx, 1.0, adam_lr=1e-3)
        fb.ddpg_policy_grad(fq, oa, idx, 1.0)
        fb.adam_step(1e-3)
        assert torch.equal(fa.flat_grad, fb.flat_grad)
        for a, b in zip(pi_a.parameters(), pi_b.parameters()):
            assert torch.equal(a, b)
        assert torch.equal(fa.exp_avg, fb.exp_avg) and torch.equal(fa.exp_avg_sq, fb.exp_avg_sq)
    assert float((pi_a[0].weight - mc.make_net(D, 50, 64, 4, "relu", 0)[0].weight).detach().abs().max()) > 0  # (the step moved them)


TARGET_CASES = [(12, (16, 17), (64, 50), "relu", "tanh", 1, None, 1.0), (42, (64, 64), (64, 64), "relu", "relu", 17, "perm", 1.0),
                (40, (50, 50), (17, 1), "tanh", "relu", 15, "rep", 0.5), (60, (1, 64), (64, 64), "tanh", "tanh", 16, "perm", 0.5),
                (48, (64, 64), (50, 50), "relu", "relu", TAIL, "rep", 1.0)]


def _target_inputs(D, B, index, seed=5):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = B if index is None else 2 * B + 3
    obs2 = torch.randn(rows, D, device=DEV, generator=g)
    rew = torch.randn(rows, device=DEV, generator=g)
    done = (torch.rand(rows, device=DEV, generator=g) < 0.3).float()
    idx = None if index is None else mc.make_index(index, rows, B, seed + 1)
    return obs2, rew, done, idx


@pytest.mark.parametrize("case", TARGET_CASES, ids=_id)
def test_target_matches_float64_and_leaves_other_rows(case, record_property):
    from phoenix_drone_simulation_amd.fused import ddpg_target
    D, ph, qh, pact, qact, B, index, limit = case
    pi, q, fpi, fq = _nets(D, ph, qh, pact, qact)
    obs2, rew, done, idx = _target_inputs(D, B, index)
    gamma = 0.99
    out = torch.full((obs2.shape[0],), 7.0, device=DEV)
    ddpg_target(fpi, fq, obs2, idx, rew, done, gamma, limit, out)
    p64, q64 = mc.net64(pi), mc.net64(q)
    with torch.no_grad():
        o = obs2.double()
        qv = q64(torch.cat([o, limit * torch.tanh(p64(o))], dim=-1)).squeeze(-1)
        want = rew.double() + gamma * (1 - done.double()) * qv
    sel = torch.ones_like(done, dtype=torch.bool) if idx is None else torch.zeros_like(done, dtype=torch.bool).index_fill_(0, idx, True)
    err = (out.double() - want).abs()[sel]
    margin = float((err / (2e-6 + 1e-5 * want.abs()[sel])).max())
    print(f"ddpg-target {_id(case)}: err {float(err.max()):.3e} margin {margin:.3f}")
    record_property("margin", margin)
    assert torch.allclose(out.double()[sel], want[sel], rtol=1e-5, atol=2e-6), float(err.max())
    assert torch.all(out[~sel] == 7.0)  # rows outside the index are untouched
    # done = 1 or gamma = 0: the backup is the reward, bit for bit
    out1 = torch.full_like(out, 7.0)
    ddpg_target(fpi, fq, obs2, idx, rew, torch.ones_like(done), gamma, limit, out1)
    assert torch.equal(out1[sel], rew[sel]) and torch.all(out1[~sel] == 7.0)
    out0 = torch.full_like(out, 7.0)
    ddpg_target(fpi, fq, obs2, idx, rew, done, 0.0, limit, out0)
    assert torch.equal(out0[sel], rew[sel])
    # what the fused Q update reads: target[index[g]]
    again = torch.full_like(out, 7.0)
    ddpg_target(fpi, fq, obs2, idx, rew, done, gamma, limit, again)
    assert torch.equal(again, out)


@pytest.mark.parametrize("rho", [0.995, 0.5])
def test_polyak_is_bitwise_the_two_torch_inplace_ops(rho):
    from phoenix_drone_simulation_amd.fused import FusedMLP, polyak
    src = mc.make_net(13, 17, 33, 3, "relu", 0)
    targ = mc.make_net(13, 17, 33, 3, "relu", 1)
    want = copy.deepcopy(targ)
    ft, fs = FusedMLP(targ, "relu"), FusedMLP(src, "relu")
    src_before = [p.detach().clone() for p in src.parameters()]
    for _ in range(3):
        polyak(ft, fs, rho)
        with torch.no_grad():
            for p, p_targ in zip(src.parameters(), want.parameters()):
                p_targ.data.mul_(rho)
                p_targ.data.add_((1 - rho) * p.data)
        for a, b in zip(targ.parameters(), want.parameters()):
            assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(src_before, src.parameters()))


def test_argument_checks():
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.fused import _ptr
    nat = pds.native
    lib = nat.load()
    D = 42
    pi, q, fpi, fq = _nets(D, (50, 50), (64, 64), "relu", "relu")
    oa = torch.zeros(16, D + 4, device=DEV)
    obs2 = torch.zeros(16, D, device=DEV)
    r = torch.zeros(16, device=DEV)
    out = torch.full((16,), 7.0, device=DEV)
    grads = torch.full_like(fpi.flat_grad, 7.0)
    stats = torch.full((4,), 7.0, device=DEV)
    n = lib.pds_ddpg_workspace_floats(C.byref(fpi.m), C.byref(fq.m))
    assert n == 256 * 4 * (fpi.flat_grad.numel() + 4)
    ws = torch.empty(n, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, Q = C.byref(fpi.m), C.byref(fq.m)

    def grad(pi_=P, q_=Q, oa_=_ptr(oa), B=16, g=_ptr(grads), st=_ptr(stats), w=_ptr(ws)):
        return lib.pds_ddpg_policy_grad(pi_, q_, oa_, None, B, 1.0, g, st, w, None, s)

    def target(pi_=P, q_=Q, o=_ptr(obs2), B=16, rew=_ptr(r), done=_ptr(r), t=_ptr(out)):
        return lib.pds_ddpg_target(pi_, q_, o, None, B, rew, done, 0.99, 1.0, t, s)

    assert lib.pds_ddpg_supported(P, Q) == 1
    for kw in (dict(pi_=None), dict(q_=None), dict(oa_=None), dict(B=0), dict(g=None), dict(st=None), dict(w=None)):
        assert grad(**kw) == nat.EINVAL, kw
    for kw in (dict(pi_=None), dict(q_=None), dict(o=None), dict(B=0), dict(rew=None), dict(done=None), dict(t=None)):
        assert target(**kw) == nat.EINVAL, kw
    bad_pi = nat.Mlp.from_buffer_copy(fpi.m); bad_pi.d_out = 3
    bad_q = nat.Mlp.from_buffer_copy(fq.m); bad_q.d_out = 2
    off_q = nat.Mlp.from_buffer_copy(fq.m); off_q.d_in = D + 3
    for kw in (dict(pi_=C.byref(bad_pi)), dict(q_=C.byref(bad_q)), dict(q_=C.byref(off_q))):
        assert grad(**kw) == nat.EINVAL and target(**kw) == nat.EINVAL, kw
        assert lib.pds_ddpg_supported(kw.get("pi_", P), kw.get("q_", Q)) == 0
    # D + 4 = 65: a shape pds_mlp covers, this kernel does not
    wide_pi = nat.Mlp.from_buffer_copy(fpi.m); wide_pi.d_in = 61
    wide_q = nat.Mlp.from_buffer_copy(fq.m); wide_q.d_in = 65
    assert grad(pi_=C.byref(wide_pi), q_=C.byref(wide_q)) == nat.EUNSUPPORTED
    assert target(pi_=C.byref(wide_pi), q_=C.byref(wide_q)) == nat.EUNSUPPORTED
    assert lib.pds_ddpg_supported(C.byref(wide_pi), C.byref(wide_q)) == 0
    assert lib.pds_ddpg_workspace_floats(C.byref(wide_pi), C.byref(wide_q)) == nat.EUNSUPPORTED
    other = nat.Mlp.from_buffer_copy(fpi.m); other.h1 = 49
    assert lib.pds_polyak(P, C.byref(other), 0.995, s) == nat.EINVAL
    assert lib.pds_polyak(P, None, 0.995, s) == nat.EINVAL and lib.pds_polyak(P, P, 1.5, s) == nat.EINVAL
    torch.cuda.synchronize()
    assert torch.all(grads == 7.0) and torch.all(stats == 7.0) and torch.all(out == 7.0)
