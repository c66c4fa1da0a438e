"""The kernels of include/pds_mlp_broad.h (csrc/pds_mlp_broad.hip, csrc/pds_ddpg_broad.hip) on the device, the five properties of
tests/test_gpu_ddpg_kernels.py at hidden widths above 64: the deterministic policy gradient and the value gradient against
float64 autograd of the reference's compute_loss_pi / compute_loss_q, the forward and the Bellman backup against float64, the
polyak step against the two torch in-place ops bit for bit, the exactness properties, and the argument checks.

Bars.  The existing bars were set for sums of at most 64 terms; here a sum has up to 512.  So the bar of every quantity is 4 UNITS,
the unit being the error of torch's own float32 arithmetic against the same float64, the largest over the case table, in the
measure of tests/ddpg_broad_cases.py -- measured on the device by profiles/tools/ddpg_broad_margins.py and entered below from
profiles/ddpg_broad_parity_margins.txt, which also holds the kernels' own errors -- and never below the floor the existing bars
admit (2e-6).  Every case records its margin (error / bar) as a test property."""
import copy
import ctypes as C

import pytest
import torch

import ddpg_broad_cases as bc

pytestmark = pytest.mark.gpu
DEV = bc.DEV

# profiles/ddpg_broad_parity_margins.txt, KERNEL_UNITS: the largest float32-torch error against float64 over the case table
KERNEL_UNITS = {
    "pi_grad.W1": 9.060e-07,
    "pi_grad.b1": 8.722e-07,
    "pi_grad.W2": 1.495e-06,
    "pi_grad.b2": 6.909e-07,
    "pi_grad.W3": 6.601e-07,
    "pi_grad.b3": 6.703e-07,
    "sum_q": 1.043e-07,
    "q_grad.W1": 1.337e-06,
    "q_grad.b1": 1.620e-06,
    "q_grad.W2": 1.406e-06,
    "q_grad.b2": 1.254e-06,
    "q_grad.W3": 1.479e-06,
    "q_grad.b3": 3.304e-06,
    "sum_sq_err": 2.912e-08,
    "forward": 3.157e-07,
    "target": 2.051e-07,
}

_measured = {}


def _measure(c):
    """every quantity of a case, computed once and shared by the four tests that read it"""
    key = bc.case_id(c)
    if key not in _measured:
        _measured[key] = bc.measure(c)
    return _measured[key]


def _check(c, quantities, record_property):
    m = _measure(c)
    worst = 0.0
    for k in quantities:
        err, f32 = m[k]
        b = bc.bar(KERNEL_UNITS, k)
        print(f"{bc.case_id(c)} {k}: kernel {err:.3e} float32-torch {f32:.3e} bar {b:.3e} margin {err / b:.3f}")
        worst = max(worst, err / b)
    record_property("margin", worst)
    for k in quantities:
        assert m[k][0] <= bc.bar(KERNEL_UNITS, k), (k, m[k], bc.bar(KERNEL_UNITS, k))


def test_the_units_table_names_every_quantity():
    assert sorted(KERNEL_UNITS) == sorted(bc.QUANTITIES) and all(0.0 <= u < 1e-3 for u in KERNEL_UNITS.values())


@pytest.mark.parametrize("c", bc.CASES, ids=bc.case_id)
def test_policy_gradient_and_sum_q_match_float64_autograd(c, record_property):
    _check(c, ["pi_grad." + n for n in bc.TENSORS] + ["sum_q"], record_property)


@pytest.mark.parametrize("c", bc.CASES, ids=bc.case_id)
def test_value_gradient_matches_float64_autograd(c, record_property):
    _check(c, ["q_grad." + n for n in bc.TENSORS] + ["sum_sq_err"], record_property)


@pytest.mark.parametrize("c", bc.CASES, ids=bc.case_id)
def test_forward_matches_float64(c, record_property):
    _check(c, ["forward"], record_property)


@pytest.mark.parametrize("c", bc.CASES, ids=bc.case_id)
def test_target_matches_float64(c, record_property):
    _check(c, ["target"], record_property)


def test_the_largest_batch_the_workspace_holds(record_property):
    """65533 samples through a repeating index: 2048 two-tile chain blocks with a ragged last one, 16 parts of the weight-gradient
    sum with a short last part.  tanh networks, so that no relu kink of a sample decides the comparison; the bars of the table."""
    c = bc.Case(bc.Shape("largest", (65, 64), (64, 65), "tanh", "tanh"), 34, 65533, "rep", 1.0)
    _check(c, ["pi_grad." + n for n in bc.TENSORS] + ["sum_q"] + ["q_grad." + n for n in bc.TENSORS] + ["sum_sq_err", "forward", "target"],
           record_property)


def test_the_float64_reference_has_teeth():
    """a kernel that dropped the bias column of its weight-gradient strips, or ran the actor's backward on Q's activations, would
    sit far outside the bars: zeroing b2's gradient, and using act'(H) of a differently seeded actor, each move the measure by more
    than 100 bars"""
    c = bc.CASES[2]
    pi, q, fpi, fq = bc.nets(c)
    oa, _, _, _, idx = bc.rows(c)
    want, _ = bc.policy_grad_ref(pi, q, oa, idx, c.D, c.limit, torch.float64)
    w = bc.split_flat(want, pi)
    assert bc.tensor_error(torch.zeros_like(w["b2"]), w["b2"]) > 100 * bc.bar(KERNEL_UNITS, "pi_grad.b2")
    other, _ = bc.policy_grad_ref(bc.nets(c, seed=5)[0], q, oa, idx, c.D, c.limit, torch.float64)
    assert bc.tensor_error(bc.split_flat(other, pi)["W2"], w["W2"]) > 100 * bc.bar(KERNEL_UNITS, "pi_grad.W2")


# ---- exactness: no tolerance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 3, 15, 21], ids=lambda i: bc.case_id(bc.CASES[i]))
def test_statistics_count_and_q_is_only_read(ci):
    c = bc.CASES[ci]
    pi, q, fpi, fq = bc.nets(c)
    oa, _, _, _, idx = bc.rows(c)
    q_before = [p.detach().clone() for p in q.parameters()]
    oa_before = oa.clone()
    st = fpi.ddpg_policy_grad(fq, oa, idx, c.limit)
    assert float(st[3]) == c.B and float(st[1]) == 0.0 and float(st[2]) == 0.0
    assert all(torch.equal(a, b) for a, b in zip(q_before, q.parameters())) and torch.equal(oa, oa_before)
    # the stored actions are never read: other actions, the same bits
    got = fpi.flat_grad.clone()
    oa[:, c.D:] = 123.0
    fpi.ddpg_policy_grad(fq, oa, idx, c.limit)
    assert torch.equal(fpi.flat_grad, got)


@pytest.mark.parametrize("name", ["default", "corner", "odd-first"])
def test_zeroed_action_columns_give_a_gradient_of_exactly_zero(name):
    c = next(c for c in bc.CASES if c.shape.name == name and c.B == 1000)
    pi, q, fpi, fq = bc.nets(c)
    with torch.no_grad():
        q[0].weight[:, c.D:] = 0.0
    oa, _, _, _, idx = bc.rows(c)
    fpi.flat_grad.fill_(7.0)
    fpi.ddpg_policy_grad(fq, oa, idx, c.limit)
    assert torch.all(fpi.flat_grad == 0.0)


@pytest.mark.parametrize("B", [128, 1000])
def test_the_gradient_calls_give_the_same_bits_twice(B):
    c = next(c for c in bc.CASES if c.shape.name == "default" and c.B == B)
    pi, q, fpi, fq = bc.nets(c)
    oa, _, _, _, idx = bc.rows(c)
    target_rows = torch.randn(oa.shape[0], device=DEV)
    st = fpi.ddpg_policy_grad(fq, oa, idx, c.limit).clone()
    g = fpi.flat_grad.clone()
    sq = fq.value_grad(oa, target_rows, index=idx).clone()
    gq = fq.flat_grad.clone()
    assert float(g.abs().max()) > 0 and float(gq.abs().max()) > 0
    fpi.flat_grad.fill_(7.0); fq.flat_grad.fill_(7.0)
    assert torch.equal(fpi.ddpg_policy_grad(fq, oa, idx, c.limit), st) and torch.equal(fpi.flat_grad, g)
    assert torch.equal(fq.value_grad(oa, target_rows, index=idx), sq) and torch.equal(fq.flat_grad, gq)


@pytest.mark.parametrize("B", [17, 1000])
def test_the_adam_step_on_a_gradient_call_gives_the_bits_of_pds_mlp_broad_adam_step(B):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    c = next(c for c in bc.CASES if c.shape.name == "default" and c.B == B)
    pi_a, q_a, fa, fqa = bc.nets(c)
    pi_b, q_b = copy.deepcopy(pi_a), copy.deepcopy(q_a)
    fb, fqb = FusedMLP(pi_b, c.shape.pact, broad=True), FusedMLP(q_b, c.shape.qact, broad=True)
    pi_0 = copy.deepcopy(pi_a)
    oa, _, _, _, idx = bc.rows(c)
    target_rows = torch.randn(oa.shape[0], device=DEV)
    for _ in range(3):
        fa.ddpg_policy_grad(fqa, oa, idx, 1.0, adam_lr=1e-3)
        fb.ddpg_policy_grad(fqb, oa, idx, 1.0)
        fb.adam_step(1e-3)
        fqa.value_grad(oa, target_rows, index=idx, adam_lr=1e-3)
        fqb.value_grad(oa, target_rows, index=idx)
        fqb.adam_step(1e-3)
        for x, y in ((fa, fb), (fqa, fqb)):
            assert torch.equal(x.flat_grad, y.flat_grad)
            assert torch.equal(x.exp_avg, y.exp_avg) and torch.equal(x.exp_avg_sq, y.exp_avg_sq)
        for a, b in zip(list(pi_a.parameters()) + list(q_a.parameters()), list(pi_b.parameters()) + list(q_b.parameters())):
            assert torch.equal(a, b)
    assert float((pi_a[0].weight - pi_0[0].weight).detach().abs().max()) > 0  # (the step moved them)


@pytest.mark.parametrize("rho", [0.0, 0.995, 1.0])
def test_polyak_is_bitwise_the_two_torch_inplace_ops(rho):
    from phoenix_drone_simulation_amd.fused import FusedMLP, polyak
    import mlp_cases as mc
    src, targ = mc.make_net(13, 300, 65, 3, "relu", 0), mc.make_net(13, 300, 65, 3, "relu", 1)
    want = copy.deepcopy(targ)
    ft, fs = FusedMLP(targ, "relu", broad=True), FusedMLP(src, "relu", broad=True)
    assert ft.broad and fs.broad
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


@pytest.mark.parametrize("B", [17, 128, 1000])
def test_target_leaves_other_rows_and_writes_the_same_bits_for_repeats(B):
    from phoenix_drone_simulation_amd.fused import ddpg_target
    c = next(c for c in bc.CASES if c.index == "rep" and c.B == B)
    pi, q, fpi, fq = bc.nets(c)
    _, obs2, rew, done, idx = bc.rows(c)
    sel = torch.zeros_like(done, dtype=torch.bool).index_fill_(0, idx, True)
    out = torch.full_like(rew, 7.0)
    ddpg_target(fpi, fq, obs2, idx, rew, done, 0.99, c.limit, out)
    assert torch.all(out[~sel] == 7.0) and bool((~sel).any()) and torch.all(out[sel] != 7.0)
    # every selected row once, without an index: the same bits as through an index that may repeat rows
    once = torch.full_like(rew, 7.0)
    rows_sel = torch.nonzero(sel).squeeze(-1)
    ddpg_target(fpi, fq, obs2, rows_sel, rew, done, 0.99, c.limit, once)
    assert torch.equal(once, out)
    # done = 1 or gamma = 0: the backup is the reward, bit for bit
    out1 = torch.full_like(rew, 7.0)
    ddpg_target(fpi, fq, obs2, idx, rew, torch.ones_like(done), 0.99, c.limit, out1)
    assert torch.equal(out1[sel], rew[sel]) and torch.all(out1[~sel] == 7.0)
    out0 = torch.full_like(rew, 7.0)
    ddpg_target(fpi, fq, obs2, idx, rew, done, 0.0, c.limit, out0)
    assert torch.equal(out0[sel], rew[sel])


def test_the_keyword_changes_nothing_at_64_and_is_needed_above():
    from phoenix_drone_simulation_amd.fused import FusedMLP, ddpg_supported
    import mlp_cases as mc
    net = mc.make_net(42, 64, 64, 4, "relu", 0)
    a, b = FusedMLP(net, "relu"), FusedMLP(copy.deepcopy(net), "relu", broad=True)
    assert not a.broad and not b.broad and a._names == b._names
    x = torch.randn(33, 42, device=DEV)
    assert torch.equal(a.forward(x), b.forward(x))
    big = mc.make_net(42, 400, 300, 4, "relu", 0)
    with pytest.raises(ValueError, match="outside the fused kernels' range"):
        FusedMLP(big, "relu")
    fb = FusedMLP(big, "relu", broad=True)
    assert fb.broad and fb.workspace is None  # (allocated by the first gradient call)
    with pytest.raises(NotImplementedError):
        fb.ppo_grad(x, x[:, :4], x[:, 0], x[:, 0], torch.zeros(4, device=DEV), 0.2)
    q64 = FusedMLP(mc.make_net(46, 64, 64, 1, "relu", 1), "relu", broad=True)
    assert not ddpg_supported(fb, q64) and not ddpg_supported(b, FusedMLP(mc.make_net(46, 400, 300, 1, "relu", 1), "relu", broad=True))


def test_argument_checks_leave_the_outputs_alone():
    """the codes of tests/test_mlp_broad_cpu.py, here with real tensors: nothing is written by a refused call; a (64, 64) pair is
    PDS_EINVAL with the text that names the entry points of include/pds.h"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.fused import _ptr
    nat = pds.native
    lib = nat.load()
    c = bc.CASES[0]
    D = c.D
    pi, q, fpi, fq = bc.nets(c)
    _, _, f64pi, f64q = bc.nets(bc.Case(bc.Shape("narrow", (64, 64), (64, 64), "relu", "relu"), D, 16, None, 1.0), broad=False)
    oa, obs2, r = torch.zeros(16, D + 4, device=DEV), torch.zeros(16, D, device=DEV), torch.zeros(16, device=DEV)
    out = torch.full((16,), 7.0, device=DEV)
    grads, stats = torch.full_like(fpi.flat_grad, 7.0), torch.full((4,), 7.0, device=DEV)
    ws = torch.empty(1 << 20, device=DEV)  # (never read: every call below is refused)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Pm, Qm = C.byref(fpi.m), C.byref(fq.m)

    def grad(pi_=Pm, q_=Qm, oa_=_ptr(oa), B=16, g=_ptr(grads), st=_ptr(stats), w=_ptr(ws)):
        return lib.pds_ddpg_broad_policy_grad(pi_, q_, oa_, None, B, 1.0, g, st, w, None, s)

    def target(pi_=Pm, q_=Qm, o=_ptr(obs2), B=16, rew=_ptr(r), done=_ptr(r), t=_ptr(out)):
        return lib.pds_ddpg_broad_target(pi_, q_, o, None, B, rew, done, 0.99, 1.0, t, s)

    assert lib.pds_ddpg_broad_supported(Pm, Qm) == 1
    for kw in (dict(pi_=None), dict(q_=None), dict(oa_=None), dict(B=0), dict(g=None), dict(st=None), dict(w=None)):
        assert grad(**kw) == nat.EINVAL, kw
    for kw in (dict(pi_=None), dict(q_=None), dict(o=None), dict(B=0), dict(rew=None), dict(done=None), dict(t=None)):
        assert target(**kw) == nat.EINVAL, kw
    bad_pi = nat.Mlp.from_buffer_copy(fpi.m); bad_pi.d_out = 3
    bad_q = nat.Mlp.from_buffer_copy(fq.m); bad_q.d_out = 2
    off_q = nat.Mlp.from_buffer_copy(fq.m); off_q.d_in = D + 3
    for kw in (dict(pi_=C.byref(bad_pi)), dict(q_=C.byref(bad_q)), dict(q_=C.byref(off_q))):
        assert grad(**kw) == nat.EINVAL and target(**kw) == nat.EINVAL, kw
    assert grad(pi_=C.byref(f64pi.m), q_=C.byref(f64q.m)) == nat.EINVAL and target(pi_=C.byref(f64pi.m), q_=C.byref(f64q.m)) == nat.EINVAL
    text = lib.pds_last_error(None)
    assert b"pds_ddpg_policy_grad" in text and b"pds_ddpg_target" in text and b"pds_polyak" in text
    wide_pi = nat.Mlp.from_buffer_copy(fpi.m); wide_pi.d_in = 61
    wide_q = nat.Mlp.from_buffer_copy(fq.m); wide_q.d_in = 65
    assert grad(pi_=C.byref(wide_pi), q_=C.byref(wide_q)) == nat.EUNSUPPORTED
    assert target(pi_=C.byref(wide_pi), q_=C.byref(wide_q)) == nat.EUNSUPPORTED
    assert grad(B=65537) == nat.EUNSUPPORTED
    other = nat.Mlp.from_buffer_copy(fpi.m); other.h1 = 399
    before = [p.detach().clone() for p in pi.parameters()]
    assert lib.pds_polyak_broad(Pm, C.byref(other), 0.995, s) == nat.EINVAL
    assert lib.pds_polyak_broad(Pm, None, 0.995, s) == nat.EINVAL and lib.pds_polyak_broad(Pm, Pm, 1.5, s) == nat.EINVAL
    torch.cuda.synchronize()
    assert torch.all(grads == 7.0) and torch.all(stats == 7.0) and torch.all(out == 7.0)
    assert all(torch.equal(a, b) for a, b in zip(before, pi.parameters()))
    # ... and through the one checked call path: a broad network is kept away from the entry points of include/pds.h
    with pytest.raises(NotImplementedError, match="pds_mlp_broad.h"):
        nat.call("pds_polyak", fpi, fpi, 0.5, on=oa)
    with pytest.raises(NotImplementedError, match="above 64"):
        nat.call("pds_polyak_broad", f64pi, f64pi, 0.5, on=oa)
