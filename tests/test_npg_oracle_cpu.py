"""The references and bars of tests/npg_cases.py checked without a device: the two float64 statements of the Fisher-vector
product agree, float32 torch arithmetic on the CPU meets every bar (they are attainable), deliberately wrong float32
restatements miss them (they bite), the one-launch CG reference chains into the solve-level references, and the case table
reaches every kernel instantiation of csrc/pds_npg.hip."""
import functools
import math

import numpy as np
import pytest
import torch

import npg_cases as nc

F32, F64 = torch.float32, torch.float64
TINY_FVP = [c for c in nc.FVP_CASES if c.B <= nc.DENSE_MAX]
TINY_LS = [c for c in nc.LS_CASES if c.B <= nc.DENSE_MAX]


def _one_tail_per_nin(cases):
    seen, out = set(), []
    for c in cases:
        if c.B == nc.TAIL and nc.nin_of(c.d_in) not in seen:
            seen.add(nc.nin_of(c.d_in))
            out.append(c)
    return out


TAIL_FVP, TAIL_LS = _one_tail_per_nin(nc.FVP_CASES), _one_tail_per_nin(nc.LS_CASES)


@functools.lru_cache(maxsize=None)
def _inputs(c):
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    return nc.make_inputs(c, "cpu")


@functools.lru_cache(maxsize=None)
def _want(c):
    i = _inputs(c)
    return nc.ref_fvp(i["net"], i["xs"], i["log_std"], i["v"])


@functools.lru_cache(maxsize=None)
def _dense(c):
    i = _inputs(c)
    return nc.ref_fvp_dense(i["net"], i["xs"], i["log_std"], i["v"], nc.cancel_depth(c))


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_table_counts_are_literal():
    assert len(nc.FVP_CASES) == nc.N_FVP_CASES == 36
    assert len(nc.LS_CASES) == nc.N_LS_CASES == 16
    assert len({nc.case_id(c) for c in nc.CASES}) == len(nc.CASES)


def test_table_covers_the_shape_axes():
    fvp, ls = nc.FVP_CASES, nc.LS_CASES
    assert {1, 16, 17, 32, 33, 47, 64, 65, 128, 129, 191, 192} <= {c.d_in for c in fvp}
    hidden = {1, 16, 17, 33, 48, 49, 50, 63, 64}
    for cases in (fvp, ls):
        assert {c.d_out for c in cases} == set(range(1, 9))
        reach = {(nc.nin_of(c.d_in), c.act) for c in cases}
        assert reach == {(n, a) for n in nc.NINS for a in ("relu", "tanh")}, reach
        for c in cases:  # every shape at a tiny and at a tail batch
            if c.B != nc.BIG:
                assert {k.B for k in cases if k[1:6] == c[1:6]} >= {nc.TAIL} and c.B in nc.TINY + (nc.TAIL,)
    for n in nc.NINS:
        order = {(c.h1 < c.h2) for c in fvp if nc.nin_of(c.d_in) == n and c.h1 != c.h2}
        assert order == {True, False}, n
        assert all(c.h1 in hidden and c.h2 in hidden for c in fvp if c.h1 != c.h2)
    assert {c.h1 < c.h2 for c in ls if c.h1 != c.h2} == {True, False}
    for d in (34, 42, 40, 48):  # the trainer's shapes stay
        assert any(c[1:5] == (d, 50, 50, 4) for c in fvp)
    assert any((c.h1, c.h2) == (64, 64) for c in fvp)
    assert sum(c.B == nc.BIG for c in fvp) == 2
    assert {c.index for c in fvp} == {None, "perm", "rep"}
    assert {c.index for c in fvp if c.B == nc.TAIL} == {None, "perm", "rep"}
    assert nc.TAIL == 2 * 16384 + 53 and nc.TAIL % 16 != 0
    assert {c.B for c in fvp if c.B <= nc.DENSE_MAX} == set(nc.TINY)


def test_nin_mirror_matches_the_launchers():
    src = nc.source_thresholds()
    for name in ("launch_fvp", "launch_surrogate"):
        pairs, last = src[name]
        assert pairs == [(2, 2), (4, 4), (8, 8)] and last == [12], (name, pairs, last)
    assert tuple(t for t, _ in src["launch_fvp"][0]) == nc.NIN_THRESHOLDS
    with open(nc.NPG_SOURCE) as f:
        text = f.read()
    assert text.count("nin = (m->d_in + kTW - 1) / kTW") == 2  # both entry points form nin the same way
    for d_in, want in ((1, 2), (32, 2), (33, 4), (64, 4), (65, 8), (128, 8), (129, 12), (192, 12)):
        assert nc.nin_of(d_in) == want


# ---- the two float64 statements of F v -------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TINY_FVP, ids=nc.case_id)
def test_double_backward_equals_the_gauss_newton_form(c):
    """zero gradient of the KL at theta_old: the double backward IS J^T D J v / (B A), relu and tanh, h1 != h2"""
    want, (dense, cancel) = _want(c), _dense(c)
    assert float(torch.norm(want - dense)) <= 1e-12 * float(torch.norm(dense))
    assert bool((cancel >= 0).all()) and cancel.shape == want.shape


# ---- float32 torch arithmetic meets the bars --------------------------------------------------------------------------
def _check_fvp(c, got, want, cancel):
    whole, per = nc.fvp_bars(c, want, cancel)
    worst = float(torch.norm(got.double() - want)) / whole
    for name, sl in nc.slices(c).items():
        worst = max(worst, float(torch.norm(got[sl].double() - want[sl])) / per[name])
    return worst


@pytest.mark.parametrize("c", TINY_FVP + TAIL_FVP, ids=nc.case_id)
def test_float32_autograd_meets_the_fvp_bars(c):
    i = _inputs(c)
    # the kink cap at its strictest: no sample near a kink is left in any batch; the tiny batches needed no redraw for
    # their seeds, the larger ones redrew about 0.1 % of their rows
    assert i["kink_redraws"] <= (0 if c.B <= nc.DENSE_MAX else c.B // 500)
    assert c.act != "relu" or not bool(nc.near_kink(i["net"], i["xs"]).any())
    got = nc.fvp_autograd(i["net"], i["xs"], i["log_std"], i["v"], F32)
    cancel = _dense(c)[1] if c.B <= nc.DENSE_MAX else None
    worst = _check_fvp(c, got, _want(c), cancel)
    assert worst < 1.0, worst


def test_cancellation_allowance_is_the_rank_one_case_only():
    assert [nc.case_id(c) for c in nc.FVP_CASES if nc.cancel_applies(c)] == ["fvp-1x16x17x1-relu-B1"]
    for c in nc.FVP_CASES:
        if c.B >= 4096:  # exactly zero, so below the 2e-5 term
            want = torch.ones(nc.param_count(c), dtype=F64)
            whole, _ = nc.fvp_bars(c, want, torch.ones_like(want))
            assert whole == nc.FVP_REL * float(torch.norm(want))
    c = nc.FVP_CASES[0]
    want, (_, cancel) = _want(c), _dense(c)
    whole, _ = nc.fvp_bars(c, want, cancel)
    assert whole > nc.FVP_REL * float(torch.norm(want))
    # no looser than the allowance it generalises (parameter count in place of the depth, max 1 / sigma^2)
    i = _inputs(c)
    j = nc.jacobian64(i["net"], i["xs"])[0]
    old = nc.param_count(c) * nc.EPS32 * float((j * i["v"].double()).abs().sum()) * float(torch.norm(j)) * \
        float(torch.exp(-2 * i["log_std"].double()).max())
    assert float(torch.norm(cancel)) <= old


def test_tensor_bars_stay_inside_their_range():
    for name in nc.TENSORS:
        for c in nc.FVP_CASES:
            assert nc.TENSOR_FLOOR <= nc.fvp_tensor_rel(name, c) <= nc.FVP_REL


# ---- a float32 restatement of the kernel's arithmetic, and wrong versions of it ---------------------------------------
def _manual_fvp(c, i, wrong=None, dtype=F32):
    """tangent forward, scale, backward: the Gauss-Newton product as fvp_kernel forms it, in torch `dtype`"""
    lin = [m for m in i["net"] if isinstance(m, torch.nn.Linear)]
    W1, b1, W2, b2, W3, b3 = (t.detach().to(dtype) for l in lin for t in (l.weight, l.bias))
    sl, v = nc.slices(c), i["v"].to(dtype)
    V1, vb1, V2, vb2, V3, vb3 = (v[sl[n]] for n in nc.TENSORS)
    V1, V2, V3 = V1.view(c.h1, c.d_in), V2.view(c.h2, c.h1), V3.view(c.d_out, c.h2)
    if wrong == "v2_swapped":  # gemm_glb(V2, m.h1, m.h2, ...): the flat tensor read as [h1][h2], zero outside
        M = torch.zeros(64, 64, dtype=dtype)
        M[:c.h1, :c.h2] = v[sl["W2"]].view(c.h1, c.h2)
        V2 = M[:c.h2, :c.h1]
    x = i["xs"].to(dtype)
    B = x.shape[0]
    if wrong == "skip_one":
        x = x[:-1]
    fn = torch.relu if c.act == "relu" else torch.tanh
    dfn = (lambda h: (h > 0).to(dtype)) if c.act == "relu" else (lambda h: 1 - h * h)
    h1 = fn(x @ W1.t() + b1)
    t1 = dfn(h1) * (x @ V1.t() + vb1)
    h2 = fn(h1 @ W2.t() + b2)
    dz2 = h1 @ V2.t() + t1 @ W2.t()
    t2 = dfn(h2) * (dz2 if wrong == "no_vb2" else dz2 + vb2)
    dmu = h2 @ V3.t() + t2 @ W3.t() + vb3
    isg2 = torch.exp(-i["log_std"].to(dtype)) ** 2
    u = dmu * (isg2[0] if wrong == "isg2_0" else isg2)
    dW3, db3 = u.t() @ h2, u.sum(0)
    dZ2 = (u @ W3) * dfn(h2)
    dW2, db2 = dZ2.t() @ h1, dZ2.sum(0)
    dZ1 = (dZ2 @ W2) * dfn(h1)
    dW1, db1 = dZ1.t() @ x, dZ1.sum(0)
    flat = torch.cat([t.reshape(-1) for t in (dW1, db1, dW2, db2, dW3, db3)])
    return flat / (B * c.d_out)


_MUT_CASES = [c for c in TINY_FVP + TAIL_FVP if c.h1 != c.h2 and c.d_out > 1][:3] + \
    [c for c in TAIL_FVP if c.h1 != c.h2 and c.d_out > 1][:1]


@pytest.mark.parametrize("c", _MUT_CASES, ids=nc.case_id)
def test_wrong_float32_fisher_products_miss_the_bars(c):
    i, want = _inputs(c), _want(c)
    cancel = _dense(c)[1] if c.B <= nc.DENSE_MAX else None
    assert _check_fvp(c, _manual_fvp(c, i), want, cancel) < 1.0  # the restatement itself is inside
    for wrong in ("v2_swapped", "no_vb2", "isg2_0") + (("skip_one",) if c.B == nc.TAIL else ()):
        worst = _check_fvp(c, _manual_fvp(c, i, wrong), want, cancel)
        assert worst > 1.0, (wrong, worst)


def _ls32(c, i, f, sigma0=False, dtype=F32):
    """a candidate in float32 torch arithmetic -> (ra, kl, rs, theta)"""
    import copy
    theta = i["theta"] + torch.tensor(f, dtype=F32) * i["s"]
    n = copy.deepcopy(i["net"]).to(dtype)
    off = 0
    with torch.no_grad():
        for p in n.parameters():
            p.copy_(theta[off:off + p.numel()].view_as(p))
            off += p.numel()
        mu = n(i["x"].to(dtype))
        ls = i["log_std"].to(dtype)
        if sigma0:
            ls = ls[:1].expand_as(ls)
        std = torch.exp(ls)
        lp = torch.distributions.Normal(mu, std).log_prob(i["act"].to(dtype)).sum(-1)
        ratio = torch.exp(lp - i["logp_old"].to(dtype))
        kl = torch.distributions.kl.kl_divergence(torch.distributions.Normal(i["mu_old"].to(dtype), std),
                                                  torch.distributions.Normal(mu, std)).sum()
    return float((ratio * i["adv"].to(dtype)).sum()), float(kl), float(ratio.sum()), theta


def _ls_worst(c, i, f, sigma0=False):
    ra, kl, rs, theta = _ls32(c, i, f, sigma0)
    ref = nc.ref_ls(i["net"], theta, i["x"], i["act"], i["adv"], i["logp_old"], i["mu_old"], i["log_std"])
    bars = nc.ls_bars(ref, c.B, c.d_out)
    return [abs(ra - ref["ra"]) / bars[0], abs(kl - ref["kl"]) / bars[1], abs(rs - ref["rs"]) / bars[2]]


@pytest.mark.parametrize("c", TINY_LS + TAIL_LS, ids=nc.case_id)
def test_float32_line_search_meets_the_bars(c):
    i = _inputs(c)
    for f in nc.LS_FRACS[:-1]:
        assert max(_ls_worst(c, i, f)) < 1.0, f


@pytest.mark.parametrize("c", [c for c in TINY_LS + TAIL_LS if c.d_out > 1][:4], ids=nc.case_id)
def test_line_search_with_one_sigma_for_all_outputs_misses_the_bars(c):
    i = _inputs(c)
    w = _ls_worst(c, i, 0.8, sigma0=True)
    assert w[1] > 1.0 and (w[0] > 1.0 or w[2] > 1.0), w  # the KL, and the log-probability through a ratio sum


# ---- conjugate gradients ---------------------------------------------------------------------------------------------
def _cg64(avp, b, nsteps, residual_tol=1e-10, eps=1e-6):
    """the reference of tests/test_gpu_npg_kernels.py"""
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


def _chain(d, b, launches, tol=1e-10, eps=1e-6):
    x = r = p = np.zeros_like(b, dtype=np.float64)
    s = nc.ref_cg_step(x, r, p, b, np.zeros(2), eps, tol, True)
    hist = []
    for _ in range(launches):
        s = nc.ref_cg_step(s["x"], s["r"], s["p"], d * s["p"], s["st"], eps, tol, False)
        hist.append(s)
    return s, hist


@pytest.mark.parametrize("tol", [1e-10, 0.3])
def test_chained_cg_steps_reproduce_the_solve_level_references(tol):
    d, b = (t.astype(np.float64) for t in nc.cg_problem(5000))
    s, hist = _chain(d, b, 10, tol)
    D, Bt = torch.as_tensor(d), torch.as_tensor(b)
    want = _cg64(lambda p: D * p, Bt.clone(), 10, residual_tol=tol)
    assert np.abs(s["x"] - want.numpy()).max() <= 1e-13 * np.abs(want.numpy()).max()
    from phoenix_drone_simulation_amd.npg import conjugate_gradients
    ref = conjugate_gradients(lambda p: D * p, Bt.clone(), 10, residual_tol=tol)
    assert np.abs(s["x"] - ref.numpy()).max() <= 1e-13 * np.abs(ref.numpy()).max()
    stopped = [h["stopped_now"] for h in hist]
    assert (sum(stopped) == 1 and s["st"][1] == 1.0) if tol == 0.3 else not any(stopped)
    if tol == 0.3:  # after the break nothing moves
        k = stopped.index(True)
        for key in ("x", "r", "p", "st"):
            assert np.array_equal(hist[k][key], s[key])


def _dot32(a, b, skip_last=False):
    """cg_dot in numpy float32: thread-strided chains, the butterfly inside each wave, the sixteen waves in order"""
    m = a.size - 1 if skip_last else a.size
    prod = (a[:m] * b[:m]).astype(np.float32)
    rows = -(-max(m, 1) // 1024)
    prod = np.concatenate([prod, np.zeros(rows * 1024 - m, np.float32)]).reshape(rows, 1024)
    s = np.zeros(1024, np.float32)
    for row in prod:
        s = s + row
    s = s.reshape(16, 64)
    lanes = np.arange(64)
    for dd in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ dd]
    t = np.float32(0)
    for w in range(16):
        t = t + s[w, 0]
    return t


def _step32(x, r, p, z, st, eps, tol, skip_last=False):
    """cg_kernel's non-init launch in numpy float32"""
    f = np.float32
    alpha = f(st[0]) / (_dot32(p, z, skip_last) + f(eps))
    x = x + alpha * p
    r = r - alpha * z
    nr = _dot32(r, r, skip_last)
    if np.sqrt(nr) < f(tol):
        return x, r, p, np.array([st[0], 1.0], f)
    mu = nr / (f(st[0]) + f(eps))
    return x, r, (r + mu * p).astype(f), np.array([nr, 0.0], f)


def _cg_worst(ref, x, r, p, st):
    bars = nc.cg_step_bars(ref)
    w = [np.max(np.abs(x - ref["x"]) / bars["x"]), np.max(np.abs(r - ref["r"]) / bars["r"]),
         abs(float(st[0]) - ref["st"][0]) / bars["nr"]]
    if "p" in bars:
        w.append(np.max(np.abs(p - ref["p"]) / bars["p"]))
    return float(max(w))


@pytest.mark.parametrize("n", nc.CG_SIZES)
def test_float32_cg_step_is_inside_the_step_bars_and_a_skipped_element_is_not(n):
    d, b = nc.cg_problem(n)
    assert d.dtype == np.float32 and abs(b[-1]) >= 1.0
    x, r, p, st = np.zeros(n, np.float32), b.copy(), b.copy(), np.array([_dot32(b, b), 0.0], np.float32)
    assert abs(float(st[0]) - float(b.astype(np.float64) @ b.astype(np.float64))) <= nc.cg_dot_bar(b, b)
    assert abs(float(_dot32(b, b, True)) - float(b.astype(np.float64) @ b.astype(np.float64))) > nc.cg_dot_bar(b, b)
    for launch in range(6):
        z = (d * p).astype(np.float32)
        ref = nc.ref_cg_step(x, r, p, z, st, 1e-6, 1e-10, False)
        if launch == 0:
            bad = _step32(x, r, p, z, st, 1e-6, 1e-10, skip_last=True)
            assert _cg_worst(ref, *bad) > 1.0
        x, r, p, st = _step32(x, r, p, z, st, 1e-6, 1e-10)
        assert _cg_worst(ref, x, r, p, st) < 1.0, launch
