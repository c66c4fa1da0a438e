"""The host side of the kernels for two-hidden-layer networks with a hidden width above 64 (no GPU): the rows of
native.MLP_BROAD_SIGNATURES against their declarations in include/pds_mlp_broad.h (include/pds.h and native.SIGNATURES are pinned
entry for entry by tests/test_host_cpu.py, so the entry points stand beside them), the library's exports, the parameter count and
flat layout against torch, every refusal the header names (all raised before any device call), ddpg.fused_supported with and
without its keyword, the translation units in build._UNITS and the case table of tests/ddpg_broad_cases.py."""
import ctypes as C
import os
import re

import pytest
import torch

NAMES = ["pds_mlp_broad_supported", "pds_mlp_broad_param_count", "pds_mlp_broad_workspace_floats", "pds_mlp_broad_forward",
         "pds_mlp_broad_value_grad_step", "pds_mlp_broad_adam_step", "pds_ddpg_broad_supported", "pds_ddpg_broad_workspace_floats",
         "pds_ddpg_broad_policy_grad", "pds_ddpg_broad_target", "pds_polyak_broad"]
P = 4096  # stands for a device pointer: every call below is refused before anything reads it


def test_the_table_matches_the_header_and_the_library_exports_the_symbols(monkeypatch):
    """by the comparison of tests/test_host_cpu.py (its _table_mismatches, reading this header); a row that lost an argument must
    not pass; include/pds.h and native.SIGNATURES still agree without the symbols and name none of them; every row is the row of
    the include/pds.h entry point of the same name"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.MLP_BROAD_SIGNATURES
    assert list(table) == NAMES and not set(table) & set(native.SIGNATURES)
    n, bad = th._table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) and not bad, bad
    assert not any(name in th._header() for name in NAMES)  # include/pds.h does not declare the new names

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_mlp_broad.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == len(NAMES) and not bad, bad
    twins = {"pds_mlp_broad_param_count": "pds_mlp_param_count", "pds_mlp_broad_workspace_floats": "pds_mlp_workspace_floats",
             "pds_mlp_broad_forward": "pds_mlp_forward", "pds_mlp_broad_value_grad_step": "pds_value_grad_step",
             "pds_mlp_broad_adam_step": "pds_adam_step", "pds_ddpg_broad_supported": "pds_ddpg_supported",
             "pds_ddpg_broad_workspace_floats": "pds_ddpg_workspace_floats", "pds_ddpg_broad_policy_grad": "pds_ddpg_policy_grad",
             "pds_ddpg_broad_target": "pds_ddpg_target", "pds_polyak_broad": "pds_polyak"}
    for name, twin in twins.items():
        assert table[name] == native.SIGNATURES[twin], name
    restype, argtypes = table["pds_ddpg_broad_policy_grad"]
    _, bad = th._table_mismatches(dict(table, pds_ddpg_broad_policy_grad=(restype, argtypes[:-1])), native)
    assert bad == ["pds_ddpg_broad_policy_grad: 10 argtypes for 11 parameters"]
    _, bad = th._table_mismatches({k: table[k] for k in NAMES[1:]}, native)
    assert len(bad) == 1 and bad[0].startswith("names")
    lib = native.load()
    for name in NAMES:
        assert hasattr(lib, name), f"libpds_hip.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.argtypes == table[name][1] and fn.restype is table[name][0]
    text = header()
    assert int(re.search(r"#define\s+PDS_MLP_BROAD_MAX_HIDDEN\s+(\d+)", text).group(1)) == native.MLP_BROAD_MAX_HIDDEN == 512
    assert int(re.search(r"#define\s+PDS_MLP_BROAD_MAX_BATCH\s+(\d+)", text).group(1)) == native.MLP_BROAD_MAX_BATCH == 65536


def test_the_translation_units_and_their_headers_are_in_the_build():
    from phoenix_drone_simulation_amd import build
    for unit in ("pds_mlp_broad.hip", "pds_ddpg_broad.hip"):
        assert unit in build._UNITS and os.path.exists(os.path.join(build._CSRC, unit))
    assert len(build._UNITS) == len(set(build._UNITS)) and "pds_mlp_broad_tile.h" in build._HEADERS
    assert any(os.path.normpath(d).endswith(os.path.join("include", "pds_mlp_broad.h")) for d in build._DEPS)
    with open(os.path.join(build._CSRC, "pds_mlp_broad_tile.h")) as f:
        text = f.read()
    import ddpg_broad_cases as bc
    pair_from = int(re.search(r"kBroadPairFrom = (\d+);", text).group(1))
    split_rows = int(re.search(r"kBroadSplitRows = (\d+);", text).group(1))
    # the case table crosses both thresholds: the two-tile chain block and a weight-gradient sum of more than one part
    assert min(bc.BATCHES) < pair_from <= max(bc.BATCHES) and min(bc.BATCHES) <= split_rows < max(bc.BATCHES)
    for unit in ("pds_mlp_broad.hip", "pds_ddpg_broad.hip", "pds_mlp_broad_tile.h"):
        with open(os.path.join(build._CSRC, unit)) as f:
            src = f.read()
        assert "atomicAdd" not in src and "PDS_MFMA_BF" not in src  # fixed-order sums only; exact f32 MFMA, no split form


def _m(d_in, h1, h2, d_out, act="relu", base=P):
    from phoenix_drone_simulation_amd import native
    return native.mlp(d_in, h1, h2, d_out, act, base=base)


@pytest.mark.parametrize("d_in,h1,h2,d_out", [(42, 400, 300, 4), (46, 400, 300, 1), (1, 65, 1, 1), (64, 512, 512, 8), (38, 64, 65, 4),
                                              (34, 300, 400, 4)])
def test_param_count_and_flat_layout_are_the_torch_sequentials(d_in, h1, h2, d_out):
    from phoenix_drone_simulation_amd import native
    from phoenix_drone_simulation_amd.ppo import _mlp
    lib = native.load()
    net = _mlp([d_in, h1, h2, d_out], "relu")
    m = _m(d_in, h1, h2, d_out)
    total = sum(p.numel() for p in net.parameters())
    assert total == torch.nn.utils.parameters_to_vector(net.parameters()).numel()
    assert lib.pds_mlp_broad_param_count(C.byref(m)) == total and lib.pds_mlp_broad_supported(C.byref(m)) == 1
    assert lib.pds_mlp_param_count(C.byref(m)) < 0  # (include/pds.h refuses the shape, as before)
    # workspace: the six [B][.] slabs of 65536 samples, a statistics row per 16 samples, 16 parts of the gradient
    assert lib.pds_mlp_broad_workspace_floats(C.byref(m)) == 65536 * (d_in + 2 * (h1 + h2) + d_out) + 4 * 4096 + 16 * total
    off = P  # the pointers mlp(base=...) lays out are the running sums of parameters_to_vector's order
    for name, p in zip(("w1", "b1", "w2", "b2", "w3", "b3"), net.parameters()):
        assert getattr(m, name) == off
        off += 4 * p.numel()


def test_fused_mlp_flat_layout_is_parameters_to_vector_order():
    """FusedMLP(..., broad=True) needs device parameters; the layout it relies on is checked here on what it is built from: .grad
    views into one flat buffer in parameters_to_vector order (the constructor's loop), stated over the same parameter list"""
    from phoenix_drone_simulation_amd.ppo import _mlp
    net = _mlp([42, 400, 300, 4], "relu")
    lin = [l for l in net if isinstance(l, torch.nn.Linear)]
    params = [p for l in lin for p in (l.weight, l.bias)]
    assert all(a is b for a, b in zip(params, net.parameters())) and len(params) == 6
    vec = torch.nn.utils.parameters_to_vector(params)
    off = 0
    for p in params:
        assert torch.equal(vec[off:off + p.numel()].view_as(p), p)
        off += p.numel()
    assert off == vec.numel() == 42 * 400 + 400 + 400 * 300 + 300 + 300 * 4 + 4


def test_fused_mlp_refuses_a_cpu_network_with_and_without_the_keyword():
    from phoenix_drone_simulation_amd.fused import FusedMLP
    from phoenix_drone_simulation_amd.ppo import _mlp
    import inspect
    assert inspect.signature(FusedMLP.__init__).parameters["broad"].default is False
    for kw in ({}, {"broad": True}):
        with pytest.raises(ValueError, match="contiguous float32 parameters on the HIP device"):
            FusedMLP(_mlp([42, 400, 300, 4], "relu"), "relu", **kw)


def test_fused_supported_with_and_without_the_keyword():
    from phoenix_drone_simulation_amd import ddpg
    big = (400, 300)
    assert ddpg.fused_supported(42, big, big) is False and ddpg.fused_supported(42, big, big, broad=True) is True
    assert ddpg.fused_supported(42, (64, 64), (64, 64)) is True
    for pi, q in (((513, 64), big), (big, (513, 64)), ((64, 64), (64, 64)), ((64, 64), big), (big, (64, 64)), ((400,), big),
                  ((400, 300, 200), big), ((0, 400), big)):
        assert ddpg.fused_supported(42, pi, q, broad=True) is False, (pi, q)
    assert ddpg.fused_supported(60, big, big, broad=True) is True and ddpg.fused_supported(61, big, big, broad=True) is False
    assert ddpg.fused_supported(42, (65, 64), (64, 65), "tanh", "relu", broad=True) is True
    assert ddpg.fused_supported(42, (512, 512), (512, 512), broad=True) is True
    assert ddpg.fused_supported(42, big, big, "elu", "relu", broad=True) is False
    assert ddpg.BROAD_MAX_HIDDEN == 512 and ddpg.FUSED_MAX_HIDDEN == 64
    # ... and the library's answer to the same questions
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    for D, pi, q in ((42, big, big), (42, (513, 64), big), (42, (64, 64), (64, 64)), (60, big, big), (61, big, big), (42, (65, 64), (64, 65)),
                     (42, (64, 64), big)):
        mp, mq = _m(D, pi[0], pi[1], 4), _m(D + 4, q[0], q[1], 1)
        assert (lib.pds_ddpg_broad_supported(C.byref(mp), C.byref(mq)) == 1) == ddpg.fused_supported(D, pi, q, broad=True), (D, pi, q)


def test_every_refusal_comes_before_any_device_call():
    """The pointers are made up and no test here has a device: a call that got as far as a launch would not return these codes."""
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    EINVAL, EUNSUPPORTED = native.EINVAL, native.EUNSUPPORTED
    pi, q = _m(42, 400, 300, 4), _m(46, 400, 300, 1)
    R = lambda m: C.byref(m) if m is not None else None

    def fwd(m=pi, x=P, B=16, mean=None, std=None, y=P):
        return lib.pds_mlp_broad_forward(R(m), x, None, B, mean, std, 1e-5, y, None)

    def mse(m=q, x=P, target=P, B=16, grads=P, stats=P, ws=P, opt=None):
        return lib.pds_mlp_broad_value_grad_step(R(m), x, None, target, B, grads, stats, ws, opt, None)

    def grad(pi_=pi, q_=q, oa=P, B=16, grads=P, stats=P, ws=P, opt=None):
        return lib.pds_ddpg_broad_policy_grad(R(pi_), R(q_), oa, None, B, 1.0, grads, stats, ws, opt, None)

    def target(pi_=pi, q_=q, o=P, B=16, rew=P, done=P, t=P):
        return lib.pds_ddpg_broad_target(R(pi_), R(q_), o, None, B, rew, done, 0.99, 1.0, t, None)

    assert lib.pds_mlp_broad_supported(R(pi)) == 1 and lib.pds_ddpg_broad_supported(R(pi), R(q)) == 1
    for kw in (dict(m=None), dict(x=None), dict(y=None), dict(B=0), dict(B=-3), dict(mean=P), dict(std=P)):
        assert fwd(**kw) == EINVAL, kw
    for kw in (dict(m=None), dict(x=None), dict(target=None), dict(B=0), dict(grads=None), dict(stats=None), dict(ws=None), dict(m=pi)):
        assert mse(**kw) == EINVAL, kw  # (m=pi: d_out != 1)
    for kw in (dict(pi_=None), dict(q_=None), dict(oa=None), dict(B=0), dict(grads=None), dict(stats=None), dict(ws=None)):
        assert grad(**kw) == EINVAL, kw
    for kw in (dict(pi_=None), dict(q_=None), dict(o=None), dict(B=0), dict(rew=None), dict(done=None), dict(t=None)):
        assert target(**kw) == EINVAL, kw
    # widths and activation outside the range; a NULL tensor
    outside = [_m(42, 513, 64, 4), _m(42, 64, 513, 4), _m(42, 0, 400, 4), _m(42, 400, 0, 4), _m(42, 400, 300, 9), _m(42, 400, 300, 0),
               _m(0, 400, 300, 4), _m(193, 400, 300, 4)]
    act2 = _m(42, 400, 300, 4); act2.activation = 2
    null = _m(42, 400, 300, 4); null.w2 = None
    for m in outside + [act2, null]:
        assert fwd(m=m) == EINVAL and lib.pds_mlp_broad_param_count(R(m)) < 0 and lib.pds_mlp_broad_supported(R(m)) == 0
        assert lib.pds_mlp_broad_workspace_floats(R(m)) < 0 and grad(pi_=m) == EINVAL and target(pi_=m) == EINVAL
        assert lib.pds_polyak_broad(R(m), R(m), 0.5, None) == EINVAL
    # both widths at most 64: the network of include/pds.h, and the text says so
    small_pi, small_q = _m(42, 64, 64, 4), _m(46, 64, 64, 1)
    assert grad(pi_=small_pi, q_=small_q) == EINVAL and target(pi_=small_pi, q_=small_q) == EINVAL
    text = lib.pds_last_error(None)
    for name in (b"pds_ddpg_policy_grad", b"pds_ddpg_target", b"pds_polyak", b"pds_mlp_forward", b"pds_value_grad_step", b"pds.h"):
        assert name in text, text
    assert fwd(m=small_pi) == EINVAL and mse(m=small_q) == EINVAL and lib.pds_polyak_broad(R(small_pi), R(small_pi), 0.5, None) == EINVAL
    assert lib.pds_ddpg_broad_supported(R(small_pi), R(small_q)) == 0 and lib.pds_ddpg_supported(R(small_pi), R(small_q)) == 1
    assert lib.pds_ddpg_broad_supported(R(pi), R(small_q)) == 0 and lib.pds_ddpg_broad_supported(R(small_pi), R(q)) == 0
    # the pair: an actor with d_out != 4, a Q with d_out != 1 or d_in != D + 4
    for kw in (dict(pi_=_m(42, 400, 300, 3)), dict(q_=_m(46, 400, 300, 2)), dict(q_=_m(45, 400, 300, 1))):
        assert grad(**kw) == EINVAL and target(**kw) == EINVAL, kw
        assert lib.pds_ddpg_broad_supported(R(kw.get("pi_", pi)), R(kw.get("q_", q))) == 0
        assert lib.pds_ddpg_broad_workspace_floats(R(kw.get("pi_", pi)), R(kw.get("q_", q))) == EINVAL
    # D + 4 = 65: valid networks the kernels do not cover -- behind every PDS_EINVAL
    wpi, wq = _m(61, 400, 300, 4), _m(65, 400, 300, 1)
    assert grad(pi_=wpi, q_=wq) == EUNSUPPORTED and target(pi_=wpi, q_=wq) == EUNSUPPORTED
    assert lib.pds_ddpg_broad_supported(R(wpi), R(wq)) == 0 and lib.pds_ddpg_broad_workspace_floats(R(wpi), R(wq)) == EUNSUPPORTED
    assert grad(pi_=wpi, q_=wq, B=0) == EINVAL and target(pi_=wpi, q_=wq, t=None) == EINVAL
    assert fwd(m=wq) == EUNSUPPORTED and mse(m=wq) == EUNSUPPORTED and lib.pds_mlp_broad_supported(R(wq)) == 0
    assert lib.pds_mlp_broad_param_count(R(wq)) > 0 and lib.pds_mlp_broad_workspace_floats(R(wq)) == EUNSUPPORTED
    # more samples than the workspace holds: behind every PDS_EINVAL too (the forward and the target have no such limit)
    assert mse(B=65537) == EUNSUPPORTED and grad(B=65537) == EUNSUPPORTED and mse(B=65537, ws=None) == EINVAL
    # a bad opt: no moments, or a step count below 1
    for opt in (native.Adam(None, P, 1, 3e-4, 0.9, 0.999, 1e-8), native.Adam(P, None, 1, 3e-4, 0.9, 0.999, 1e-8),
                native.Adam(P, P, 0, 3e-4, 0.9, 0.999, 1e-8)):
        assert mse(opt=C.byref(opt)) == EINVAL and grad(opt=C.byref(opt)) == EINVAL
    adam = lambda m=pi, g=P, em=P, ev=P, step=1: lib.pds_mlp_broad_adam_step(R(m), g, em, ev, step, 3e-4, 0.9, 0.999, 1e-8, None)
    for kw in (dict(m=None), dict(g=None), dict(em=None), dict(ev=None), dict(step=0), dict(m=small_pi)):
        assert adam(**kw) == EINVAL, kw
    # polyak: outside [0, 1], NULL, shapes that differ
    assert lib.pds_polyak_broad(R(pi), R(pi), 1.5, None) == EINVAL and lib.pds_polyak_broad(R(pi), R(pi), -0.1, None) == EINVAL
    assert lib.pds_polyak_broad(R(pi), None, 0.5, None) == EINVAL and lib.pds_polyak_broad(None, R(pi), 0.5, None) == EINVAL
    assert lib.pds_polyak_broad(R(pi), R(_m(42, 400, 299, 4)), 0.5, None) == EINVAL
    assert lib.pds_polyak_broad(R(pi), R(pi), float("nan"), None) == EINVAL


def test_the_case_table_holds_what_the_issue_names():
    import ddpg_broad_cases as bc
    ids = [bc.case_id(c) for c in bc.CASES]
    assert len(set(ids)) == len(ids) == len(bc.SHAPES) * len(bc.BATCHES)
    hidden = {(s.pi, s.q) for s in bc.SHAPES}
    for pair in (((400, 300), (400, 300)), ((65, 64), (65, 64)), ((64, 65), (64, 65)), ((512, 512), (512, 512)), ((300, 400), (300, 400))):
        assert pair in hidden
    assert any(s.pi != s.q for s in bc.SHAPES)
    assert {(s.pact, s.qact) for s in bc.SHAPES} >= {("relu", "relu"), ("tanh", "tanh"), ("relu", "tanh")}
    assert {c.D for c in bc.CASES} == {34, 60} and {c.B for c in bc.CASES} == {1, 17, 128, 1000}
    assert {c.index for c in bc.CASES} == {None, "rep", "perm"}
    for s in bc.SHAPES:
        mine = [c for c in bc.CASES if c.shape is s]
        assert {c.B for c in mine} == set(bc.BATCHES) and {c.D for c in mine} == {34, 60} and None in {c.index for c in mine} and "rep" in {c.index for c in mine}
    assert bc.BAR_UNITS == 4.0 and bc.FLOOR == 2e-6
