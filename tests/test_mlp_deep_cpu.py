"""The host side of the kernels for networks with three and four hidden layers (no GPU): the rows of native.MLP_DEEP_SIGNATURES
against their declarations in include/pds_mlp_deep.h (include/pds.h and native.SIGNATURES are pinned entry for entry by
tests/test_host_cpu.py, so the entry points stand beside them), the library's exports, pds_mlp_deep_param_count against torch,
every refusal the header names (all raised before any device call), the translation unit in build._UNITS, and the teeth of the
float64 reference that tests/test_gpu_mlp_deep.py compares the kernels with."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import mlp_cases as mc
import mlp_deep_cases as dc

NAMES = ["pds_mlp_deep_supported", "pds_mlp_deep_param_count", "pds_mlp_deep_workspace_floats", "pds_mlp_deep_forward",
         "pds_mlp_deep_ppo_policy_grad_step", "pds_mlp_deep_value_grad_step", "pds_mlp_deep_adam_step"]
P = 4096  # stands for a device pointer: every call below is refused before anything reads it


def test_the_table_matches_the_header_and_the_library_exports_the_symbols(monkeypatch):
    """by the comparison of tests/test_host_cpu.py (its _table_mismatches, reading this header: a struct pds_mlp_deep goes in as
    a plain pointer); a row that lost an argument, or holds a wrong class, must not pass; include/pds.h and native.SIGNATURES
    still agree without the symbols; the ctypes mirror of the struct field by field"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.MLP_DEEP_SIGNATURES
    assert list(table) == NAMES and not set(table) & set(native.SIGNATURES)
    n, bad = th._table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) and not bad, bad
    assert not any(name in th._header() for name in NAMES)  # include/pds.h does not declare the new names

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_mlp_deep.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == len(NAMES) and not bad, bad
    restype, argtypes = table["pds_mlp_deep_forward"]
    assert argtypes[1:] == native.SIGNATURES["pds_mlp_forward"][1][1:]  # pds_mlp_forward's, behind the struct
    assert table["pds_mlp_deep_ppo_policy_grad_step"][1][1:] == native.SIGNATURES["pds_ppo_policy_grad_step"][1][1:]
    assert table["pds_mlp_deep_value_grad_step"][1][1:] == native.SIGNATURES["pds_value_grad_step"][1][1:]
    assert table["pds_mlp_deep_adam_step"][1][1:] == native.SIGNATURES["pds_adam_step"][1][1:]
    _, bad = th._table_mismatches(dict(table, pds_mlp_deep_forward=(restype, argtypes[:-1])), native)
    assert bad == ["pds_mlp_deep_forward: 8 argtypes for 9 parameters"]
    wrong = list(argtypes); wrong[3] = C.c_int  # B is an int64_t
    _, bad = th._table_mismatches(dict(table, pds_mlp_deep_forward=(restype, wrong)), native)
    assert len(bad) == 1 and "argument 3" in bad[0]
    _, bad = th._table_mismatches({k: table[k] for k in NAMES[1:]}, native)
    assert len(bad) == 1 and bad[0].startswith("names")
    lib = native.load()
    for name in NAMES:
        assert hasattr(lib, name), f"libpds_hip.so does not export {name}"
        fn = getattr(lib, name)
        assert fn.argtypes == table[name][1] and fn.restype is table[name][0]
    # struct pds_mlp_deep against its ctypes mirror
    body = re.search(r"typedef\s+struct\s+pds_mlp_deep\s*\{(.*?)\}\s*pds_mlp_deep\s*;", header(), flags=re.S).group(1)
    assert int(re.search(r"#define\s+PDS_MLP_DEEP_MAX_HIDDEN\s+(\d+)", header()).group(1)) == native.MLP_DEEP_MAX_HIDDEN == 4
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        base, rest = re.match(r"((?:const\s+)?\w+)\s*(.*)", decl, flags=re.S).groups()
        for item in rest.split(","):
            name = re.sub(r"[\s\*]|\[.*\]", "", item)
            n_arr = {"PDS_MLP_DEEP_MAX_HIDDEN": 4, "PDS_MLP_DEEP_MAX_HIDDEN+1": 5}.get(re.sub(r"\s", "", (re.search(r"\[(.*)\]", item) or [None, ""])[1]))
            cls = C.c_void_p if "*" in item else {"int32_t": C.c_int32}[base]
            fields.append((name, cls * n_arr if n_arr else cls))
    assert [(n, c._type_ if hasattr(c, "_length_") else c, getattr(c, "_length_", 0)) for n, c in native.MlpDeep._fields_] == \
        [(n, c._type_ if hasattr(c, "_length_") else c, getattr(c, "_length_", 0)) for n, c in fields]


def test_the_translation_unit_and_its_headers_are_in_the_build():
    from phoenix_drone_simulation_amd import build
    assert "pds_mlp_deep.hip" in build._UNITS and os.path.exists(os.path.join(build._CSRC, "pds_mlp_deep.hip"))
    assert any(os.path.normpath(d).endswith(os.path.join("include", "pds_mlp_deep.h")) for d in build._DEPS)
    with open(os.path.join(build._CSRC, "pds_mlp_deep.hip")) as f:
        text = f.read()
    assert f"kDeepMaxBlocks = {dc.MAX_BLOCKS};" in text  # the grid cap behind mlp_deep_cases.grid_round
    assert "(L == 4 && LOSS != LOSS_NONE) ? 3 : kDeepMaxWaves" in text and "kDeepMaxWaves = 4;" in text


def _m(d_in, hidden, d_out, act="relu", base=P):
    from phoenix_drone_simulation_amd import native
    return native.mlp_deep(d_in, hidden, d_out, act, base=base)


@pytest.mark.parametrize("d_in,hidden,d_out", [(34, (50, 30, 20), 4), (34, (32, 32, 32, 32), 4), (1, (1, 1, 1), 1),
                                               (64, (64, 64, 64, 64), 8)])
def test_param_count_is_the_torch_sequentials(d_in, hidden, d_out):
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    net = dc.make_net(d_in, hidden, d_out, "tanh", 0, device="cpu")
    m = _m(d_in, hidden, d_out)
    total = sum(p.numel() for p in net.parameters())
    assert lib.pds_mlp_deep_param_count(C.byref(m)) == total
    assert lib.pds_mlp_deep_supported(C.byref(m)) == 1
    assert lib.pds_mlp_deep_workspace_floats(C.byref(m)) == dc.MAX_BLOCKS * 4 * (total + 4)  # one partial per wave of the grid
    # the flat layout is torch's order: the pointers mlp_deep(base=...) lays out are the running sums of the parameters' sizes
    off = P
    for l, lin in enumerate(l for l in net if isinstance(l, torch.nn.Linear)):
        assert m.w[l] == off
        off += 4 * lin.weight.numel()
        assert m.b[l] == off
        off += 4 * lin.bias.numel()


def test_param_count_is_negative_outside_the_range():
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    bad = [_m(34, (50,), 4), _m(34, (50, 30), 4), _m(34, (50, 0, 20), 4), _m(34, (50, 65, 20), 4), _m(34, (50, 30, 20), 0),
           _m(34, (50, 30, 20), 9), _m(0, (50, 30, 20), 4), _m(193, (50, 30, 20), 4), _m(34, (8, 8, 8, 65), 4)]
    five = _m(34, (8, 8, 8, 8), 4)
    five.n_hidden = 5
    act2 = _m(34, (50, 30, 20), 4)
    act2.activation = 2
    for m in bad + [five, act2]:
        assert lib.pds_mlp_deep_param_count(C.byref(m)) < 0
        assert lib.pds_mlp_deep_supported(C.byref(m)) == 0 and lib.pds_mlp_deep_workspace_floats(C.byref(m)) < 0
    assert lib.pds_mlp_deep_param_count(None) < 0 and lib.pds_mlp_deep_supported(None) == 0


def _forward(lib, m, B=16, x=P, y=P, mean=None, std=None):
    return lib.pds_mlp_deep_forward(C.byref(m) if m is not None else None, x, None, B, mean, std, 1e-5, y, None)


def _ppo(lib, m, B=16, opt=None, **null):
    a = dict(x=P, act=P, adv=P, logp=P, ls=P, grads=P, stats=P, ws=P)
    a.update(null)
    return lib.pds_mlp_deep_ppo_policy_grad_step(C.byref(m) if m is not None else None, a["x"], a["act"], a["adv"], a["logp"], a["ls"],
                                                 B, 0.2, a["grads"], a["stats"], a["ws"], opt, None)


def _mse(lib, m, B=16, opt=None, **null):
    a = dict(x=P, target=P, grads=P, stats=P, ws=P)
    a.update(null)
    return lib.pds_mlp_deep_value_grad_step(C.byref(m) if m is not None else None, a["x"], None, a["target"], B, a["grads"], a["stats"],
                                            a["ws"], opt, None)


def test_every_refusal_comes_before_any_device_call():
    """PDS_EINVAL for a NULL struct or tensor pointer among the first n_hidden + 1 layers, B < 1, a width or activation outside
    the range, n_hidden == 2 (with the text that names pds_mlp), d_out != 1 for the value gradient, a bad opt; PDS_EUNSUPPORTED
    behind those for d_in 65 and 192; a NULL w[4] / b[4] is nothing at n_hidden == 3.  The pointers are made up and no test
    here has a device: a call that got as far as a launch would not return these codes."""
    from phoenix_drone_simulation_amd import native
    lib = native.load()
    EINVAL, EUNSUPPORTED = native.EINVAL, native.EUNSUPPORTED
    good, critic = _m(34, (50, 30, 20), 4), _m(34, (64, 64, 64, 64), 1)
    assert good.w[4] is None and good.b[4] is None  # (mlp_deep leaves the unused layer's pointers NULL)
    assert lib.pds_mlp_deep_supported(C.byref(good)) == 1 and lib.pds_mlp_deep_param_count(C.byref(good)) == 3984
    assert _forward(lib, None) == EINVAL and _ppo(lib, None) == EINVAL and _mse(lib, None) == EINVAL
    for l in range(4):  # a NULL tensor among the first n_hidden + 1 layers
        for field in ("w", "b"):
            m = _m(34, (50, 30, 20), 4)
            getattr(m, field)[l] = None
            assert _forward(lib, m) == EINVAL and _ppo(lib, m) == EINVAL and lib.pds_mlp_deep_param_count(C.byref(m)) < 0
    m = _m(34, (64, 64, 64, 64), 1)
    m.b[4] = None
    assert _mse(lib, m) == EINVAL
    for B in (0, -5):
        assert _forward(lib, good, B=B) == EINVAL and _ppo(lib, good, B=B) == EINVAL and _mse(lib, critic, B=B) == EINVAL
    assert _forward(lib, good, x=None) == EINVAL and _forward(lib, good, y=None) == EINVAL
    assert _forward(lib, good, mean=P) == EINVAL and _forward(lib, good, std=P) == EINVAL  # mean and std come together
    for k in ("x", "act", "adv", "logp", "ls", "grads", "stats", "ws"):
        assert _ppo(lib, good, **{k: None}) == EINVAL
    for k in ("x", "target", "grads", "stats", "ws"):
        assert _mse(lib, critic, **{k: None}) == EINVAL
    assert _mse(lib, good) == EINVAL  # d_out != 1
    for m in (_m(34, (50, 65, 20), 4), _m(34, (50, 30, 0), 4), _m(34, (50, 30, 20), 9), _m(0, (50, 30, 20), 4), _m(193, (50, 30, 20), 4)):
        assert _forward(lib, m) == EINVAL and _ppo(lib, m) == EINVAL
    m = _m(34, (50, 30, 20), 4)
    m.activation = 2
    assert _forward(lib, m) == EINVAL
    two = _m(34, (50, 50), 4)
    assert _forward(lib, two) == EINVAL and _ppo(lib, two) == EINVAL
    assert b"pds_mlp" in lib.pds_last_error(None) and b"n_hidden == 2" in lib.pds_last_error(None)
    # a bad opt: no moments, or a step count below 1
    for opt in (native.Adam(None, P, 1, 3e-4, 0.9, 0.999, 1e-8), native.Adam(P, None, 1, 3e-4, 0.9, 0.999, 1e-8),
                native.Adam(P, P, 0, 3e-4, 0.9, 0.999, 1e-8)):
        assert _ppo(lib, good, opt=C.byref(opt)) == EINVAL and _mse(lib, critic, opt=C.byref(opt)) == EINVAL
    assert lib.pds_mlp_deep_adam_step(C.byref(good), P, None, P, 1, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL
    assert lib.pds_mlp_deep_adam_step(C.byref(good), P, P, P, 0, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL
    assert lib.pds_mlp_deep_adam_step(C.byref(good), None, P, P, 1, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL
    assert lib.pds_mlp_deep_adam_step(C.byref(two), P, P, P, 1, 3e-4, 0.9, 0.999, 1e-8, None) == EINVAL
    # 65 .. 192 inputs: a valid network the kernels do not cover -- behind every PDS_EINVAL
    for d_in in (65, 192):
        m, mc1 = _m(d_in, (50, 30, 20), 4), _m(d_in, (64, 64, 64), 1)
        assert lib.pds_mlp_deep_param_count(C.byref(m)) > 0 and lib.pds_mlp_deep_supported(C.byref(m)) == 0
        assert lib.pds_mlp_deep_workspace_floats(C.byref(m)) == EUNSUPPORTED
        assert _forward(lib, m) == EUNSUPPORTED and _ppo(lib, m) == EUNSUPPORTED and _mse(lib, mc1) == EUNSUPPORTED
        assert _forward(lib, m, B=0) == EINVAL and _ppo(lib, m, ws=None) == EINVAL and _mse(lib, m) == EINVAL


def test_the_case_table_holds_what_it_is_meant_to():
    assert dc.grid_round("fwd", 3) == dc.grid_round("ppo", 3) == dc.grid_round("fwd", 4) == 16384 and dc.grid_round("mse", 4) == 12288
    ids = [dc.case_id(c) for c in dc.CASES]
    assert len(set(ids)) == len(ids)
    for c in dc.CASES:
        assert len(c.hidden) in (3, 4) and c.d_in <= 64 and max(c.hidden) <= 64 and c.d_out <= 8
        assert c.B in dc.SMALL + (524288, 1 << 20) or c.B > 2 * dc.grid_round(c.kind, len(c.hidden)) and c.B % 16 != 0
    for kind in ("fwd", "ppo", "mse"):
        for depth in (3, 4):
            assert {c.act for c in dc.CASES if c.kind == kind and len(c.hidden) == depth} == {"relu", "tanh"}
    assert {c.index for c in dc.CASES if c.kind == "fwd"} == {None, "perm", "rep"} and {c.std for c in dc.CASES if c.kind == "fwd"} == {True, False}


# ---- teeth of the float64 reference ---------------------------------------------------------------------------------------
def _seq(sizes, weights, biases, last_act=True):
    layers = []
    for j, (w, b) in enumerate(zip(weights, biases)):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        hidden = j < len(weights) - 1
        layers += [lin, torch.nn.ReLU() if hidden and (last_act or j < len(weights) - 2) else torch.nn.Identity()]
    return torch.nn.Sequential(*layers)


def test_the_float64_reference_has_teeth():
    """on 34 -> 50, 30, 20 -> 4 in float64: dropping the activation behind the last hidden layer, swapping the widths of hidden
    layers 2 and 3 (W2's first 20 rows, W3 transposed, b3 and W4 widened by repeating their first entries) and using the bias
    of the wrong layer (b2 and b3 exchanged, cut or repeated to fit) each move the forward output and the PPO gradient by more
    than 100 times the two-hidden-layer bar.  The gradient is compared over the first layer, the part whose shape survives the
    swap."""
    torch.manual_seed(4)
    net = dc.make_net(34, (50, 30, 20), 4, "relu", 9, device="cpu").double()
    (W1, b1), (W2, b2), (W3, b3), (W4, b4) = [(l.weight.detach(), l.bias.detach()) for l in net if isinstance(l, torch.nn.Linear)]
    B = 512
    x = torch.randn(B, 34, dtype=torch.float64)
    log_std = torch.full((4,), math.log(0.3), dtype=torch.float64)
    with torch.no_grad():
        mu = net(x)
    act = mu + 0.3 * torch.randn(B, 4, dtype=torch.float64)
    logp_old = torch.distributions.Normal(mu, 0.3).log_prob(act).sum(-1) + 0.1 * torch.randn(B, dtype=torch.float64)
    adv = torch.randn(B, dtype=torch.float64)
    n1 = W1.numel() + b1.numel()
    y = dc.ref_forward(net, x)
    grad = dc.ref_ppo(net, x, act, adv, logp_old, log_std)[0][:n1]
    same = _seq(None, [W1, W2, W3, W4], [b1, b2, b3, b4])
    assert torch.equal(dc.ref_forward(same, x), y) and torch.equal(dc.ref_ppo(same, x, act, adv, logp_old, log_std)[0][:n1], grad)
    slips = {
        "no activation behind the last hidden layer": _seq(None, [W1, W2, W3, W4], [b1, b2, b3, b4], last_act=False),
        "widths of hidden layers 2 and 3 swapped": _seq(None, [W1, W2[:20], W3.T.contiguous(), torch.cat([W4, W4[:, :10]], 1)],
                                                        [b1, b2[:20], torch.cat([b3, b3[:10]]), b4]),
        "the bias of the wrong layer": _seq(None, [W1, W2, W3, W4], [b1, torch.cat([b3, b3[:10]]), b2[:20], b4]),
    }
    for name, slipped in slips.items():
        ys = dc.ref_forward(slipped, x)
        gs = dc.ref_ppo(slipped, x, act, adv, logp_old, log_std)[0][:n1]
        fwd = float(((ys - y).abs() / (2e-6 + 1e-5 * y.abs())).max())
        grd = float(((gs - grad).abs() / (mc.grad_atol(grad, B) + 2e-4 * grad.abs())).max())
        assert fwd > 100 and grd > 100, (name, fwd, grd)
