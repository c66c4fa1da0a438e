"""The dispatch mirror of tests/mlp_cases.py against the launch sites of csrc/pds_mlp.hip and csrc/pds_mlp_wide.hip (no
GPU): every instantiation that can run has a case in test_gpu_mlp_dispatch.py, so a new kernel variant without one, or a
case table that loses one, fails here."""
import os
import re
from collections import defaultdict

import mlp_cases as mc


def _src(name):
    with open(os.path.join(mc.CSRC, name)) as f:
        return f.read()


def _domain():
    """every predicate boundary of the host code: d_in on both sides of 16 / 32 / 34 / 48 / 64 and of each input-tile pair of
    launch_nin, hidden widths on both sides of 48 / 50 / 64 with h1 != h2, both losses, both activations, batches on both
    sides of the bf16 switch, with and without index / standardisation"""
    d_ins = (1, 15, 16, 17, 31, 32, 33, 34, 35, 47, 48, 49, 50, 63, 64, 65, 96, 97, 128, 129, 160, 161, 191, 192)
    hs = (1, 16, 17, 33, 48, 49, 50, 51, 63, 64)
    for kind in ("fwd", "ppo", "mse"):
        for act in ("relu", "tanh"):
            for d in d_ins:
                for h1 in hs:
                    for h2 in hs:
                        for B in (1, mc.BF16_MIN_SAMPLES - 1, mc.BF16_MIN_SAMPLES):
                            for index in (False, True):
                                for mean in (False, True):
                                    yield (kind, d, h1, h2, act, B, index, mean)


def test_constants_of_the_mirror_match_the_sources():
    common, narrow, wide = _src("pds_mlp_common.h"), _src("pds_mlp.hip"), _src("pds_mlp_wide.hip")
    for name, val in (("kTS", mc.TILE), ("kTW", mc.TILE), ("kMaxDim", mc.MAX_DIM), ("kWaves", mc.NARROW_WAVES),
                      ("kWideWaves", mc.WIDE_WAVES), ("kWideMaxBlocks", mc.MAX_BLOCKS), ("kMaxDimIn", 192)):
        assert re.search(rf"constexpr int {name} = {val};", common), name
    assert re.search(rf"constexpr int kMaxGridBlocks = {mc.MAX_BLOCKS};", narrow)
    assert re.search(r"constexpr int kPairs = kWaves / 2;", narrow)
    assert re.search(rf"return \(int\)\(blocks < {mc.MAX_BLOCKS} \? blocks : {mc.MAX_BLOCKS}\);", narrow)
    assert "PDS_MLP_SPLIT" not in narrow  # the split route is unconditional: no switch back to mlp_kernel, no third role
    assert re.search(rf'getenv\("PDS_BF16_MIN_SAMPLES"\); return e \? atoll\(e\) : {mc.BF16_MIN_SAMPLES}ll;', narrow)
    # the predicates restated in mlp_cases.py, as the host code spells them today
    for frag in ("const bool gb = a.m.h1 == kMaxDim || a.m.h2 == kMaxDim || a.m.d_in == kMaxDim;",
                 "const bool wide = gb ? a.m.d_in > 3 * kTW : a.m.d_in >= 3 * kTW;",
                 "const bool ktiled = a.m.d_in > kMaxDim;",
                 "inline bool two_hidden_steps(const pds_mlp &m) { return m.h1 == m.h2 && m.h1 > 48 && last_steps(m.h1) == 2; }",
                 "inline bool two_input_steps(const pds_mlp &m) { return m.d_in > 32 && m.d_in <= 48 && last_steps(m.d_in) == 2; }",
                 "const bool wide = m->d_in > 3 * kTW;"):
        assert frag in narrow, frag
    assert "const int nin = (a.m.d_in + kTW - 1) / kTW;" in wide
    for n in (6, 8, 10):
        assert f"if (nin <= {n}) hipLaunchKernelGGL((mlp_wide_kernel<LOSS, ACT, {n}>)" in wide or \
            f"else if (nin <= {n}) hipLaunchKernelGGL((mlp_wide_kernel<LOSS, ACT, {n}>)" in wide, n


def test_every_launch_site_resolves_to_an_instantiation():
    """17 sites in pds_mlp.hip (reduce_kernel one of them), 4 in pds_mlp_wide.hip: a new one must be added to the mirror
    and to the case table"""
    sites, raw = mc.launch_sites()
    assert raw == {"pds_mlp.hip": 17, "pds_mlp_wide.hip": 4}, raw
    pat = re.compile(r"^(mlp_kernel<LOSS_(PPO|MSE|NONE),[01],[12],(true|false),[24],[24]>|ppo_split_kernel<[24],(true|false)>|"
                     r"mlp_wide_kernel<LOSS_(PPO|MSE|NONE),[01],(6|8|10|12)>)$")
    for f, m in sites:
        assert pat.match(m), (f, m)
    assert len(sites) == 16 + 7 + 4 + 1 + 24  # PDS_MLP_LAUNCH x 4 calls, forward, split, critic, wide
    assert len(set(m for _, m in sites)) == len(sites)


def test_mirror_codomain_equals_the_launch_sites():
    launch = mc.launch_set()
    codomain = defaultdict(list)
    for kind, d, h1, h2, act, B, index, mean in _domain():
        codomain[mc.instantiation(kind, d, h1, h2, act, B, index, mean)].append((kind, d, h1, h2, act, B, index, mean))
    assert set(codomain) == launch, (set(codomain) ^ launch)


def _abi_unreachable():
    """instantiations that only a PPO call WITH an index or a standardisation would reach (the PPO entry points never pass
    either: checked against pds_ppo_policy_grad_step's body).  There is none: such a call falls through to the generic
    PDS_MLP_LAUNCH(LOSS_PPO, 0), which plain calls reach too."""
    text = _src("pds_mlp.hip")
    body = text[text.index('extern "C" int pds_ppo_policy_grad_step'):text.index('extern "C" int pds_ppo_policy_grad(')]
    assert "a.index" not in body and "a.mean" not in body
    reach, only = set(), set()
    for kind, d, h1, h2, act, B, index, mean in _domain():
        m = mc.instantiation(kind, d, h1, h2, act, B, index, mean)
        if kind == "ppo" and (index or mean):
            only.add(m)
        else:
            reach.add(m)
    return only - reach


def test_case_table_reaches_every_instantiation():
    unreachable = _abi_unreachable()
    assert unreachable == set(), unreachable  # every instantiation the library launches has a GPU case
    for c in mc.CASES:
        assert not (c.kind == "ppo" and (c.index or c.std)), c
        assert c.kind != "mse" or c.d_out == 1, c
    by_member = defaultdict(list)
    for c in mc.CASES:
        by_member[mc.case_member(c)].append(c)
    missing = mc.launch_set() - unreachable - set(by_member)
    assert not missing, sorted(missing)
    for member, cases in by_member.items():
        rnd = mc.family_round(member)
        # a tiny batch (less than one tile or exactly one) and a ragged tail past the second round of the persistent grid
        assert any(c.B <= mc.TILE + 1 for c in cases) or member.startswith("ppo_split_kernel<") and member.endswith("true>"), member
        assert any(c.B > 2 * rnd and c.B % mc.TILE for c in cases), member


def test_case_table_covers_the_shape_axes():
    cases = mc.CASES
    d_ins = {c.d_in for c in cases}
    assert {1, 3, 15, 16, 17, 31, 32, 33, 34, 47, 48, 49, 63, 64, 65, 96, 97, 128, 129, 160, 161, 191, 192} <= d_ins
    hs = {c.h1 for c in cases} & {c.h2 for c in cases}
    assert {1, 16, 17, 33, 48, 49, 50, 63, 64} <= hs
    for kind in ("fwd", "ppo", "mse"):
        assert any(c.h1 != c.h2 and c.d_in > mc.MAX_DIM for c in cases if c.kind == kind), kind
        assert any(c.h1 != c.h2 and c.d_in <= mc.MAX_DIM for c in cases if c.kind == kind), kind
        for act in ("relu", "tanh"):
            assert any(c.act == act for c in cases if c.kind == kind), (kind, act)
            assert any(c.act == act and c.d_in > mc.MAX_DIM for c in cases if c.kind == kind), (kind, act)
    assert {c.d_out for c in cases if c.kind != "mse"} >= set(range(1, 9))
    assert {c.d_out for c in cases if c.kind == "ppo" and c.d_in > mc.MAX_DIM} >= {1, 2, 3, 4, 5, 8}
    Bs = {c.B for c in cases}
    assert {1, 15, 16, 17, mc.BF16_MIN_SAMPLES - 1, mc.BF16_MIN_SAMPLES, 1 << 20} <= Bs
    assert any(c.kind == "mse" and c.B == 524288 and c.index == "perm" and c.d_in == 34 and c.h1 == 64 for c in cases)
    assert any(c.kind == "mse" and c.B == 524288 and c.index == "rep" for c in cases)
    for kind in ("fwd", "mse"):
        assert {c.index for c in cases if c.kind == kind} == {None, "perm", "rep"}, kind
    assert {(c.d_in, c.h1, c.act) for c in cases if c.kind == "fwd" and c.B == 1 << 20} >= {(34, 50, "relu"), (34, 64, "tanh")}
    # the K-tiled kernels: the first column of a new input tile pair for every NIN of launch_nin
    for d in (65, 97, 129, 161):
        for kind in ("fwd", "ppo", "mse"):
            assert any(c.d_in == d for c in cases if c.kind == kind), (d, kind)
