"""GPU tests of the policy sampler and the trainer's bookkeeping kernels (csrc/pds_train.hip; box_muller and
PDS_GAUSSIAN_PHILOX in csrc/pds_device.h) against float64: pds_box_muller swept exhaustively in each factor, pds_gaussian_sample /
pds_gaussian_sample_dev / pds_counter_add and the noise of pds_es_perturb draw for draw against the restatement of the
contract in tests/sampler_oracle.py, pds_rollout_record exactly, pds_adam_step per step.

The bar on a standard normal.  The radius sweep (all 2^24 values of a >> 8 at b = 0: the angle is exactly 0 revolutions, z0 = r)
gives E_r = max |r_hip - r64|, the angle sweep (all 2^24 values of b >> 8 at a = 0) E_t = max over cos and sin of
|z_hip / r_hip(a = 0) - trig64|.  For any word pair then |z - z64| <= E_r + R_MAX E_t + 2^-23 |z64| (R_MAX = 5.768, the last
term: the rounding of the product r * cos).  E_z = E_r + R_MAX E_t as measured on the MI355X is in
profiles/gaussian_sample_accuracy.txt; Z_BAR = 1.25 E_z is the bar of every comparison of a draw below: the sweeps are
exhaustive in each factor, the margin covers only the interplay of the product's rounding with them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import phoenix_drone_simulation_amd as pds
from phoenix_drone_simulation_amd.fused import FusedMLP

import sampler_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64          # elements behind every output buffer that the kernels must leave alone
SENTINEL = 12345.0
# measured on the MI355X (profiles/gaussian_sample_accuracy.txt), rounded up to three digits
E_R = 4.88e-7
E_T = 1.65e-7
E_Z = E_R + so.R_MAX * E_T  # 1.44e-6
Z_BAR = 1.25 * E_Z         # 1.80e-6

SEED = 0x5EED0123456789
CALL = (1 << 33) + 3
ID_BASES = (0, (1 << 32) - 100, (1 << 40) + 7)   # small; the ids cross the 32-bit boundary inside the launch; high half in use
NS = (1, 255, 256, 257, 1000)                    # one lane; one block less one, exactly one, one more; four blocks with a partial one


def _lib():
    return pds.native.load()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _word(value):
    """a uint64 device word (torch holds the bits as int64)"""
    value &= (1 << 64) - 1
    return torch.tensor([value - (1 << 64) if value >> 63 else value], dtype=torch.int64, device=DEV)


def _read_word(t):
    return int(t.cpu()[0]) & ((1 << 64) - 1)


def z_close(got, want64):
    """|z - z64| <= Z_BAR + 2^-23 |z64| elementwise; returns the worst error in units of the bound"""
    err = np.abs(got.astype(np.float64) - want64)
    return float((err / (Z_BAR + 2.0 ** -23 * np.abs(want64))).max())


def sample(mu, log_std, seed, call, id_base=0, deterministic=False, call_word=None, expect=pds.native.OK):
    """pds_gaussian_sample (call_word None) or pds_gaussian_sample_dev (call = *call_word + call) into guarded buffers:
    (act [n, d], logp [n])"""
    n, d = mu.shape
    act = torch.full((n * d + GUARD,), SENTINEL, device=DEV)
    logp = torch.full((n + GUARD,), SENTINEL, device=DEV)
    if call_word is None:
        rc = _lib().pds_gaussian_sample(_ptr(mu), _ptr(log_std), n, d, seed, call, id_base, int(deterministic), _ptr(act),
                                        _ptr(logp), _stream())
    else:
        rc = _lib().pds_gaussian_sample_dev(_ptr(mu), _ptr(log_std), n, d, seed, _ptr(call_word), call, id_base,
                                            int(deterministic), _ptr(act), _ptr(logp), _stream())
    assert rc == expect
    if rc != pds.native.OK:
        assert bool((act == SENTINEL).all()) and bool((logp == SENTINEL).all()), "a refused call wrote its outputs"
        return None
    assert bool((act[n * d:] == SENTINEL).all()) and bool((logp[n:] == SENTINEL).all()), "the sampler wrote behind its outputs"
    return act[:n * d].reshape(n, d), logp[:n]


def normals(n, d, seed=SEED, call=CALL, id_base=0, **kw):
    """z [n, d] of the kernel: mu = 0, log_std = 0 make the action z itself"""
    return sample(torch.zeros(n, d, device=DEV), torch.zeros(d, device=DEV), seed, call, id_base, **kw)[0]


@functools.lru_cache(maxsize=None)
def reference(n, id_base, seed=SEED, call=CALL):
    """normals64 at d = 8, computed once per case and left unchanged"""
    z = so.normals64(n, 8, seed, call, id_base)
    z.setflags(write=False)
    return z


# ---- pds_box_muller: the accuracy of the hardware log / sqrt / sin / cos route, exhaustively in each factor ---------------------
def box_muller(words):
    """words [n, 2] (int64 numpy of 32-bit values) -> z [n, 2] float32 numpy"""
    w = torch.from_numpy(words.astype(np.uint32).view(np.int32)).to(DEV).contiguous()
    n = w.shape[0]
    out = torch.full((2 * n + GUARD,), SENTINEL, device=DEV)
    assert _lib().pds_box_muller(_ptr(w), n, _ptr(out), _stream()) == pds.native.OK
    assert bool((out[2 * n:] == SENTINEL).all()), "pds_box_muller wrote behind its output"
    return out[:2 * n].reshape(n, 2).cpu().numpy()


def test_box_muller_radius_sweep():
    """All 2^24 values of a >> 8 at b = 0: z0 = r, z1 = +-0, everything finite -- u1 = 2^-24 (a = 0: r = R_MAX, the cut-off) and
    u1 = 1 (a = 0xFFFFFFFF: r = 0, no NaN from the square root of -0) included.  E_r = max |r_hip - r64| is the measured figure
    the bar on z rests on: it must not exceed the recorded one."""
    words = np.zeros((1 << 24, 2), dtype=np.int64)
    words[:, 0] = np.arange(1 << 24, dtype=np.int64) << 8
    words[-1, 0] = 0xFFFFFFFF
    z = box_muller(words)
    r64, _ = so.box_muller64(words[:, 0], words[:, 1])
    assert np.isfinite(z).all()
    assert (z[:, 1] == 0.0).all()
    assert z[-1, 0] == 0.0 and abs(float(z[0, 0]) - so.R_MAX) < 1e-5
    err = np.abs(z[:, 0].astype(np.float64) - r64)
    e_r = float(err.max())
    print(f"E_r = {e_r:.4e} at a >> 8 = {int(err.argmax())} (r64 = {r64[err.argmax()]:.6f}); recorded {E_R:.4e}")
    assert e_r <= E_R


def test_box_muller_angle_sweep():
    """All 2^24 values of b >> 8 at a = 0 (the largest radius): E_t = max over cos and sin of |z_hip / r_hip(a = 0) - trig64|."""
    words = np.zeros((1 << 24, 2), dtype=np.int64)
    words[:, 1] = np.arange(1 << 24, dtype=np.int64) << 8
    z = box_muller(words).astype(np.float64)
    assert np.isfinite(z).all()
    r_hip = z[0, 0]  # b = 0: the angle is exactly 0 revolutions
    u2 = np.arange(1 << 24, dtype=np.float64) * 2.0 ** -24
    err_c, err_s = np.abs(z[:, 0] / r_hip - np.cos(2.0 * np.pi * u2)), np.abs(z[:, 1] / r_hip - np.sin(2.0 * np.pi * u2))
    e_t = float(max(err_c.max(), err_s.max()))
    print(f"E_t = {e_t:.4e} (cos {float(err_c.max()):.4e} at {int(err_c.argmax())}, sin {float(err_s.max()):.4e} at "
          f"{int(err_s.argmax())}); r_hip(a = 0) = {r_hip:.7f}; recorded {E_T:.4e}")
    assert e_t <= E_T


def test_box_muller_ignores_the_low_bits_and_meets_the_bar():
    """The low 8 bits of both words do not matter (the bits of the same words with them cleared), random word pairs sit within
    the bar on z, and the entry point refuses NULL pointers and n < 1."""
    rs = np.random.RandomState(5)
    words = rs.randint(0, 1 << 32, size=(4096, 2), dtype=np.int64)
    words[:4] = [[0xFF, 0xFF], [0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFF00, 0xFF], [0x000000FF, 0xFFFFFFFF]]
    assert (words & 0xFF).any(axis=1).all()
    z = box_muller(words)
    assert np.array_equal(z.view(np.uint32), box_muller(words & 0xFFFFFF00).view(np.uint32))
    z0, z1 = so.box_muller64(words[:, 0], words[:, 1])
    worst = z_close(z, np.stack([z0, z1], axis=1))
    print(f"4096 random word pairs: worst error {worst:.3f} of the bar {Z_BAR:.3e}")
    assert worst <= 1.0
    w = torch.zeros(8, dtype=torch.int32, device=DEV)
    out = torch.full((8,), SENTINEL, device=DEV)
    lib = _lib()
    for args in ((None, 4, _ptr(out)), (_ptr(w), 4, None), (_ptr(w), 0, _ptr(out)), (_ptr(w), -1, _ptr(out))):
        assert lib.pds_box_muller(*args, _stream()) == pds.native.EINVAL
    assert bool((out == SENTINEL).all())


# ---- pds_gaussian_sample draw for draw --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("id_base", ID_BASES)
@pytest.mark.parametrize("n", NS)
def test_draws_follow_the_contract(n, id_base):
    """Every d in 1 .. 8: the action at mu = 0, log_std = 0 against normals64 at the z bar, with the high halves of seed, call
    and sample id in use.  A wrong counter field gives differences of order 1."""
    want = reference(n, id_base)
    for d in range(1, 9):
        got = normals(n, d, id_base=id_base).cpu().numpy()
        worst = z_close(got, want[:, :d])
        print(f"n {n} d {d} id_base {id_base:#x}: worst error {worst:.3f} of the bar")
        assert worst <= 1.0, (d, float(np.abs(got - want[:, :d]).max()))


def test_draws_at_small_counters_and_at_the_last_id():
    """(seed, call) = (3, 1), what the older tests use, and the four largest ids the counter packing holds"""
    assert z_close(normals(1000, 4, seed=3, call=1).cpu().numpy(), so.normals64(1000, 4, 3, 1)) <= 1.0
    top = (1 << 56) - 4
    assert z_close(normals(4, 8, id_base=top).cpu().numpy(), so.normals64(4, 8, SEED, CALL, top)) <= 1.0


@pytest.mark.parametrize("id_base", ID_BASES[1:])
def test_column_and_slice_structure_is_bitwise(id_base):
    n = 1000
    whole = normals(n, 8, id_base=id_base)
    for d in range(1, 8):
        assert torch.equal(normals(n, d, id_base=id_base), whole[:, :d]), d
    for k in (1, 99, 100, 101, 256, 999):
        assert torch.equal(normals(n - k, 8, id_base=id_base + k), whole[k:]), k
        assert torch.equal(normals(n - k, 3, id_base=id_base + k), whole[k:, :3]), k
    assert not torch.equal(whole[:, :4], whole[:, 4:])


def logp_bound(z64, log_std64):
    """(d + 3) 2^-24 sum_j (z_j^2 / 2 + |ls_j| + 0.919)"""
    d = z64.shape[1]
    return (d + 3) * 2.0 ** -24 * (0.5 * z64 * z64 + np.abs(log_std64) + so.HALF_LOG_2PI).sum(axis=1)


@pytest.mark.parametrize("d", (1, 3, 4, 5, 8))
@pytest.mark.parametrize("n", (257, 1000))
def test_affine_map_and_log_probability_against_float64(n, d):
    """z is the kernel's own draw (the mu = 0, log_std = 0 call, held against the contract above); with it in float64:
    |act - (mu + e^ls z)| <= 2^-23 |e^ls z| + 2^-24 |act|: expf is within 1 ulp (a relative 2^-23 on the product), and the fmaf
    rounds once (half an ulp of act).
    |logp - logp64(z)| <= (d + 3) 2^-24 sum_j (z_j^2 / 2 + |ls_j| + 0.919): a term -z^2 / 2 - ls - c takes at most three
    roundings (the square -- the halving is exact --, two subtractions; fewer where the compiler contracts) and the float32
    constant c is within 2^-24 c, each at most 2^-24 of the term's absolute sum; adding the d terms takes d - 1 more roundings,
    each at most 2^-24 of the absolute sum of all terms.  First order, for any summation or contraction order.  Derived, not
    measured."""
    g = torch.Generator().manual_seed(10 * n + d)
    mu = torch.randn(n, d, generator=g).to(DEV)
    log_std = torch.linspace(-3.0, 0.5, 8)[torch.randperm(8, generator=g)[:d]].to(DEV)
    id_base = (1 << 32) - 100
    z = normals(n, d, id_base=id_base)
    act, logp = sample(mu, log_std, SEED, CALL, id_base)
    z64, mu64, ls64 = z.cpu().double().numpy(), mu.cpu().double().numpy(), log_std.cpu().double().numpy()
    act_np, logp_np = act.cpu().double().numpy(), logp.cpu().double().numpy()
    sz = np.exp(ls64) * z64
    err, bound = np.abs(act_np - (mu64 + sz)), 2.0 ** -23 * np.abs(sz) + 2.0 ** -24 * np.abs(act_np)
    print(f"n {n} d {d}: act worst error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    lerr, lbound = np.abs(logp_np - so.logp64(z64, ls64)), logp_bound(z64, ls64)
    print(f"n {n} d {d}: logp worst error / bound {float((lerr / lbound).max()):.3f}")
    assert (lerr <= lbound).all()
    # the whole of it against the contract: act and logp of sample64 with the z bar carried through
    act64, logp64, zc = so.sample64(mu64, ls64, SEED, CALL, id_base)
    zb = Z_BAR + 2.0 ** -23 * np.abs(zc)
    assert (np.abs(act_np - act64) <= np.exp(ls64) * zb + bound).all()
    assert (np.abs(logp_np - logp64) <= ((np.abs(zc) + zb) * zb).sum(axis=1) + lbound).all()


@pytest.mark.parametrize("d", (1, 4, 7))
def test_deterministic_mode(d):
    """act == mu bitwise, logp = -sum(ls + ln(2 pi) / 2) to the bound of the log-probability at z = 0, whatever the seed"""
    n = 257
    g = torch.Generator().manual_seed(d)
    mu = torch.randn(n, d, generator=g).to(DEV)
    log_std = torch.linspace(-3.0, 0.5, d).to(DEV)
    act, logp = sample(mu, log_std, SEED, CALL, 7, deterministic=True)
    assert torch.equal(act, mu)
    ls64 = log_std.cpu().double().numpy()
    zero = np.zeros((n, d))
    assert (np.abs(logp.cpu().double().numpy() - so.logp64(zero, ls64)) <= logp_bound(zero, ls64)).all()
    for seed, call, id_base in ((SEED + 1, CALL, 7), (3, 1, 0), (SEED, CALL + 1, 1 << 40)):
        act2, logp2 = sample(mu, log_std, seed, call, id_base, deterministic=True)
        assert torch.equal(act2, act) and torch.equal(logp2, logp)
    word = _word(5)
    act2, logp2 = sample(mu, log_std, 1, 2, 3, deterministic=True, call_word=word)
    assert torch.equal(act2, act) and torch.equal(logp2, logp)


@pytest.mark.parametrize("seed,call", so.DISTRIBUTION_SEEDS)
def test_draws_against_the_normal_distribution(seed, call):
    """2^21 rows of d = 8 (2^24 variates) through the statistics of sampler_oracle.distribution_statistics -- the bars that
    tests/test_sampler_oracle_cpu.py shows the float64 restatement alone to meet at these seeds."""
    n = 1 << 21
    z = normals(n, 8, seed=seed, call=call).double()
    assert bool(torch.isfinite(z).all())
    others = (("next call", normals(n, 8, seed=seed, call=call + 1).double()),
              ("next seed", normals(n, 8, seed=seed + 1, call=call).double()))
    for name, value, bar in so.distribution_statistics(z, others, z_bar=Z_BAR):
        print(f"seed {seed:#x} call {call}: {name}: {value:.6g} (bar {bar:.6g}, {abs(value) / bar:.2f} of it)")
        assert abs(value) <= bar, (name, value, bar)
    assert float(z.abs().max()) > 5.0


# ---- the device call counter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word,offset", (((1 << 32) - 1, 1), ((1 << 64) - 1, 2)))
def test_device_call_counter(word, offset):
    """pds_gaussian_sample_dev(word W, offset o) gives the bits of pds_gaussian_sample(call = (W + o) mod 2^64), and those follow
    the contract"""
    n, d = 257, 5
    g = torch.Generator().manual_seed(1)
    mu, log_std = torch.randn(n, d, generator=g).to(DEV), torch.linspace(-1.0, 0.3, d).to(DEV)
    call = (word + offset) & ((1 << 64) - 1)
    w = _word(word)
    act, logp = sample(mu, log_std, SEED, offset, 11, call_word=w)
    want_act, want_logp = sample(mu, log_std, SEED, call, 11)
    assert torch.equal(act, want_act) and torch.equal(logp, want_logp)
    assert _read_word(w) == word  # the sampler only reads the word
    assert z_close(normals(n, d, call=offset, id_base=11, call_word=w).cpu().numpy(), so.normals64(n, d, SEED, call, 11)) <= 1.0


@pytest.mark.parametrize("word", ((1 << 32) - 1, (1 << 64) - 1, 0))
def test_counter_add(word):
    """pds_counter_add leaves exactly (W + inc) mod 2^64 and nothing else; a following _dev call uses it"""
    inc = (1 << 33) + 5
    buf = torch.cat([_word(word), torch.full((GUARD,), 0x0123456789ABCDEF, dtype=torch.int64, device=DEV)])
    assert _lib().pds_counter_add(_ptr(buf), inc, _stream()) == pds.native.OK
    after = (word + inc) & ((1 << 64) - 1)
    assert _read_word(buf) == after and bool((buf[1:] == 0x0123456789ABCDEF).all())
    assert torch.equal(normals(300, 8, call=2, call_word=buf), normals(300, 8, call=(after + 2) & ((1 << 64) - 1)))
    assert _lib().pds_counter_add(None, inc, _stream()) == pds.native.EINVAL


# ---- the ES noise without the detour through the sampler --------------------------------------------------------------------------
@pytest.mark.parametrize("cross", (False, True))
@pytest.mark.parametrize("n", (9, 170))
def test_es_noise_follows_the_contract(n, cross):
    """pds_es_perturb with mu = 0, sigma = 1 gives the rows +eps / -eps; eps against normals64 (sample id (pair_base + i) Q + q,
    d = 8) at the z bar -- also with a pair_base that makes the ids cross 2^32 inside the launch."""
    pairs, generation = 3, 3
    Q = (n + 7) // 8
    pair_base = -(-(1 << 32) // Q) - 2 if cross else 0
    if cross:
        assert pair_base * Q < 1 << 32 < (pair_base + pairs) * Q
    buf = torch.full((2 * pairs * n + GUARD,), SENTINEL, device=DEV)
    rc = _lib().pds_es_perturb(_ptr(torch.zeros(n, device=DEV)), n, pairs, 1.0, SEED, generation, pair_base, _ptr(buf), _stream())
    assert rc == pds.native.OK
    assert bool((buf[2 * pairs * n:] == SENTINEL).all())
    theta = buf[:2 * pairs * n].reshape(2 * pairs, n).cpu().numpy()
    assert np.array_equal(theta[1::2], -theta[0::2])
    want = so.normals64(pairs * Q, 8, SEED, generation, pair_base * Q).reshape(pairs, 8 * Q)[:, :n]
    worst = z_close(theta[0::2], want)
    print(f"n {n} pair_base {pair_base}: worst error {worst:.3f} of the bar")
    assert worst <= 1.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_sampler_refusals():
    """d_out of 0 and 9, n = 0, each NULL pointer and sample ids beyond 2^56 (the counter packs id hi << 8 | block into one word)
    return PDS_EINVAL from both entry points and leave the outputs as they were"""
    lib, E = _lib(), pds.native.EINVAL
    n, d = 10, 4
    mu, ls = torch.zeros(n, d, device=DEV), torch.zeros(d, device=DEV)
    act, logp = torch.full((n * d,), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV)
    word = _word(1)
    good = dict(mu=_ptr(mu), ls=_ptr(ls), n=n, d=d, id_base=0, act=_ptr(act), logp=_ptr(logp))
    cases = [dict(d=0), dict(d=9), dict(d=-1), dict(n=0), dict(n=-5), dict(mu=None), dict(ls=None), dict(act=None), dict(logp=None),
             dict(id_base=(1 << 56) - n + 1), dict(id_base=1 << 56), dict(id_base=(1 << 64) - 1), dict(id_base=(1 << 64) - n)]
    for case in cases:
        a = {**good, **case}
        assert lib.pds_gaussian_sample(a["mu"], a["ls"], a["n"], a["d"], SEED, CALL, a["id_base"], 0, a["act"], a["logp"],
                                       _stream()) == E, case
        assert lib.pds_gaussian_sample_dev(a["mu"], a["ls"], a["n"], a["d"], SEED, _ptr(word), 0, a["id_base"], 0, a["act"],
                                           a["logp"], _stream()) == E, case
    assert bool((act == SENTINEL).all()) and bool((logp == SENTINEL).all())
    # ... and id_base + n == 2^56 is the last launch that fits
    assert lib.pds_gaussian_sample(_ptr(mu), _ptr(ls), n, d, SEED, CALL, (1 << 56) - n, 0, _ptr(act), _ptr(logp), _stream()) == 0
    assert z_close(act.reshape(n, d).cpu().numpy(), so.normals64(n, d, SEED, CALL, (1 << 56) - n)) <= 1.0


# ---- pds_rollout_record, exactly -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 1000))
def test_rollout_record_exactly(n):
    """T = 4 steps with small integer rewards (|r| <= 8): every running return and every sum in stats is an integer far below
    2^24, exact in float32 whatever the order of the atomics, so the comparison with a plain loop over time and envs is ==.
    Step 0: no env done (nothing is added to stats); step 1: terminated only / truncated only / both / neither mixed;
    step 2: every env done; step 3: mixed again.  Episode return, length and stats start from non-zero values."""
    T = 4
    rs = np.random.RandomState(n)
    rew = rs.randint(-8, 9, size=(T, n)).astype(np.float32)
    kind = rs.randint(0, 4, size=(T, n))              # 0 neither, 1 terminated only, 2 truncated only, 3 both
    kind[0] = 0
    kind[2] = rs.randint(1, 4, size=n)
    kind[1, :min(n, 4)] = [1, 2, 3, 0][:min(n, 4)]
    term, trunc = ((kind == 1) | (kind == 3)).astype(np.uint8), ((kind == 2) | (kind == 3)).astype(np.uint8)
    ep_ret0, ep_len0 = rs.randint(-8, 9, size=n).astype(np.float32), rs.randint(0, 6, size=n).astype(np.float32)
    stats0 = np.array([3.0, 7.0, 2.0], dtype=np.float32)

    # the reference: a plain loop
    er, el, st = ep_ret0.astype(np.float64), ep_len0.astype(np.float64), stats0.astype(np.float64)
    st_after = []
    for t in range(T):
        for i in range(n):
            er[i] += rew[t, i]
            el[i] += 1.0
            if term[t, i] or trunc[t, i]:
                st += (er[i], el[i], 1.0)
                er[i] = el[i] = 0.0
        st_after.append(st.copy())
    assert np.array_equal(st_after[0], stats0) and st_after[2][2] - st_after[1][2] == n

    def guarded(a, dtype):
        t = torch.full((a.size + GUARD,), 77, dtype=dtype, device=DEV)
        t[:a.size] = torch.from_numpy(a.reshape(-1)).to(DEV)
        return t
    rew_buf = torch.full((T * n + GUARD,), SENTINEL, device=DEV)
    term_buf = torch.full((T * n + GUARD,), 77, dtype=torch.uint8, device=DEV)
    trunc_buf = torch.full((T * n + GUARD,), 77, dtype=torch.uint8, device=DEV)
    ep_ret, ep_len, stats = guarded(ep_ret0, torch.float32), guarded(ep_len0, torch.float32), guarded(stats0, torch.float32)
    d_rew, d_term, d_trunc = (torch.from_numpy(a).to(DEV) for a in (rew, term, trunc))
    for t in range(T):
        rc = _lib().pds_rollout_record(_ptr(d_rew[t]), _ptr(d_term[t]), _ptr(d_trunc[t]), n, _ptr(rew_buf[t * n:]),
                                       _ptr(term_buf[t * n:]), _ptr(trunc_buf[t * n:]), _ptr(ep_ret), _ptr(ep_len), _ptr(stats),
                                       _stream())
        assert rc == pds.native.OK
        assert np.array_equal(stats[:3].cpu().numpy().astype(np.float64), st_after[t]), t
        # the slices of the steps still to come are untouched
        assert bool((rew_buf[(t + 1) * n:] == SENTINEL).all()) and bool((term_buf[(t + 1) * n:] == 77).all())
        assert bool((trunc_buf[(t + 1) * n:] == 77).all())
    assert np.array_equal(rew_buf[:T * n].reshape(T, n).cpu().numpy(), rew)
    assert np.array_equal(term_buf[:T * n].reshape(T, n).cpu().numpy(), term)
    assert np.array_equal(trunc_buf[:T * n].reshape(T, n).cpu().numpy(), trunc)
    assert np.array_equal(ep_ret[:n].cpu().numpy().astype(np.float64), er)
    assert np.array_equal(ep_len[:n].cpu().numpy().astype(np.float64), el)
    for buf, size in ((ep_ret, n), (ep_len, n), (stats, 3)):
        assert bool((buf[size:] == 77).all())
    assert torch.equal(d_rew, torch.from_numpy(rew).to(DEV)) and torch.equal(d_term, torch.from_numpy(term).to(DEV))  # inputs intact


# ---- pds_adam_step, per step, against float64 -------------------------------------------------------------------------------------
def ulp32(x):
    """the float32 unit in the last place at |x| (float64 array in, float64 out)"""
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("step", (1, 2, 10, 1000, 10 ** 6))
@pytest.mark.parametrize("sizes", ((1, 1, 1, 1), (34, 50, 50, 4)))
def test_adam_step_against_float64(sizes, step):
    """One pds_adam_step at optimiser step `step` from a random state (m, v), against float64 with the float32 values of lr,
    beta1, beta2, eps that the ABI receives.  u = 2^-24.

    exp_avg_sq = b2 v + ((1 - b2) g) g: 1 - b is exact (Sterbenz), every term is >= 0, and each of the at most four roundings is
    at most half an ulp of a quantity no larger than the result: within 2 ulp of the float64 value.
    exp_avg = b1 m + (1 - b1) g: the same count, within 2 ulp -- of the largest of the result and its two terms: where the
    terms have opposite signs the float32 rounding of a term is already that large whatever the kernel does with it (for terms
    of one sign the largest is the result itself, and the bar is 2 ulp of the result).
    The increment p_new - p_old against inc64 = -(lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps), m', v', bc1 = 1 - b1^t,
    bc2 = 1 - b2^t in float64:
      the quotient     7 u |inc64|, 3.5 ulp: one rounding (relative u) each for sqrtf(v'), the division by sqrt(bc2), the sum with
                       eps, m' / denom, lr / bc1, their product, and the host's sqrtf(bc2);
                       + the kernel's own m' and v' within the bars above: (lr / bc1) / denom * bar(m') and
                       |inc64| * bar(v') / (2 v') (the square root halves a relative error);
      the corrections  powf is within 1 ulp of a number below 1, at most u in absolute terms, and the subtraction from 1 rounds
                       by at most u / 2: 1.5 u / (1 - b1^t) on bc1, half of 1.5 u / (1 - b2^t) on the square root of bc2,
                       relative to |inc64|;
      the store        u max(|p_old|, |p_new|): p - x rounds once.
    First order.  Derived, not measured.  Gradients: magnitudes 1e-3 .. 10, exact zeros and 1e-20, whose square underflows in
    float32; every result must be finite.  Every parameter tensor is compared on its own, so an element that lands in the wrong
    tensor or at the wrong offset shows (all gradients differ)."""
    d_in, h1, h2, d_out = sizes
    torch.manual_seed(sum(sizes))
    net = torch.nn.Sequential(torch.nn.Linear(d_in, h1), torch.nn.Tanh(), torch.nn.Linear(h1, h2), torch.nn.Tanh(),
                              torch.nn.Linear(h2, d_out)).to(DEV)
    f = FusedMLP(net, "tanh")
    total = f.flat_grad.numel()
    assert total == h1 * d_in + h1 + h2 * h1 + h2 + d_out * h2 + d_out
    rs = np.random.RandomState(step % 1000 + total)
    if total == 6:
        g = np.array([1e-3, -10.0, 0.0, 1e-20, 0.5, -2.0])
    else:
        g = 10.0 ** rs.uniform(-3.0, 1.0, size=total) * rs.choice([-1.0, 1.0], size=total)
        g[rs.rand(total) < 0.1] = 0.0
        g[rs.rand(total) < 0.1] = 1e-20
        g[:4] = [0.0, 1e-20, -1e-20, 10.0]
    g = g.astype(np.float32)
    m0 = (0.1 * rs.standard_normal(total)).astype(np.float32)
    v0 = (10.0 ** rs.uniform(-6.0, 0.0, size=total)).astype(np.float32)
    lr, b1, b2, eps = (float(np.float32(v)) for v in (1e-2, 0.9, 0.999, 1e-8))

    def guarded(a):
        t = torch.full((total + GUARD,), SENTINEL, device=DEV)
        t[:total] = torch.from_numpy(a).to(DEV)
        return t
    em, ev = guarded(m0), guarded(v0)
    f.exp_avg, f.exp_avg_sq, f.adam_steps = em[:total], ev[:total], step - 1
    f.flat_grad.copy_(torch.from_numpy(g).to(DEV))
    p_old = [p.detach().clone() for p in f.params]
    f.adam_step(lr, betas=(b1, b2), eps=eps)
    assert f.adam_steps == step
    assert bool((em[total:] == SENTINEL).all()) and bool((ev[total:] == SENTINEL).all())
    assert torch.equal(f.flat_grad, torch.from_numpy(g).to(DEV))

    u = 2.0 ** -24
    g64, m64, v64 = g.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    t1, t2 = b1 * m64, (1.0 - b1) * g64
    m_new, v_new = t1 + t2, b2 * v64 + (1.0 - b2) * g64 * g64
    bar_m = 2.0 * ulp32(np.maximum(np.abs(m_new), np.maximum(np.abs(t1), np.abs(t2))))
    bar_v = 2.0 * ulp32(v_new)
    got_m, got_v = em[:total].cpu().double().numpy(), ev[:total].cpu().double().numpy()
    assert np.isfinite(got_m).all() and np.isfinite(got_v).all()
    print(f"{sizes} step {step}: exp_avg worst error / bar {float((np.abs(got_m - m_new) / bar_m).max()):.3f}, "
          f"exp_avg_sq {float((np.abs(got_v - v_new) / bar_v).max()):.3f}")
    assert (np.abs(got_m - m_new) <= bar_m).all()
    assert (np.abs(got_v - v_new) <= bar_v).all()

    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v_new) / np.sqrt(bc2) + eps
    inc64 = -(lr / bc1) * (m_new / denom)
    rel = 7 * u + bar_v / (2.0 * v_new) + 1.5 * u / bc1 + 0.75 * u / bc2
    bound_inc = np.abs(inc64) * rel + (lr / bc1) / denom * bar_m
    off = 0
    for p, old in zip(f.params, p_old):
        k = p.numel()
        new64, old64 = p.detach().reshape(-1).cpu().double().numpy(), old.reshape(-1).cpu().double().numpy()
        assert np.isfinite(new64).all()
        err = np.abs((new64 - old64) - inc64[off:off + k])
        bound = bound_inc[off:off + k] + u * np.maximum(np.abs(new64), np.abs(old64))
        print(f"{sizes} step {step}: tensor {tuple(p.shape)} worst increment error / bound {float((err / bound).max()):.3f}; "
              f"share of the store in the bound {float((u * np.abs(old64) / bound).mean()):.2f}")
        assert (err <= bound).all(), tuple(p.shape)
        off += k
    assert off == total
