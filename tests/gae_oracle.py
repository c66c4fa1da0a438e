"""float64 references of csrc/pds_gae.hip (Buffer.finish_path, algs/core.py:461-533, with the cut-wins rule of
algs/iwpg/iwpg.py:374-379) and the bar the kernel is held to.

  gae_numpy    the reference Buffer's own form: per column, per path, `np.append(rews, last_val)` and two discount_cumsums
  gae_oracle   the same numbers as one backward recursion per column, which also returns, per output element, the sum S of
               magnitudes that the float32 roundings of that element are relative to
  BAR_ULPS     |got - want| <= BAR_ULPS * 2^-24 * S, element by element

The bar.  One step of the advantage chain in float32 without contraction rounds six times: r * scale, gamma * next_val, the
add, the subtraction of v, gl * next_adv, the last add.  Each rounding is at most 2^-24 of its result, every result is bounded
by the sum of the magnitudes that enter the step, and what the step inherits from t + 1 (the error of next_adv) is scaled by
gl -- so the error of adv[t] is at most 6 * 2^-24 * S_t with

  adv       S_t = |rs_t| + gamma |next_val| + |v_t| + gl |next_adv| + gl S_{t+1}
  target_v  S_adv + |a_t| + |v_t|                       (one more add)
  ret       S_t = |r_t| + gamma |next_ret| + gamma S_{t+1}  (two roundings per step)

to first order; S_{t+1} = 0 where a path ends at t.  gamma, lam, rew_scale and rew_clip enter as the float32 values the kernel
receives (a C float argument), so their own rounding is not part of the error."""
import numpy as np

U32 = 2.0 ** -24
BAR_ULPS = 6.0


def gae_numpy(rew, val, term, trunc, fval, last_val, gamma, lam, scale, clip):
    """Host restatement of Buffer.finish_path per path (algs/core.py:461-533) for [T, N] arrays."""
    T, N = rew.shape
    adv, tv, dr = np.zeros_like(rew), np.zeros_like(rew), np.zeros_like(rew)
    for n in range(N):
        start = 0
        for t in range(T):
            end = term[t, n] or trunc[t, n] or t == T - 1
            if not end:
                continue
            b = fval[t, n] if trunc[t, n] else (0.0 if term[t, n] else last_val[n])  # (cut wins: iwpg.py:374-379)
            r = np.append(rew[start:t + 1, n], b).astype(np.float64)
            v = np.append(val[start:t + 1, n], b).astype(np.float64)
            disc = np.zeros(len(r)); acc = 0.0
            for k in range(len(r) - 1, -1, -1):
                acc = r[k] + gamma * acc; disc[k] = acc
            rs = np.clip(r * scale, -clip, clip) if scale > 0 else r
            deltas = rs[:-1] + gamma * v[1:] - v[:-1]
            a = np.zeros(len(deltas)); acc = 0.0
            for k in range(len(deltas) - 1, -1, -1):
                acc = deltas[k] + gamma * lam * acc; a[k] = acc
            adv[start:t + 1, n], tv[start:t + 1, n], dr[start:t + 1, n] = a, a + v[:-1], disc[:-1]
            start = t + 1
    return adv, tv, dr


def _f32(x):
    return float(np.float32(x))


def gae_oracle(rew, val, term, trunc, fval, last_val, gamma, lam, scale=0.0, clip=10.0):
    """[T, N] arrays (fval may be None: a cut bootstraps with 0) -> ((adv, target_v, disc_ret), (S_adv, S_target_v, S_ret)),
    all float64 [T, N].  The columns are independent; the recursion runs over all of them at once."""
    rew, val = np.asarray(rew, dtype=np.float64), np.asarray(val, dtype=np.float64)
    T, N = rew.shape
    te, tr = np.asarray(term).astype(bool), np.asarray(trunc).astype(bool)
    gamma, lam, scale, clip = _f32(gamma), _f32(lam), _f32(scale), _f32(clip)
    gl = gamma * lam
    out = [np.zeros((T, N)) for _ in range(6)]
    adv, tv, dr, s_adv, s_tv, s_ret = out
    next_val = np.asarray(last_val, dtype=np.float64).reshape(N).copy()
    next_ret = next_val.copy()
    next_adv, sa_next, sr_next = np.zeros(N), np.zeros(N), np.zeros(N)
    for t in range(T - 1, -1, -1):
        end = te[t] | tr[t]
        with np.errstate(invalid="ignore"):  # (the fval rows no path reads may hold NaN)
            b = np.where(tr[t], np.zeros(N) if fval is None else np.asarray(fval[t], dtype=np.float64), 0.0)
        next_val, next_ret = np.where(end, b, next_val), np.where(end, b, next_ret)
        next_adv, sa_next, sr_next = np.where(end, 0.0, next_adv), np.where(end, 0.0, sa_next), np.where(end, 0.0, sr_next)
        r, v = rew[t], val[t]
        rs = np.clip(r * scale, -clip, clip) if scale > 0 else r
        a = rs + gamma * next_val - v + gl * next_adv
        g = r + gamma * next_ret
        sa = np.abs(rs) + gamma * np.abs(next_val) + np.abs(v) + gl * np.abs(next_adv) + gl * sa_next
        sr = np.abs(r) + gamma * np.abs(next_ret) + gamma * sr_next
        adv[t], tv[t], dr[t] = a, a + v, g
        s_adv[t], s_tv[t], s_ret[t] = sa, sa + np.abs(a) + np.abs(v), sr
        next_val, next_adv, next_ret, sa_next, sr_next = v, a, g, sa, sr
    return (adv, tv, dr), (s_adv, s_tv, s_ret)


def margins(got, want, S):
    """max over elements of |got - want| / (BAR_ULPS 2^-24 S) per output -> [adv, target_v, ret]; every `got` finite."""
    out = []
    for x, w, s in zip(got, want, S):
        x = np.asarray(x, dtype=np.float64)
        assert x.shape == w.shape and np.all(np.isfinite(x)), "shape / non-finite output"
        bar = BAR_ULPS * U32 * s
        err = np.abs(x - w)
        out.append(float(np.max(np.where(err == 0.0, 0.0, err / np.where(bar > 0, bar, np.finfo(float).tiny)))))
    return out


# ---- the GPU cases (tests/test_gpu_gae.py) and the float32 restatement's check of the bar (tests/test_gae_oracle_cpu.py) -----
#        id                 T    N     gamma lam   scale p_term p_trunc seed
CASES = [
    ("T1-all-end-kinds",    1,   256,  .99,  .95,  0.0,  .30,   .30,    11),   # one step; all four end kinds on the last step
    ("T2-N255-gamma0",      2,   255,  0.0,  .95,  0.0,  .20,   .20,    12),   # grid tail; disc_ret == rew, adv == rs - v on the bits
    ("T37-N257-both-flags", 37,  257,  .99,  .95,  0.0,  .05,   .03,    13),   # one lane of the second block; terminated AND cut rows
    ("T37-N1000-scaled",    37,  1000, .99,  .95,  0.37, .05,   .03,    14),   # scaling without a binding clip
    ("T500-N257-one-path",  500, 257,  1.0,  1.0,  0.0,  0.0,   0.0,    15),   # longest accumulation: 500 steps bootstrapped by last_val
    ("T500-N257-clip",      500, 257,  1.0,  1.0,  3.0,  0.0,   .002,   3),    # the clip binds
    ("T200-N64-lam0",       200, 64,   .9,   0.0,  0.37, .02,   .02,    16),   # one-step advantage
    ("T500-N1-term-at-cut", 500, 1,    .99,  .95,  0.37, None,  None,   17),   # one column; the path ends exactly at the cut
]
BOTH_FLAGS = ("T1-all-end-kinds", "T37-N257-both-flags")  # the cases that name `terminated AND cut`
CLIP = 10.0


def make_case(case, poison=True):
    """-> dict of numpy inputs: N(-1, 2) rewards, N(-3, 2) values; term / trunc drawn independently.  poison: fval is NaN at
    steps that are not truncated, last_val is NaN for columns that finish on the last step (the kernel must not read either)."""
    cid, T, N, gamma, lam, scale, p_te, p_tr, seed = case
    rs = np.random.RandomState(seed)
    rew = rs.normal(-1, 2, (T, N)).astype(np.float32)
    val = rs.normal(-3, 2, (T, N)).astype(np.float32)
    fval = rs.normal(-3, 2, (T, N)).astype(np.float32)
    last = rs.normal(-3, 2, N).astype(np.float32)
    if p_te is None:  # terminated at the last step
        term, trunc = np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
        term[T - 1] = 1
    else:
        term = (rs.rand(T, N) < p_te).astype(np.uint8)
        trunc = (rs.rand(T, N) < p_tr).astype(np.uint8)
    if poison:
        fval[trunc == 0] = np.nan
        last[(term[T - 1] | trunc[T - 1]) != 0] = np.nan
    return dict(rew=rew, val=val, term=term, trunc=trunc, fval=fval, last=last, gamma=gamma, lam=lam, scale=scale, clip=CLIP)


def check_case_inputs(case, d):
    """what a case asserts on its inputs: the rows it is there for exist (both flags on one step; a clip that binds on
    5 % .. 50 % of the rewards, with both signs)"""
    cid = case[0]
    if cid in BOTH_FLAGS:
        assert int(((d["term"] != 0) & (d["trunc"] != 0)).sum()) >= 1, cid
    if cid == "T500-N257-clip":
        x = d["rew"].astype(np.float64) * _f32(d["scale"])
        share = float((np.abs(x) > CLIP).mean())
        assert 0.05 <= share <= 0.50 and (x > CLIP).any() and (x < -CLIP).any(), (cid, share)
