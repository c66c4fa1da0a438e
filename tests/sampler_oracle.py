"""A numpy float64 restatement of the Gaussian sampler's contract (csrc/pds_device.h box_muller and
PDS_GAUSSIAN_PHILOX; csrc/pds_train.hip sample_kernel) -- what pds_gaussian_sample, the in-kernel samplers of the fused rollouts
and the noise of pds_es_* are documented to draw, written from the document and not from the kernels: vectorised Philox4x32-10
on uint64 arrays, the two-word Box-Muller in float64, the counter layout, and the affine map with its log-probability.

Also the statistics that hold a block of variates against N(0, 1): tests/test_sampler_oracle_cpu.py runs them on this
restatement alone, tests/test_gpu_sampler.py on the kernel's output with the same bars."""
from math import erfc, sqrt

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
R_MAX = sqrt(48.0 * np.log(2.0))  # sqrt(-2 ln 2^-24) = 5.768: the largest radius a 24-bit u1 gives
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)

# seeds of the distribution tests: (seed, call)
DISTRIBUTION_SEEDS = ((0x5EED0123456789, 3), (12345, 77))


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays of 32-bit words held in uint64; returns the four output words."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2  # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def box_muller64(a, b):
    """(z0, z1) of the word pair (a, b) in float64: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1)"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def normals64(n, d, seed, call, id_base=0):
    """z [n, d] (float64): variate j of sample id = id_base + row in call `call` under `seed`.  Counter = (id lo,
    (id hi << 8 | block) mod 2^32, call lo, call hi), key = (seed lo, seed hi); block b = j // 4; its words (x, y) give variates
    4 b and 4 b + 1, (z, w) give 4 b + 2 and 4 b + 3.  All of id, call, seed are taken mod 2^64."""
    m64 = (1 << 64) - 1
    seed, call, id_base = int(seed) & m64, int(call) & m64, int(id_base) & m64
    ids = (np.arange(n, dtype=np.uint64) + np.uint64(id_base))  # wraps mod 2^64 like the kernel's unsigned sum
    lo, hi = ids & M32, ids >> np.uint64(32)
    z = np.empty((n, 4 * ((d + 3) // 4)), dtype=np.float64)
    for b in range((d + 3) // 4):
        x, y, zz, w = philox4x32_10(lo, ((hi << np.uint64(8)) | np.uint64(b)) & M32, call & 0xFFFFFFFF, call >> 32,
                                    seed & 0xFFFFFFFF, seed >> 32)
        z[:, 4 * b], z[:, 4 * b + 1] = box_muller64(x, y)
        z[:, 4 * b + 2], z[:, 4 * b + 3] = box_muller64(zz, w)
    return z[:, :d]


def logp64(z, log_std):
    """sum_j -(z_j^2 / 2 + log_std_j + ln(2 pi) / 2) per row, float64"""
    z, log_std = np.asarray(z, dtype=np.float64), np.asarray(log_std, dtype=np.float64)
    return -(0.5 * z * z + log_std + HALF_LOG_2PI).sum(axis=-1)


def sample64(mu, log_std, seed, call, id_base=0, deterministic=False):
    """(act [n, d], logp [n], z [n, d]) of pds_gaussian_sample in float64: act = mu + exp(log_std) z"""
    mu, log_std = np.asarray(mu, dtype=np.float64), np.asarray(log_std, dtype=np.float64)
    n, d = mu.shape
    z = np.zeros((n, d)) if deterministic else normals64(n, d, seed, call, id_base)
    return mu + np.exp(log_std) * z, logp64(z, log_std), z


def distribution_statistics(z, others=(), z_bar=0.0):
    """Every statistic of the distribution test as (name, value, bar) with the requirement |value| <= bar: z [n, d], a float64
    torch tensor on any device (the CPU test passes this module's variates, the GPU test the kernel's); m = n d variates.
    Mean, variance, skewness, kurtosis within 5 standard errors; the Kolmogorov-Smirnov distance below the 0.1 % critical
    value 1.95 / sqrt(m); the counts beyond 3 / 4 / 5 sigma within 5 sqrt(want) + 1 of the normal's; max |z| <= R_MAX + z_bar;
    every column pair uncorrelated in value (5 / sqrt(n)) and in squares (10 / sqrt(n)); the neighbouring row and each tensor
    of `others` (name, z') -- the next call, the next seed -- uncorrelated (5 / sqrt(m))."""
    import torch
    assert z.dtype == torch.float64 and z.dim() == 2
    n, d = z.shape
    flat = z.reshape(-1)
    m = flat.numel()
    se = 1.0 / sqrt(m)
    out = []
    mean, var = float(flat.mean()), float(flat.var())
    c = flat - mean
    out.append(("mean", mean, 5 * se))
    out.append(("variance - 1", var - 1.0, 5 * sqrt(2.0) * se))
    out.append(("skewness", float((c ** 3).mean()) / var ** 1.5, 5 * sqrt(6.0) * se))
    out.append(("kurtosis - 3", float((c ** 4).mean()) / var ** 2 - 3.0, 5 * sqrt(24.0) * se))
    s, _ = torch.sort(flat)
    cdf = torch.special.ndtr(s)
    i = torch.arange(1, m + 1, device=z.device, dtype=torch.float64)
    out.append(("KS distance", float(torch.maximum((i / m - cdf).abs().max(), (cdf - (i - 1) / m).abs().max())), 1.95 * se))
    a = flat.abs()
    for t in (3.0, 4.0, 5.0):
        want = m * erfc(t / sqrt(2.0))
        out.append((f"count beyond {t:g} sigma - {want:.1f}", float((a > t).sum()) - want, 5 * sqrt(want) + 1))
    out.append(("max |z|", float(a.max()), R_MAX + z_bar))
    sq = z * z - 1.0
    corr_v, corr_s = (z.T @ z) / n, (sq.T @ sq) / n
    off = ~torch.eye(d, dtype=torch.bool, device=z.device)
    out.append((f"worst of {d * (d - 1) // 2} column-pair correlations", float(corr_v[off].abs().max()), 5 / sqrt(n)))
    out.append((f"worst of {d * (d - 1) // 2} column-pair correlations of squares", float(corr_s[off].abs().max()), 10 / sqrt(n)))
    out.append(("neighbouring row", float((z[:-1] * z[1:]).mean()), 5 * se))
    for name, other in others:
        out.append((name, float((z * other).mean()), 5 * se))
    return out
