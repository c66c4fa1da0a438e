"""The float64 restatement of the sampler contract (tests/sampler_oracle.py) on its own: its Philox against the Random123
known answers and the C oracle's, its Box-Muller at the edges, its counter layout, and every statistical bar that
tests/test_gpu_sampler.py holds the kernel to -- the bars are the reference's to meet first."""
import numpy as np
import pytest

import sampler_oracle as so


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32 10 rounds"""
    ones = 0xFFFFFFFF
    assert [int(w) for w in so.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(w) for w in so.philox4x32_10(ones, ones, ones, ones, ones, ones)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # (the third vector of the file: the digits of pi)
    assert [int(w) for w in so.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)] == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_philox_agrees_with_the_c_oracle():
    from oracle import oracle as po
    rs = np.random.RandomState(11)
    words = rs.randint(0, 1 << 32, size=(300, 6), dtype=np.uint64)
    words[:8] = [[0, 0, 0, 0, 0, 0], [0xFFFFFFFF] * 6, [0xFFFFFFFF, 0, 0, 0, 0, 0], [0, 0xFFFFFFFF, 0, 0, 0, 0],
                 [0, 0, 0xFFFFFFFF, 0, 0, 0], [0, 0, 0, 0xFFFFFFFF, 0, 0], [0, 0, 0, 0, 0xFFFFFFFF, 0], [0, 0, 0, 0, 0, 0xFFFFFFFF]]
    got = np.stack(so.philox4x32_10(*words.T), axis=1)
    assert got.dtype == np.uint64 and int(got.max()) < 1 << 32
    for row, g in zip(words, got):
        assert [int(v) for v in g] == po.philox4x32_10([int(v) for v in row[:4]], [int(v) for v in row[4:]])


def test_box_muller_edges():
    z0, z1 = so.box_muller64([0, 0xFF, 0xFFFFFFFF, 0xFFFFFF00, 0], [0, 0xFF, 0, 0, 0x40000000])
    assert z0[0] == so.R_MAX == z0[1] and abs(so.R_MAX - 5.768) < 1e-3 and z1[0] == 0.0  # the low 8 bits do not matter
    assert z0[2] == 0.0 and z0[3] == 0.0 and z1[2] == 0.0                                 # u1 = 1: r = 0, no NaN from sqrt(-0)
    assert abs(z0[4]) < 1e-15 and z1[4] == so.R_MAX                                       # a quarter turn
    assert np.isfinite(z0).all() and np.isfinite(z1).all()


def test_counter_layout():
    """each field of the counter where the contract puts it, on ids / calls / seeds with their high halves in use"""
    seed, call = 0x5EED0123456789, (1 << 33) + 3
    for id_base in ((1 << 32) - 3, (1 << 40) + 7):
        z = so.normals64(6, 8, seed, call, id_base)
        for i in range(6):
            gid = id_base + i
            for b in range(2):
                w = so.philox4x32_10(gid & 0xFFFFFFFF, ((gid >> 32) << 8 | b) & 0xFFFFFFFF, call & 0xFFFFFFFF, call >> 32,
                                     seed & 0xFFFFFFFF, seed >> 32)
                z0, z1 = so.box_muller64(w[0], w[1])
                z2, z3 = so.box_muller64(w[2], w[3])
                assert [float(z0), float(z1), float(z2), float(z3)] == list(z[i, 4 * b:4 * b + 4])
    z = so.normals64(16, 8, seed, call, 5)
    for d in range(1, 8):
        assert np.array_equal(so.normals64(16, d, seed, call, 5), z[:, :d])
    assert np.array_equal(so.normals64(10, 8, seed, call, 11), z[6:])
    assert not np.array_equal(z[:, :4], z[:, 4:])
    for other in (so.normals64(16, 8, seed + (1 << 32), call, 5), so.normals64(16, 8, seed, call + (1 << 32), 5),
                  so.normals64(16, 8, seed, call, 5 + (1 << 32)), so.normals64(16, 8, seed + 1, call, 5)):
        assert np.abs(other - z).max() > 1.0


def test_sample_and_log_probability():
    rs = np.random.RandomState(2)
    mu, ls = rs.standard_normal((50, 3)), np.array([-3.0, -0.5, 0.5])
    act, logp, z = so.sample64(mu, ls, 9, 4, 100)
    assert np.array_equal(z, so.normals64(50, 3, 9, 4, 100))
    assert np.allclose(act, mu + np.exp(ls) * z, rtol=0, atol=1e-15)
    from scipy import stats
    assert np.allclose(logp, stats.norm(mu, np.exp(ls)).logpdf(act).sum(-1), rtol=1e-9, atol=1e-9)
    act, logp, z = so.sample64(mu, ls, 9, 4, 100, deterministic=True)
    assert np.array_equal(act, mu) and np.allclose(logp, -(ls + so.HALF_LOG_2PI).sum())


@pytest.mark.parametrize("seed,call", so.DISTRIBUTION_SEEDS)
def test_restatement_meets_every_statistical_bar(seed, call):
    """n = 2^21 rows of d = 8 (2^24 variates), the shapes and bars of the GPU test"""
    n = 1 << 21
    import torch
    z = torch.from_numpy(so.normals64(n, 8, seed, call))
    others = (("next call", torch.from_numpy(so.normals64(n, 8, seed, call + 1))),
              ("next seed", torch.from_numpy(so.normals64(n, 8, seed + 1, call))))
    for name, value, bar in so.distribution_statistics(z, others):
        print(f"seed {seed:#x} call {call}: {name}: {value:.6g} (bar {bar:.6g}, {abs(value) / bar:.2f} of it)")
        assert abs(value) <= bar, (name, value, bar)
    assert float(z.abs().max()) > 5.0
