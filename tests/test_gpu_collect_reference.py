"""pds_collect (csrc/pds_collect.h) and the composed per-step path (pds_mlp_forward, pds_ddpg_explore / pds_sac_sample, pds_step
and the torch bookkeeping of OffPolicyTrainer.step_env / learn_one_epoch) against an INDEPENDENT reference:
tests/collect_oracle.py -- the float64 CPU oracle behind a numpy float64 MLP and the numpy noise contract, the collection loop
restated from the reference's text.  tests/test_gpu_collect.py compares the two device paths with each other; both were written
together and could be wrong together (obs2 = the `final_obs` row where the env finished, done = terminated & ~truncated, the
noise of step s = call first_call + s for sample id = env row, the running sums zeroed after the accumulators read them, the
eight tile statistics).  Here each of those fails.

The rule (one statement, collect_oracle.check):
  agreement  an env agrees when its `done` column and its finished flags (obs2 differs from the next o exactly where the env
             finished) equal the reference's at every step; at most max(1, N // 1000) envs may not -- counted, printed, their
             rows left out, their tile left out of the slab comparison.
  exact      done and the finished flags through the agreement itself (the cap is what binds them); on the agreeing envs
             ep_len, the slab's count, length sum, min and max; ptr and size; the fill in every ring row no step reached.
  float      each array within 4 UNITS.  The unit is measured, not chosen: the float32 reference's own max distance from the
             float64 reference on the same case and array (tests/test_collect_oracle_cpu.py prints it), floored at one float32
             rounding of the array's largest entry.  The action columns' tolerance is floored at the elementwise bars the project
             already holds the two exploration rules to (test_ddpg_explore_against_float64, _check_sample): the reference draws
             its z in float64 and does not contain the device's Box-Muller error.  4 is the project's margin for a device path
             against float64.  Return sum and sum of squares of a tile: 1e-5 relative.
Each comparison prints `MARGIN <case> <path> <array> unit=... ratio=... excluded=...` and records the ratio as a test property;
profiles/collect_parity_margins.txt keeps a run."""
import numpy as np
import pytest
import torch

import collect_oracle as co

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _env(c):
    import phoenix_drone_simulation_amd as pds
    env = pds.make(c.env_id, num_envs=c.N, device=DEV, seed=c.env_seed, max_episode_steps=c.limit, **c.kwargs)
    assert env.obs_dim == c.D
    return env


def _fm(c):
    """the case's actor as a FusedMLP"""
    from phoenix_drone_simulation_amd.fused import FusedMLP
    from phoenix_drone_simulation_amd.ppo import _mlp
    d_out = 8 if c.mode == co.SAC else 4
    net = _mlp([c.D, c.hidden[0], c.hidden[1], d_out], c.activation).to(DEV)
    with torch.no_grad():
        for lin, w, b in zip((net[0], net[2], net[4]), c.actor[0::2], c.actor[1::2]):
            lin.weight.copy_(torch.from_numpy(w)); lin.bias.copy_(torch.from_numpy(b))
    return FusedMLP(net, c.activation)


def _run(c, fused):
    """the case's launches on a fresh env, through pds_collect (fused) or the per-step path -> the dict collect_oracle.check reads"""
    from test_gpu_collect import _composed, _fused, _ring
    env, fm = _env(c), _fm(c)
    buf = _ring(c.N, c.D, c.capacity // c.N, c.fill)
    buf.ptr = c.ptr
    log_std = torch.tensor(c.log_std, dtype=torch.float32, device=DEV)
    state, slabs, call = None, [], c.first_call
    for k in c.launches:
        kw = dict(first_call=call, log_std=log_std, act_limit=c.act_limit, seed=c.noise_seed, state=state)
        if fused:
            obs, ep_ret, ep_len, slab = _fused(env, fm, c.mode, k, buf, **kw)
            slabs.append(slab.double().cpu().numpy())
        else:
            obs, ep_ret, ep_len, steps = _composed(env, fm, c.mode, k, buf, **kw)
            slabs.append(_slab_of(c, steps))
        state, call = (obs, ep_ret, ep_len), call + k
    assert env.tick == env.sync_tick() == 1 + c.K
    env.close()
    f64 = lambda t: t.double().cpu().numpy()
    return dict(oa=f64(buf.oa), obs2=f64(buf.obs2), rew=f64(buf.rew), done=f64(buf.done), obs=f64(state[0]), ep_ret=f64(state[1]),
                ep_len=f64(state[2]), slabs=slabs, ptr=buf.ptr, size=buf.size)


def _slab_of(c, steps):
    """learn_one_epoch's eight accumulators per 64-env tile from the composed run's per-step data (float32 sums, as torch adds)"""
    out = np.tile(np.asarray(co.NEUTRAL), (c.tiles, 1))
    for t in range(c.tiles):
        rows = slice(co.TILE * t, co.TILE * (t + 1))
        acc = torch.tensor(co.NEUTRAL, dtype=torch.float32, device=DEV)
        for dn, _, _, ret, ln in steps:
            dn, ret, ln = dn[rows], ret[rows], ln[rows]
            if not bool(dn.any()):
                continue
            r, l = ret[dn], ln[dn]
            acc[0] += dn.sum(); acc[1] += r.sum(); acc[2] += (r * r).sum()
            acc[3], acc[4] = torch.minimum(acc[3], r.min()), torch.maximum(acc[4], r.max())
            acc[5] += l.sum(); acc[6], acc[7] = torch.minimum(acc[6], l.min()), torch.maximum(acc[7], l.max())
        out[t] = acc.double().cpu().numpy()
    return out


@pytest.mark.parametrize("name", co.CASES)
def test_collection_against_the_float64_reference(name, record_property):
    """Every case of tests/collect_oracle.py (its table says what each is for): the kernel and the composed path, each against
    the float64 reference, and bit for bit against each other."""
    c = co.case(name)
    fused, composed = _run(c, True), _run(c, False)
    co.check(c, fused, "fused", record_property)
    co.check(c, composed, "composed", record_property)
    for k in ("oa", "obs2", "rew", "done", "obs", "ep_ret", "ep_len"):
        assert np.array_equal(fused[k], composed[k]), (name, k, int((fused[k] != composed[k]).sum()))
    assert (fused["ptr"], fused["size"]) == (composed["ptr"], composed["size"])
    if c.N == 67:  # the case means whole pieces that are not 16-byte aligned: the blocks of odd s
        assert (c.block(1) * (c.D + 4) * 4) % 16 == 8 and (c.block(1) * c.D * 4) % 16 == 8
