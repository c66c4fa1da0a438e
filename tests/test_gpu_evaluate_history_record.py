"""The recorded flights of observation-history policies on the GPU (pds_evaluate_policies_history_record of
include/pds_history_record.h, the record form of evaluate_hist_kernel, csrc/pds_evaluate_hist.h; evaluation.evaluate_population(..., history_fused=True, record=R)): the
launch of tests/test_gpu_evaluate_history.py that also stores x(s), a(s) and the history the actor read, bit for bit what the
composed path -- pds_mlp_forward per policy + pds_step + pds_history_advance, reading the state in front of every step -- gives,
and within the bars of tests/test_gpu_evaluate_forms_reference.py of the independent float64 reference (tests/flight_oracle.py).
The recorded observation is the history tile of the kernel: here it is compared directly, not through the actions it leads to."""
import ctypes as C

import pytest
import torch

import flight_oracle as fo
from test_gpu_evaluate_forms_reference import _fly, _record_tensors, check_metrics, check_record
from test_gpu_evaluate_forms_variants import HISTORY_FLIGHTS, LIMIT, MAX_STEPS, E, _population as _variant_population
from test_gpu_evaluate_history import CASES, HOVER, TAKEOFF, _equal, _make, _pop_for, _population, _snapshot, _unchanged

pytestmark = pytest.mark.gpu
TWO = ["a_hover_h4", "h_takeoff_h8"]  # 68 inputs (a row is no whole number of 64-lane passes) and 192 (the widest)
SENTINEL = 0x5A5A5A5A  # (a float of 1.5e16: nothing a flight holds)


def _bits_differ(a, b):
    return [int((x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)).sum()) for x, y in zip(a, b)]


def _record(env, pop, fused, R, metrics=True, **kw):
    """evaluate_population with a record -> the tensors of _record_tensors and the Flights"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    path = dict(fused=True, history_fused=True) if fused else dict(fused=False)
    out = evaluate_population(env, pop, metrics=metrics, record=R, **path, **kw)
    return _record_tensors(out), out[-1]


@pytest.mark.parametrize("R", [64, 128])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_equals_composed_bit_for_bit(case, R):
    """P = 3, E = 128: two tiles per policy, of which with R = 64 the second does not record.  Return, length, cost, the raw
    metrics, state, action, observation, length and last_action0 of the record launch and of the composed path are equal on the
    bits, in cases that hold both endings; the recorded observation is the whole history"""
    P, E = 3, 128
    pop = _population(case, P)
    env_f, env_c = _make(case, P * E), _make(case, P * E)
    limit, d_in = env_f._max_episode_steps, CASES[case][3]
    fused, fl = _record(env_f, pop, True, R)
    composed, _ = _record(env_c, pop, False, R)
    assert len(fused) == len(composed) == 9
    assert _equal(fused, composed), (case, R, _bits_differ(fused, composed))
    assert tuple(fl.observation.shape) == (P, R, limit, d_in) and d_in == env_f.obs_dim  # H x half columns
    assert tuple(fl.state.shape) == (P, R, limit, 12) and tuple(fl.action.shape) == (P, R, limit, 4)
    length = fused[1]
    assert torch.equal(fl.length, length[:, :R])
    early, cut = int((length < limit).sum()), int((length == limit).sum())
    assert early + cut == P * E and float(length.min()) >= 1
    if CASES[case][0] == TAKEOFF:
        assert early == 0 and cut == P * E  # (no termination on this task)
    else:
        assert early >= 1 and cut >= 1, (early, cut)
    assert env_f.sync_tick() == env_c.sync_tick()
    env_f.close(); env_c.close()


@pytest.mark.parametrize("case", TWO)
def test_without_observations(case):
    """record_observations=False: observation is None, every other tensor the bits of the call that records them"""
    P, E = 3, 128
    pop = _population(case, P)
    env_a, env_b = _make(case, P * E), _make(case, P * E)
    with_obs, _ = _record(env_a, pop, True, 64)
    without, fl = _record(env_b, pop, True, 64, record_observations=False)
    assert fl.observation is None and len(without) == 8
    assert _equal(without, with_obs[:8]), _bits_differ(without, with_obs[:8])
    env_a.close(); env_b.close()


@pytest.mark.parametrize("case", TWO)
def test_the_record_moves_nothing_else(case):
    """return, length, cost and raw metrics of the record launch == those of the metrics launch of the history kernel, on envs of
    the same seed"""
    from phoenix_drone_simulation_amd.evaluation import evaluate_population
    P, E = 3, 128
    pop = _population(case, P)
    env_a, env_b = _make(case, P * E), _make(case, P * E)
    rec, _ = _record(env_a, pop, True, 64)
    m = evaluate_population(env_b, pop, fused=True, history_fused=True, metrics=True)
    want = list(m[:3]) + [m[3].raw]
    assert _equal(rec[:4], want), _bits_differ(rec[:4], want)
    assert env_a.sync_tick() == env_b.sync_tick()
    env_a.close(); env_b.close()


def _abi_record(env, pop, obs, history, T, R, flight, obs_rec, raw=None, out=None, E=None):
    """pds_evaluate_policies_history_record through ctypes; flight / obs_rec: tensors, addresses or None -> (rc, ret, len, cost)"""
    n = env.num_envs
    out = out or [torch.zeros(n, device=env.device) for _ in range(3)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t)
    with torch.cuda.device(env.device):
        rc = env.lib.pds_evaluate_policies_history_record(env._handle, history, pop.P, n // pop.P if E is None else E, C.byref(pop.mlp(0)),
                                                          p(pop.theta), p(pop.mean), p(pop.std), pop.eps, T, p(obs), p(out[0]), p(out[1]),
                                                          p(out[2]), p(raw), R, p(flight), p(obs_rec), env._stream())
    return rc, out[0], out[1], out[2]


@pytest.mark.parametrize("start", [4, 5], ids=["obs_rec_16_byte_aligned", "obs_rec_4_byte_aligned"])
@pytest.mark.parametrize("T", [16, 1], ids=["limit", "one_step"])
def test_nothing_is_written_that_should_not_be(T, start):
    """the ABI with d_flight and d_obs_rec prefilled with a sentinel: P = 2, E = 128, record_per_policy = 64, Hover H = 4.  Every row
    s >= length of a recorded column keeps the sentinel, every row s < length holds none of it and the bits of the
    evaluate_population record of an env of the same seed; the slack behind either buffer, and in front of d_obs_rec, keeps the
    sentinel.  max_steps = 1: the mask of the prologue alone -- every recorded env is written at s = 0.  d_obs_rec on a 16-byte
    boundary, where the 68-float rows are copied in 16-byte pieces, and 4 bytes behind one, where they are copied dword by dword
    (what the ABI asks of d_obs_rec is 4-byte alignment): the same bits"""
    from phoenix_drone_simulation_amd import native
    case, P, E, R, HS, SLACK = "a_hover_h4", 2, 128, 64, 68, 64
    pop = _population(case, P)
    env = _make(case, P * E)
    dev = env.device
    flight = torch.full((T * 4 * P * R * 4 + SLACK,), SENTINEL, dtype=torch.int32, device=dev)
    obs_buf = torch.full((start + T * P * R * HS + SLACK,), SENTINEL, dtype=torch.int32, device=dev)
    obs_rec = obs_buf[start:]
    assert obs_buf.data_ptr() % 16 == 0 and (obs_rec.data_ptr() % 16 == 0) == (start % 4 == 0)
    raw = torch.zeros(P * E, 8, device=dev)
    obs, _ = env.reset()
    rc, ret, length, cost = _abi_record(env, pop.to(dev), obs.contiguous(), 4, T, R, flight, obs_rec, raw=raw)
    assert rc == native.OK, env.lib.pds_last_error(env._handle)
    torch.cuda.synchronize()
    env.close()
    env2 = _make(case, P * E)
    want, fl = _record(env2, pop, True, R, max_steps=T)
    env2.close()
    got = [x.cpu().reshape(P, E) for x in (ret, length, cost)] + [raw.cpu().reshape(P, E, 8)]
    assert _equal(got, want[:4]), _bits_differ(got, want[:4])
    assert bool((flight[-SLACK:] == SENTINEL).all()) and bool((obs_rec[-SLACK:] == SENTINEL).all()) and bool((obs_buf[:start] == SENTINEL).all())
    rows = flight[:-SLACK].cpu().reshape(T, 4, P * R, 4).permute(2, 0, 1, 3).reshape(P, R, T, 16)  # [column, step, piece, 4]
    hist = obs_rec[:-SLACK].cpu().reshape(T, P * R, HS).permute(1, 0, 2).reshape(P, R, T, HS)
    L = got[1][:, :R]
    on = (torch.arange(T).view(1, 1, T) < L.unsqueeze(-1)).unsqueeze(-1)
    assert float(L.min()) >= 1
    if T == 1:
        assert bool(on.all())
    else:
        assert int((L < T).sum()) >= 1 and int((L == T).sum()) >= 1
    for name, x, ref in (("flight", rows, torch.cat([fl.state, fl.action], dim=-1)), ("observation", hist, fl.observation)):
        kept = x == SENTINEL
        assert bool(kept[(~on).expand_as(kept)].all()), name          # past the end: as the caller left it
        assert not bool(kept[on.expand_as(kept)].any()), name         # below it: written
        ref = ref.contiguous().view(torch.int32)
        assert torch.equal(torch.where(on, x, torch.zeros_like(x)), ref), name


def test_the_sweep_has_104_flights():
    assert len(HISTORY_FLIGHTS) == 104 and len({f[0] for f in HISTORY_FLIGHTS}) == 104


@pytest.mark.parametrize("fid,env_id,kw,H,width", HISTORY_FLIGHTS, ids=[f[0] for f in HISTORY_FLIGHTS])
def test_every_history_configuration_records_what_the_composed_path_records(fid, env_id, kw, H, width):
    """every code object of the record form once: all 26 configurations at one H per input width class, P = 3, E = 64, record = 64,
    metrics=True, the one-launch path equal to the composed path on the bits"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.evaluation import fused_history_evaluation_built
    P = 3
    make = lambda: pds.make(env_id, num_envs=P * E, seed=17, max_episode_steps=LIMIT, observation_history_size=H, **kw)
    env_f, env_c = make(), make()
    assert env_f.obs_dim <= width and fused_history_evaluation_built(env_f)
    pop = _variant_population(env_f, P, seed=H)
    fused, fl = _record(env_f, pop, True, 64, max_steps=MAX_STEPS)
    composed, _ = _record(env_c, pop, False, 64, max_steps=MAX_STEPS)
    assert _equal(fused, composed), (fid, _bits_differ(fused, composed))
    assert tuple(fl.observation.shape) == (P, 64, MAX_STEPS, env_f.obs_dim)
    length = fused[1]
    assert float(length.min()) >= 1 and float(length.max()) <= LIMIT and int((length == LIMIT).sum()) >= 1
    assert env_f.sync_tick() == env_c.sync_tick() == 1 + MAX_STEPS
    env_f.close(); env_c.close()


@pytest.mark.parametrize("whole", [False, True], ids=["record64", "recordE"])
@pytest.mark.parametrize("name", fo.HISTORY_CASES)
def test_the_record_against_the_float64_reference(name, whole):
    """one case per input width class (68, 60, 126 and 192 inputs), record = 64 and record = E: return, length and cost by the rule
    of tests/test_gpu_evaluate_reference.py check(); metrics, state, action and the recorded HISTORY -- the float64 stack of
    tests/flight_oracle.py -- by the rule of tests/test_gpu_evaluate_forms_reference.py: within BAR_UNITS = 4 units of
    flight_oracle.units_of, the bar of the composed history record there and for its reason (the device's FMA contraction and its
    own sincos sit about as far from libm float32 as that from float64); at most evaluate_oracle.length_cap(N) envs left out.
    No bar is set from the device's output.  The MARGIN lines: profiles/evaluate_history_record_parity_margins.txt keeps a run."""
    from test_gpu_evaluate_reference import check
    case = fo.history_case(name)
    assert case.shape[0] == fo.HISTORY_INPUTS[name]
    R = case.E if whole else 64
    path = "fused_history"
    out = _fly(case, True, history_fused=True, metrics=True, record=R)
    assert len(out) == 5
    check(case, out[:3], f"{path}.record{R}")
    check_metrics(case, path, f"record{R}", out[3], out[1])
    check_record(case, path, out[4], R, True)
    assert tuple(out[4].observation.shape) == (case.P, R, case.max_steps, case.history * case.half)


def test_abi_refusals_leave_the_handle_as_it_was():
    """PDS_EINVAL for a record_per_policy of 0, 63 and E + 64, a NULL d_flight, a d_flight misaligned by 4 bytes and a d_obs_rec
    misaligned by 2; PDS_EUNSUPPORTED for a handle without auto_reset, a ground-effect env and history x half > 192; nothing
    moves and nothing is written.  After a successful call the env refuses to step until reset()"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd import native
    T, n, E_, HS = 10, 128, 64, 68

    def buffers(dev):
        return torch.zeros(T * 4 * n * 4 + 4, device=dev), torch.zeros(T * n * HS + 4, device=dev), torch.zeros(n, 8, device=dev)

    for kw in (dict(auto_reset=False), dict(use_ground_effect=True)):
        env = pds.make(HOVER, num_envs=n, seed=3, observation_history_size=4, **kw)
        obs, _ = env.reset()
        pop = _pop_for(env).to(env.device)
        flight, obs_rec, raw = buffers(env.device)
        snap = _snapshot(env)
        assert env.lib.pds_evaluate_history_supported(env._handle, 4) == 0
        assert _abi_record(env, pop, obs, 4, T, 64, flight, obs_rec, raw=raw)[0] == native.EUNSUPPORTED, kw
        assert len(env.lib.pds_last_error(env._handle)) > 0
        _unchanged(env, snap)
        assert float(flight.abs().max()) == 0.0 and float(obs_rec.abs().max()) == 0.0
        env.close()

    env = pds.make(HOVER, num_envs=n, seed=3, max_episode_steps=T, observation_history_size=4)
    assert env.obs_dim == HS and env.lib.pds_evaluate_history_supported(env._handle, 4) == 1
    obs, _ = env.reset()
    pop = _pop_for(env).to(env.device)
    flight, obs_rec, raw = buffers(env.device)
    out = [torch.zeros(n, device=env.device) for _ in range(3)]
    snap = _snapshot(env)
    assert flight.data_ptr() % 16 == 0 and obs_rec.data_ptr() % 4 == 0
    calls = dict(r0=lambda: _abi_record(env, pop, obs, 4, T, 0, flight, obs_rec, raw, out),
                 r63=lambda: _abi_record(env, pop, obs, 4, T, 63, flight, obs_rec, raw, out),
                 r_e_plus_64=lambda: _abi_record(env, pop, obs, 4, T, E_ + 64, flight, obs_rec, raw, out),
                 flight_null=lambda: _abi_record(env, pop, obs, 4, T, 64, None, obs_rec, raw, out),
                 flight_align=lambda: _abi_record(env, pop, obs, 4, T, 64, flight.data_ptr() + 4, obs_rec, raw, out),
                 obs_rec_align=lambda: _abi_record(env, pop, obs, 4, T, 64, flight, obs_rec.data_ptr() + 2, raw, out))
    for name, call in calls.items():
        assert call()[0] == native.EINVAL and len(env.lib.pds_last_error(env._handle)) > 0, name
        _unchanged(env, snap)
    assert _abi_record(env, pop, obs, 12, T, 64, flight, obs_rec, raw, out)[0] == native.EUNSUPPORTED  # 12 x 17 = 204 inputs
    _unchanged(env, snap)
    for buf in (flight, obs_rec, raw, *out):
        assert float(buf.abs().max()) == 0.0  # nothing was written
    zero = torch.zeros(n, 4, device=env.device)
    env.step(zero)  # still a reset handle
    obs, _ = env.reset()
    assert _abi_record(env, pop, obs, 4, T, 64, flight, None, None, out)[0] == native.OK  # without metrics and observations
    torch.cuda.synchronize()
    assert float(out[1].min()) >= 1 and float(raw.abs().max()) == 0.0 and float(obs_rec.abs().max()) == 0.0
    rows = flight[:T * 4 * n * 4].reshape(T, 4, n, 4)
    assert float(rows[0, 0, :, 2].min()) > 0 and float(flight[T * 4 * n * 4:].abs().max()) == 0.0  # z(0) of every env; nothing behind the end
    with pytest.raises(ValueError, match="before pds_reset"):
        env.step(zero)
    env.reset()
    env.step(zero)  # the env steps on after a reset()
    env.close()
