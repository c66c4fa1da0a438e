"""CPU-side tests of the host logic: the C-ABI library loads and exports every symbol that
include/pds.h declares (no compute without a GPU), the ctypes mirror of pds_config matches the C
struct, the env ids / kwargs mirror the reference, the product path refuses to run without the
HIP device, and the multi-GPU sharding helpers work under a world_size-2 gloo group."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "pds.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(pds_[a-z_0-9]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    import phoenix_drone_simulation_amd as pds
    lib = pds.native.load()
    syms = _declared_symbols()
    assert len(syms) >= 15
    for s in syms:
        assert hasattr(lib, s), f"libpds_hip.so does not export {s}"
    assert set(pds.native.EXPORTS) == set(syms)
    assert lib.pds_version() == 2


def _header():
    hdr = open(os.path.join(ROOT, "include", "pds.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))


def _c_class(decl, native):
    """The ctypes class of one C parameter / return type / field declaration (with or without its name)."""
    if "*" in decl or "[" in decl:
        if re.match(r"\s*const\s+char\s*\*\s*$", decl):
            return C.c_char_p
        for struct, cls in (("pds_mlp", native.Mlp), ("pds_adam", native.Adam), ("pds_config", native.Config)):
            if re.search(rf"\b{struct}\b", decl):
                return C.POINTER(cls)
        return C.c_void_p
    scalars = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
               "float": C.c_float, "double": C.c_double}
    words = [w for w in decl.split() if w != "const"]
    assert words and words[0] in scalars, decl
    return scalars[words[0]]


def _table_mismatches(signatures, native):
    """Every disagreement between `signatures` and the prototypes of include/pds.h: names, arity, return and parameter classes."""
    protos = re.findall(r"^[ \t]*((?:const\s+)?\w+[\s\*]+)(pds_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M)
    bad = [f"names: {sorted(set(signatures) ^ {name for _, name, _ in protos})}"] if set(signatures) != {n for _, n, _ in protos} else []
    for ret, name, params in protos:
        if name not in signatures:
            continue
        restype, argtypes = signatures[name]
        want = [] if params.strip() in ("", "void") else [_c_class(p, native) for p in params.split(",")]
        if restype is not _c_class(ret, native):
            bad.append(f"{name}: restype {restype} for `{ret.strip()}`")
        if len(argtypes) != len(want):
            bad.append(f"{name}: {len(argtypes)} argtypes for {len(want)} parameters")
        bad += [f"{name}: argument {i} is {a}, the header says {w}" for i, (a, w) in enumerate(zip(argtypes, want)) if a is not w]
    return len(protos), bad


def test_signature_table_matches_the_header():
    """native.SIGNATURES against every `ret pds_name(params);` of include/pds.h: the same names, and per entry point the arity, the
    return type and the class of every parameter (a wrong row would hand a kernel a truncated pointer, not fail a call); the
    ctypes mirrors of pds_mlp / pds_adam field by field.  A table that lost one argument must not pass."""
    from phoenix_drone_simulation_amd import native
    n, bad = _table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) == 73 and not bad, bad
    assert native.EXPORTS == list(native.SIGNATURES) and native.SIGNATURES["pds_version"] == (C.c_int, [])
    restype, argtypes = native.SIGNATURES["pds_mlp_forward"]
    _, bad = _table_mismatches(dict(native.SIGNATURES, pds_mlp_forward=(restype, argtypes[:-1])), native)
    assert bad == ["pds_mlp_forward: 8 argtypes for 9 parameters"]
    _, bad = _table_mismatches(dict(native.SIGNATURES, pds_tick=(C.c_int, [C.c_void_p])), native)
    assert len(bad) == 1 and "pds_tick: restype" in bad[0]
    for struct, cls in (("pds_mlp", native.Mlp), ("pds_adam", native.Adam)):
        body = re.search(rf"typedef\s+struct\s+{struct}\s*\{{(.*?)\}}\s*{struct}\s*;", _header(), flags=re.S).group(1)
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, first = re.match(r"((?:const\s+)?\w+)\s*(.*)", decl, flags=re.S).groups()
            for d in first.split(","):
                fields.append((d.replace("*", "").strip(), _c_class(f"{base} {d}", native)))
        assert fields == [(name, t) for name, t in cls._fields_], struct


class _StubLib:
    """Stands in for the loaded library: entry points that return a chosen code and record what they were given."""

    def __init__(self, rc):
        self.rc, self.got = rc, None

    def pds_reset(self, *args):
        self.got = args
        return self.rc

    def pds_last_error(self, handle):
        return b"the stub refuses"


def test_call_maps_return_codes_and_converts_arguments(monkeypatch):
    """native.call without a device (on=None) against a stub library: 0 returns; without a handle PDS_EUNSUPPORTED is
    NotImplementedError and any other code RuntimeError naming the entry point and the code; with a handle native.check's classes
    with the handle's last-error text.  A tensor arrives as its data_ptr(), None as None, an object that carries a pds_mlp is
    re-bound and arrives by reference, everything else as it is."""
    from phoenix_drone_simulation_amd import native

    class Tensorish:
        def data_ptr(self):
            return 0x7F0012345600

    class Carrier:
        def __init__(self):
            self.m, self.bound = native.Mlp(d_in=7), 0

        def _bind(self):
            self.bound += 1

    stub, net = _StubLib(0), Carrier()
    monkeypatch.setattr(native, "_lib", stub)
    assert native.call("pds_reset", Tensorish(), None, 3, 0.5, net) is None
    ptr, none, three, half, ref = stub.got
    assert (ptr, none, three, half) == (0x7F0012345600, None, 3, 0.5) and net.bound == 1
    assert C.cast(ref, C.POINTER(native.Mlp)).contents.d_in == 7 and C.addressof(ref._obj) == C.addressof(net.m)
    for rc, exc in ((native.EINVAL, RuntimeError), (native.EHIP, RuntimeError), (native.EUNSUPPORTED, NotImplementedError)):
        stub.rc = rc
        with pytest.raises(exc, match=rf"pds_reset -> {rc}$") as e:
            native.call("pds_reset", None)
        assert type(e.value) is exc
    for rc, exc in ((native.EINVAL, ValueError), (native.EUNSUPPORTED, NotImplementedError), (native.ENOMEM, MemoryError),
                    (native.EHIP, RuntimeError)):
        stub.rc = rc
        with pytest.raises(exc, match=rf"pds_reset failed \({rc}\): the stub refuses$") as e:
            native.call("pds_reset", None, handle=C.c_void_p(1))
        assert type(e.value) is exc


def test_config_struct_mirror_and_defaults():
    """pds_default_config reproduces the reference ctor defaults (envs/base.py:26-48,
    envs/hover.py:7-45, envs/circle.py:7-34, envs/takeoff.py:13-41)."""
    import phoenix_drone_simulation_amd as pds
    for task, spin, vel, arp, z0 in ((0, 1e-4, 0.0, 0.0, 1.0), (1, 1e-3, 1e-4, 1e-3, 1.0),
                                     (2, 1e-4, 0.0, 0.0, float(np.float32(0.0125)))):
        c = pds.native.default_config(task)
        assert c.struct_size == C.sizeof(pds.native.Config)
        assert (c.task, c.num_envs, c.aggregate_phy_steps, c.max_episode_steps) == (task, 1, 1, 500)
        assert (c.observation_noise, c.enable_reset_distribution, c.auto_reset) == (1, 1, 1)
        assert c.domain_randomization == 0.10 and c.motor_thrust_noise == 0.05
        assert c.time_step == 0.01 and c.motor_time_constant == 0.08
        assert (c.penalty_action, c.penalty_angle, c.penalty_terminal) == (1e-4, 0.0, 100.0)
        assert (c.penalty_spin, c.penalty_velocity, c.ARP) == (spin, vel, arp)
        assert list(c.target_pos) == [0.0, 0.0, 1.0] and list(c.init_xyz) == [0.0, 0.0, z0]
    assert pds.native.load().pds_default_config(7, C.byref(pds.native.Config())) == pds.native.EINVAL


def test_field_widths():
    import phoenix_drone_simulation_amd as pds
    lib = pds.native.load()
    want = dict(pos=3, rpy=3, vel=3, omega=3, quat=4, motor_x=4, last_action=4, prev_action=4,
                step_count=1, quat_sign=1, ref_offset=1, params=6, motor_A=4, motor_K=4, ou=4, noisy_obs=10, pid=12,
                gyro_bias=3, gyro_lpf=3)
    for name, w in want.items():
        assert lib.pds_field_width(pds.native.FIELDS[name]) == w
    assert lib.pds_field_width(99) == pds.native.EINVAL


def test_registry_mirrors_reference_ids():
    import phoenix_drone_simulation_amd as pds
    assert sorted(pds.registry) == ["DroneCircleSimpleEnv-v0", "DroneHoverSimpleEnv-v0",
                                    "DroneTakeOffSimpleEnv-v0"]
    assert all(v[1] == 500 for v in pds.registry.values())  # __init__.py:11,27,43
    with pytest.raises(KeyError):
        pds.make("DroneHoverBulletEnv-v0")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_no_silent_cpu_fallback():
    """Without a HIP device the product path must fail loudly, at the Python and at the C level."""
    import phoenix_drone_simulation_amd as pds
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pds.make("DroneHoverSimpleEnv-v0", num_envs=8)
    cfg = pds.native.default_config(0)
    cfg.observation_noise = 0
    cfg.motor_thrust_noise = 0.0
    h = C.c_void_p()
    rc = pds.native.load().pds_create(C.byref(cfg), C.byref(h))
    assert rc == pds.native.ENODEVICE and not h
    assert b"no CPU fallback" in pds.native.load().pds_last_error(None)


_BAD_CONFIGS = [
    # (task, overrides, expected code, fragment of pds_last_error)
    (0, dict(struct_size=8), "EINVAL", b"size mismatch"),
    (0, dict(num_envs=0), "EINVAL", b"invalid pds_config"),
    (0, dict(max_episode_steps=70000), "EINVAL", b"invalid pds_config"),
    (0, dict(num_envs=(1 << 30) + 1), "EINVAL", b"2^30"),
    (0, dict(env_id_base=-1), "EINVAL", b"global env id range"),
    (0, dict(env_id_base=(1 << 32) - 4, num_envs=8), "EINVAL", b"global env id range"),
    (0, dict(device=-1), "EINVAL", b"negative"),
    (0, dict(control_mode=3), "EINVAL", b"control_mode"),
    (2, dict(control_mode=1), "EUNSUPPORTED", b"PID modes"),
    (0, dict(observation_frequency=0), "EINVAL", b"observation_frequency"),
    (1, dict(observation_frequency=101), "EUNSUPPORTED", b"reference points"),
    (0, dict(observation_frequency=200), "EINVAL", b"obs_rate 0"),       # base.py:108 would divide by 0
    # (round 4: the Kalman-hold branch with latency / a PID mode is built; round 5: the ground-effect extension under a PID
    #  mode too -- what remains refused is that pair together with the hold or the latency ring)
    (0, dict(observation_frequency=50, control_mode=1, use_ground_effect=1), "EUNSUPPORTED", b"ground"),
    (0, dict(use_latency=1, latency=0.10), "EUNSUPPORTED", b"latency"),  # 10 rows > PDS_MAX_LATENCY_STEPS
    (0, dict(use_latency=1, use_ground_effect=1, control_mode=1), "EUNSUPPORTED", b"ground"),  # (latency + ground effect: PWM only)
]


@pytest.mark.parametrize("task,over,code,frag", _BAD_CONFIGS)
def test_create_validates_the_config_before_touching_a_device(task, over, code, frag):
    """pds_create rejects what the kernels are not built for (or what the reference itself would
    crash on) with a code and a message; the checks run before any HIP call, so they hold on a
    machine without a GPU as well."""
    import phoenix_drone_simulation_amd as pds
    lib = pds.native.load()
    cfg = pds.native.default_config(task)
    for k, v in over.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = lib.pds_create(C.byref(cfg), C.byref(h))
    assert rc == getattr(pds.native, code) and not h, (rc, lib.pds_last_error(None))
    assert frag in lib.pds_last_error(None), lib.pds_last_error(None)


def test_no_hot_kernel_keeps_a_local_object_in_scratch_memory():
    """Private (scratch) memory beyond the register spills means a local struct was forced into memory
    (a pointer select or a dynamic index): the latency variants ran at half speed for that in round 2.
    Read from the code-object metadata of the shipped library (profiles/tools/kernel_resources.py)."""
    sys.path.insert(0, os.path.join(ROOT, "profiles", "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    if not os.path.exists(kr.READELF):
        pytest.skip("llvm-readelf not found")
    rows = kr.kernel_table()
    hot = [r for r in rows if "step_kernel" in r[0] or "step_k_kernel" in r[0]]
    assert len(hot) > 100
    bad = [r for r in hot if kr.forced_scratch(r)]
    assert not bad, bad[:5]
    # the four headline-family kernels (Hover, full and half tile) stay within 4 waves per SIMD, spill-free or nearly
    lean = [r for r in hot if "step_kernel<pds::Variant<0, false, false, false, false, false, 0, false, false>" in r[0]]
    assert len(lean) == 2 and all(r[1] <= 128 and r[2] <= 8 for r in lean), lean


def test_product_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pkg = os.path.join(ROOT, "phoenix-drone-simulation_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "phoenix_oracle" not in txt or f.endswith((".hip", ".h")) and "oracle/phoenix_oracle" in txt, f
                assert "from oracle" not in txt and "import oracle" not in txt, f
    out = subprocess.run(["nm", "-D", os.path.join(pkg, "libpds_hip.so")], capture_output=True, text=True).stdout
    assert not [l for l in out.splitlines() if l.split()[-1].startswith("po_")]  # no oracle symbols


def test_shard_range_partitions_exactly():
    from phoenix_drone_simulation_amd import shard_range
    for total, world in ((8388608, 8), (1000, 3), (7, 8), (1, 1)):
        spans = [shard_range(total, r, world) for r in range(world)]
        assert spans[0][0] == 0 and spans[-1][1] == total
        assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_range(10, 2, 2)


_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
import phoenix_drone_simulation_amd as pds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
total, D = {total}, 42
a, b = pds.shard_range(total, rank, world)
# each rank "observes" its global env ids; gathered tensor must be ordered by global env id
obs = (torch.arange(a, b, dtype=torch.float32)[:, None] * 100 + torch.arange(D, dtype=torch.float32)[None])
full = pds.all_gather_obs(obs)
want = (torch.arange(total, dtype=torch.float32)[:, None] * 100 + torch.arange(D, dtype=torch.float32)[None])
assert full.shape == (total, D) and torch.equal(full, want), rank
full2 = pds.all_gather_obs(obs)  # shard sizes come from the cache now: no size exchange on the second call
assert torch.equal(full2, want)
# the peer-to-peer STORE variant (SURVEY 8e): same result, ordered by global env id, over several steps
# NO barrier between the calls: the result of call s is valid until this rank's call s+1 (two buffers
# alternate, a peer writes buffer j again only after the barrier inside my NEXT call); rank 1 is a slow
# consumer, rank 0 runs ahead as far as the protocol lets it
import time
gat = pds.P2PObsGather(b - a, D, "cpu")
prev = None
for step in range(7):
    got = gat.gather(obs + step)
    assert prev is None or prev.data_ptr() != got.data_ptr()
    if rank == 1:
        time.sleep(0.05)
    assert got.shape == (total, D) and torch.equal(got, want + step), (rank, step)
    assert gat.out.data_ptr() == got.data_ptr()
    prev = got
gat.release()
from phoenix_drone_simulation_amd.sharding import max_over_ranks
assert max_over_ranks(float(rank + 1), torch.device("cpu")) == float(world)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("total", [64, 65])
def test_all_gather_obs_world2_gloo(total, tmp_path):
    """N>1 path on CPU: 2 processes, gloo, equal and ragged shards."""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, total=total))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + total), WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate(timeout=120)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} ok" in o


_WORKER8 = r"""
import os, sys, time, torch, torch.distributed as dist
sys.path.insert(0, {root!r})
import phoenix_drone_simulation_amd as pds
from phoenix_drone_simulation_amd.ppo import avg_grads, OnlineMeanStd, ActorCritic
from phoenix_drone_simulation_amd.sharding import max_over_ranks
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
total, D = {total}, 34
a, b = pds.shard_range(total, rank, world)
assert b - a in (total // world, total // world + 1)
row = lambda lo, hi: torch.arange(lo, hi, dtype=torch.float32)[:, None] * 100 + torch.arange(D, dtype=torch.float32)[None]
obs, want = row(a, b), row(0, total)
for _ in range(2):  # (second call: shard sizes from the cache)
    full = pds.all_gather_obs(obs)
    assert full.shape == (total, D) and torch.equal(full, want), rank
gat = pds.P2PObsGather(b - a, D, "cpu", tag="pds_p2p_w8")
for step in range(5):
    got = gat.gather(obs + step)
    if rank in (3, 6):
        time.sleep(0.02)  # slow consumers
    assert torch.equal(got, want + step), (rank, step)
gat.release()
# gradient average: ONE flattened all-reduce == the reference's per-parameter mpi_avg_grads (utils/mpi_tools.py:30-36)
torch.manual_seed(0)
ac = ActorCritic(D, 4)
for i, p in enumerate(ac.pi.net.parameters()):
    p.grad = torch.full_like(p, float(rank + 1) * (i + 1))
avg_grads(ac.pi.net)
for i, p in enumerate(ac.pi.net.parameters()):
    assert torch.allclose(p.grad, torch.full_like(p, (world + 1) / 2 * (i + 1))), (rank, i)
# running statistics: 8 equal batches == one update on the concatenated batch (utils/online_mean_std.py:60-95), twice
torch.manual_seed(1)
data = [torch.randn(world * 16, D) * 3 + 1, torch.randn(world * 16, D) * 0.5 - 2]
oms, ref = OnlineMeanStd(shape=(D,)), OnlineMeanStd(shape=(D,))
for x in data:
    oms.update(x[rank * 16:(rank + 1) * 16])
assert max_over_ranks(float(rank), torch.device("cpu")) == float(world - 1)
dist.barrier()
dist.destroy_process_group()
for x in data:
    ref.update(x)
assert torch.allclose(oms.mean, ref.mean, atol=1e-5) and torch.allclose(oms.std, ref.std, atol=1e-4), rank
assert float(oms.count) == 2 * world * 16
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("total", [8 * 13 + 5, 8 * 16])
def test_world8_gloo_ragged_and_equal_shards(total, tmp_path):
    """Everything multi-rank at the node's real world size (8 ranks, one per MI355X): shard_range,
    all_gather_obs (ragged: pad + strip; equal: all_gather_into_tensor), the peer-to-peer store gather with slow consumers,
    the flattened gradient average, the all-reduced running statistics, max_over_ranks -- over gloo on CPU tensors."""
    script = tmp_path / "worker8.py"
    script.write_text(_WORKER8.format(root=ROOT, total=total))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29700 + total % 97), WORLD_SIZE="8", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(8)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert f"rank {r} ok" in o
