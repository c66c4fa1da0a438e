"""The host side of the fused collection under the PID control modes and the latency ring (no GPU): the two symbols' rows in
native.COLLECT_CONTROL_SIGNATURES against their declarations in include/pds_collect_control.h (include/pds.h and native.SIGNATURES
are pinned entry for entry by tests/test_host_cpu.py, so the entry points stand beside them), the library's exports, the trainers'
opt-in keyword, ddpg.collect_steps, and the translation units in build._UNITS."""
import glob
import inspect
import os
import re

import pytest

QUERY, NAME = "pds_collect_control_supported", "pds_collect_control"


def test_the_table_matches_the_header_and_the_library_exports_the_symbols(monkeypatch):
    """the rows against include/pds_collect_control.h by the comparison of tests/test_host_cpu.py (its _table_mismatches, reading
    this header); they are the rows of pds_collect_supported / pds_collect; include/pds.h does not name them; the library exports
    them, `load` binds them and they refuse a NULL handle"""
    import test_host_cpu as th
    from phoenix_drone_simulation_amd import native
    table = native.COLLECT_CONTROL_SIGNATURES
    assert list(table) == [QUERY, NAME] and not set(table) & set(native.SIGNATURES)
    n, bad = th._table_mismatches(native.SIGNATURES, native)
    assert n == len(native.SIGNATURES) and not bad, bad
    pds_h = th._header()
    assert QUERY not in pds_h and NAME not in pds_h

    def header():
        text = open(os.path.join(th.ROOT, "include", "pds_collect_control.h")).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))

    monkeypatch.setattr(th, "_header", header)
    n, bad = th._table_mismatches(table, native)
    assert n == 2 and not bad, bad
    restype, argtypes = table[NAME]
    assert (restype, argtypes) == native.SIGNATURES["pds_collect"] and len(argtypes) == 19
    assert table[QUERY] == native.SIGNATURES["pds_collect_supported"]
    _, bad = th._table_mismatches(dict(table, **{NAME: (restype, argtypes[:-1])}), native)
    assert bad == [f"{NAME}: 18 argtypes for 19 parameters"]
    lib = native.load()
    for name in (QUERY, NAME):
        assert hasattr(lib, name), f"libpds_hip.so does not export {name}"
    fn = getattr(lib, NAME)
    assert fn.argtypes == argtypes and fn.restype is restype
    assert fn(None, 1, 0, None, 1.0, None, 0, 0, None, None, None, None, 64, 0, None, None, None, None, None) == native.EINVAL
    assert getattr(lib, QUERY)(None, None, 0) == native.EINVAL


def test_control_fused_is_opt_in():
    from phoenix_drone_simulation_amd.ddpg import DDPGTrainer, OffPolicyTrainer
    from phoenix_drone_simulation_amd.sac import SACTrainer
    for cls in (DDPGTrainer, SACTrainer):
        ps = inspect.signature(cls.__init__).parameters
        assert ps["control_fused"].default is False and ps["fused_collect"].default is False
        assert list(ps)[-1] == "control_fused"
    assert OffPolicyTrainer.control_fused is False and OffPolicyTrainer.collect_fused is False and OffPolicyTrainer.fused_collect is False
    from phoenix_drone_simulation_amd import fused
    assert inspect.signature(fused.fused_collect).parameters["control"].default is False
    assert callable(fused.collect_control_supported)


@pytest.mark.parametrize("since,every,N,left,want", [(0, 50, 256, 8, 1), (0, 1000, 256, 8, 4), (512, 1000, 256, 8, 2), (0, 1000, 256, 3, 3),
                                                      (2000, 1000, 256, 8, 1), (0, 1024, 256, 8, 4), (1, 1024, 256, 8, 4), (0, 1025, 256, 8, 5)])
def test_collect_steps_is_untouched(since, every, N, left, want):
    """the launch's step count stays max(1, ceil((update_every - since_update) / N)) cut at the epoch: the update schedule of a
    control_fused run is the per-step run's"""
    from phoenix_drone_simulation_amd.ddpg import collect_steps
    assert collect_steps(since, every, N, left) == want


def test_the_six_units_are_built_and_every_collect_unit_on_disk_is_listed():
    from phoenix_drone_simulation_amd import build
    want = {f"pds_collect_{t}_{f}.hip" for t in ("hover", "circle") for f in ("pid", "lat", "pid_lat")}
    assert want <= set(build._UNITS) and len(build._UNITS) == len(set(build._UNITS))
    on_disk = {os.path.basename(f) for f in glob.glob(os.path.join(build._CSRC, "pds_collect_*.hip"))}
    assert on_disk == want | {f"pds_collect_{t}.hip" for t in ("hover", "circle", "takeoff")} and on_disk <= set(build._UNITS)
    assert any(d.endswith("pds_collect_control.h") for d in build._DEPS)
