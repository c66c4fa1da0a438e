"""ctypes binding of the C ABI declared in include/pds.h (libpds_hip.so).

The library is REQUIRED: importing works without it, but any attempt to create an environment
raises -- there is no CPU or PyTorch fallback on the product path.
"""
import ctypes as C
import os

import torch

from .build import library_path

TASK_HOVER, TASK_CIRCLE, TASK_TAKEOFF = 0, 1, 2
OK, EINVAL, ENODEVICE, EHIP, ENOMEM, EUNSUPPORTED = 0, -1, -2, -3, -4, -5
SAMPLE_FLOATS = 112
MAX_LATENCY_STEPS = 8
NOISE_FLOATS = 52
ACTIVATIONS = {"relu": 0, "tanh": 1}  # pds_mlp.activation
# field ids (enum pds_field)
FIELDS = dict(pos=0, rpy=1, vel=2, omega=3, quat=4, motor_x=5, last_action=6, prev_action=7,
              step_count=8, quat_sign=9, ref_offset=10, params=11, motor_A=12, motor_K=13, ou=14,
              gyro_bias=15, gyro_lpf=16, noisy_obs=17, pid=18, action_buffer=19, action_idx=20)
CONTROL_MODES = {'PWM': 0, 'AttitudeRate': 1, 'Attitude': 2}
INT_FIELDS = ("step_count", "quat_sign", "ref_offset", "action_idx")
# sample row offsets (PDS_S_*)
SAMPLE_LAYOUT = dict(pos_offset=(0, 3), rpy=(3, 3), vel=(6, 3), omega=(9, 3), motor_x=(12, 4),
                     action=(16, 4), dr_dt=(20, 1), dr_m=(21, 1), dr_J=(22, 3), dr_ftf0=(25, 1),
                     dr_ftf1=(26, 1), dr_T=(27, 4), dr_t2w=(31, 4), ref_offset=(35, 1),
                     noise_call0=(36, 24), noise_call1=(60, 24), action_buf=(84, 28))
# one add_noise call (PDS_N_OBS_*): offsets inside its 24 floats
OBS_NOISE_LAYOUT = dict(pos_z=0, pos_u=3, vel_z=6, bias_z=9, rw_z=12, to_z=15, th_z=18, th_u=21)
# step noise row (PDS_N_*)
STEP_NOISE_LAYOUT = dict(ou=0, a_bias=4, a_rw=7, a_to=10, obs=13, a_pos_z=37, a_pos_u=40, a_vel_z=43, a_th_z=46, a_th_u=49)


class Mlp(C.Structure):
    """struct pds_mlp (include/pds.h): 3-layer MLP, torch nn.Linear layout, device pointers."""
    _fields_ = [("d_in", C.c_int32), ("h1", C.c_int32), ("h2", C.c_int32), ("d_out", C.c_int32),
                ("activation", C.c_int32),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w3", C.c_void_p), ("b3", C.c_void_p)]


MLP_DEEP_MAX_HIDDEN = 4  # PDS_MLP_DEEP_MAX_HIDDEN


class MlpDeep(C.Structure):
    """struct pds_mlp_deep (include/pds_mlp_deep.h): MLP with 3 or 4 hidden layers, torch nn.Linear layout, device pointers."""
    _fields_ = [("d_in", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32 * MLP_DEEP_MAX_HIDDEN), ("d_out", C.c_int32),
                ("activation", C.c_int32),
                ("w", C.c_void_p * (MLP_DEEP_MAX_HIDDEN + 1)), ("b", C.c_void_p * (MLP_DEEP_MAX_HIDDEN + 1))]


class Adam(C.Structure):
    """struct pds_adam (include/pds.h): the optimiser step that rides on a gradient call."""
    _fields_ = [("d_exp_avg", C.c_void_p), ("d_exp_avg_sq", C.c_void_p), ("step", C.c_int64),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float)]


class Config(C.Structure):
    """struct pds_config (include/pds.h)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("task", C.c_int32), ("num_envs", C.c_int64),
        ("env_id_base", C.c_int64), ("seed", C.c_uint64),
        ("device", C.c_int32), ("use_motor_dynamics", C.c_int32), ("use_ground_effect", C.c_int32),
        ("observation_noise", C.c_int32), ("aggregate_phy_steps", C.c_int32),
        ("enable_reset_distribution", C.c_int32), ("max_episode_steps", C.c_int32),
        ("auto_reset", C.c_int32),
        ("domain_randomization", C.c_double), ("motor_thrust_noise", C.c_double),
        ("time_step", C.c_double), ("motor_time_constant", C.c_double),
        ("penalty_action", C.c_double), ("penalty_angle", C.c_double), ("penalty_spin", C.c_double),
        ("penalty_terminal", C.c_double), ("penalty_velocity", C.c_double), ("ARP", C.c_double),
        ("target_pos", C.c_double * 3), ("init_xyz", C.c_double * 3), ("init_rpy", C.c_double * 3),
        ("init_xyz_dot", C.c_double * 3), ("init_rpy_dot", C.c_double * 3),
        ("control_mode", C.c_int32), ("use_latency", C.c_int32), ("latency", C.c_double),
        ("observation_frequency", C.c_int32), ("reserved_", C.c_int32),
    ]


_vp, _i32, _i64, _u32, _u64, _f32, _f64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_double
_mp, _ap, _cp = C.POINTER(Mlp), C.POINTER(Adam), C.POINTER(Config)
_eval = [_vp, _i64, _i64, _mp, _vp, _vp, _vp, _f32, _i32] + [_vp] * 4  # pds_evaluate_policies up to d_cost

# name -> (restype, argtypes): every prototype of include/pds.h (tests/test_host_cpu.py compares the two)
SIGNATURES = {
    "pds_version": (_i32, []),
    "pds_default_config": (_i32, [_i32, _cp]),
    "pds_create": (_i32, [_cp, _vp]),
    "pds_destroy": (_i32, [_vp]),
    "pds_obs_dim": (_i32, [_vp]),
    "pds_num_envs": (_i64, [_vp]),
    "pds_reset": (_i32, [_vp] * 4),
    "pds_reset_from_samples": (_i32, [_vp] * 5),
    "pds_step": (_i32, [_vp] * 9),
    "pds_step_with_variates": (_i32, [_vp] * 10),
    "pds_step_k": (_i32, [_vp, _i32] + [_vp] * 8),
    "pds_step_k_fused": (_i32, [_vp]),
    "pds_set_latency": (_i32, [_vp, _f64]),
    "pds_latency_steps": (_i32, [_vp]),
    "pds_simopt_latency_steps": (_i32, [_vp, _f64]),
    "pds_simopt_evaluate": (_i32, [_vp, _i64, _vp, _vp, _i32, _i64, _i32, _i32, _f64] + [_vp] * 7),
    "pds_field_width": (_i32, [_i32]),
    "pds_get_state": (_i32, [_vp, _i32, _vp, _vp]),
    "pds_set_state": (_i32, [_vp, _i32, _vp, _vp]),
    "pds_count_nonfinite": (_i32, [_vp, _vp, _vp]),
    "pds_tick": (_u64, [_vp]),
    "pds_sync_tick": (_u64, [_vp, _vp]),
    "pds_set_tick": (_i32, [_vp, _u64]),
    "pds_bytes_per_env_step": (_i32, [_vp]),
    "pds_bytes_per_env_step_k": (_i32, [_vp, _i32]),
    "pds_last_error": (C.c_char_p, [_vp]),
    "pds_philox4x32": (_i32, [_vp, _vp, _i32, _i64, _vp, _vp]),
    "pds_noise_normals": (_i32, [_u64, _u64, _u32, _u64, _i64, _vp, _vp]),
    "pds_box_muller": (_i32, [_vp, _i64, _vp, _vp]),
    "pds_history_advance": (_i32, [_i64, _i32, _i32] + [_vp] * 4 + [_i32] + [_vp] * 4),
    "pds_gae": (_i32, [_vp] * 6 + [_f32] * 4 + [_i64, _i64] + [_vp] * 4),
    "pds_rollout": (_i32, [_vp, _i32, _mp, _mp, _vp, _vp, _f32, _vp, _u64, _vp, _u64, _i32] + [_vp] * 14),
    "pds_rollout_history": (_i32, [_vp, _i32, _i32, _mp, _vp, _vp, _f32, _vp, _u64, _vp, _u64, _i32] + [_vp] * 9 + [_i32] + [_vp] * 4),
    "pds_evaluate_supported": (_i32, [_vp]),
    "pds_evaluate_policies": (_i32, _eval + [_vp]),
    "pds_evaluate_policies_metrics": (_i32, _eval + [_vp] * 2),
    "pds_evaluate_policies_stats": (_i32, _eval + [_vp] * 3),
    "pds_evaluate_policies_record": (_i32, _eval + [_vp, _i64, _vp, _vp, _vp]),
    "pds_evaluate_history_supported": (_i32, [_vp, _i32]),
    "pds_evaluate_policies_history": (_i32, [_vp, _i32] + _eval[1:] + [_vp] * 2),
    "pds_mlp_param_count": (_i32, [_mp]),
    "pds_mlp_workspace_floats": (_i64, [_mp]),
    "pds_mlp_forward": (_i32, [_mp, _vp, _vp, _i64, _vp, _vp, _f32, _vp, _vp]),
    "pds_ppo_policy_grad": (_i32, [_mp] + [_vp] * 5 + [_i64, _f32] + [_vp] * 4),
    "pds_value_grad": (_i32, [_mp, _vp, _vp, _vp, _i64] + [_vp] * 4),
    "pds_gaussian_sample": (_i32, [_vp, _vp, _i64, _i32, _u64, _u64, _u64, _i32, _vp, _vp, _vp]),
    "pds_gaussian_sample_dev": (_i32, [_vp, _vp, _i64, _i32, _u64, _vp, _u64, _u64, _i32, _vp, _vp, _vp]),
    "pds_counter_add": (_i32, [_vp, _u64, _vp]),
    "pds_permutation": (_i32, [_vp, _i64, _u64, _u64, _vp]),
    "pds_rollout_record": (_i32, [_vp, _vp, _vp, _i64] + [_vp] * 7),
    "pds_adam_step": (_i32, [_mp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _vp]),
    "pds_ppo_policy_grad_step": (_i32, [_mp] + [_vp] * 5 + [_i64, _f32] + [_vp] * 3 + [_ap, _vp]),
    "pds_value_grad_step": (_i32, [_mp, _vp, _vp, _vp, _i64] + [_vp] * 3 + [_ap, _vp]),
    "pds_npg_workspace_floats": (_i64, [_mp, _i32]),
    "pds_npg_fisher_vector_product": (_i32, [_mp, _vp, _vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp]),
    "pds_npg_cg_step": (_i32, [_i64] + [_vp] * 5 + [_f32, _f32, _i32, _vp]),
    "pds_npg_surrogate_kl": (_i32, [_mp, _vp, _vp, _i32] + [_vp] * 6 + [_i64] + [_vp] * 4),
    "pds_es_workspace_floats": (_i64, [_i64, _i64]),
    "pds_es_perturb": (_i32, [_vp, _i64, _i64, _f32, _u64, _u64, _u64, _vp, _vp]),
    "pds_es_gradient": (_i32, [_vp, _vp, _i64, _i64, _f32, _f32, _u64, _u64, _u64, _vp, _vp, _vp]),
    "pds_ddpg_supported": (_i32, [_mp, _mp]),
    "pds_ddpg_workspace_floats": (_i64, [_mp, _mp]),
    "pds_ddpg_policy_grad": (_i32, [_mp, _mp, _vp, _vp, _i64, _f32, _vp, _vp, _vp, _ap, _vp]),
    "pds_ddpg_target": (_i32, [_mp, _mp, _vp, _vp, _i64, _vp, _vp, _f32, _f32, _vp, _vp]),
    "pds_polyak": (_i32, [_mp, _mp, _f64, _vp]),
    "pds_sac_supported": (_i32, [_mp] * 3),
    "pds_sac_workspace_floats": (_i64, [_mp] * 3),
    "pds_sac_sample": (_i32, [_vp, _i64, _f32, _u64, _u64, _u64, _i32, _vp, _vp, _vp]),
    "pds_sac_target": (_i32, [_mp] * 3 + [_vp, _vp, _i64, _vp, _vp, _f32, _f32, _f32, _u64, _u64, _vp, _vp]),
    "pds_sac_policy_grad": (_i32, [_mp] * 3 + [_vp, _vp, _i64, _f32, _f32, _u64, _u64, _vp, _vp, _vp, _ap, _vp]),
    "pds_collect_supported": (_i32, [_vp, _mp, _i32]),
    "pds_collect": (_i32, [_vp, _i32, _i32, _mp, _f32, _vp, _u64, _u64] + [_vp] * 4 + [_i64, _i64] + [_vp] * 5),
    "pds_ddpg_explore": (_i32, [_vp, _vp, _i64, _f32, _u64, _u64, _u64, _vp, _vp]),
}
EXPORTS = list(SIGNATURES)
# ... and of include/pds_history_record.h, the entry point that stands beside that ABI (tests/test_evaluate_history_record_cpu.py
# compares the two); `load` binds every table, `call` enters any
HISTORY_RECORD_SIGNATURES = {
    "pds_evaluate_policies_history_record": (_i32, [_vp, _i32] + _eval[1:] + [_vp, _i64, _vp, _vp, _vp]),
}
# ... and of include/pds_history_stats.h, the two that stand beside it likewise (tests/test_evaluate_history_stats_cpu.py)
HISTORY_STATS_SIGNATURES = {
    "pds_evaluate_history_stats_supported": (_i32, [_vp, _i32]),
    "pds_evaluate_policies_history_stats": (_i32, [_vp, _i32] + _eval[1:] + [_vp] * 3),
}
# ... and of include/pds_collect_control.h, the collection under the PID control modes and the latency ring
# (tests/test_collect_control_cpu.py): the rows of pds_collect_supported and pds_collect
COLLECT_CONTROL_SIGNATURES = {
    "pds_collect_control_supported": SIGNATURES["pds_collect_supported"],
    "pds_collect_control": SIGNATURES["pds_collect"],
}
# ... and of include/pds_history_latency.h, the per-step history launch on the latency ring (tests/test_history_latency_cpu.py)
HISTORY_LATENCY_SIGNATURES = {
    "pds_history_advance_latency": (_i32, [_i64, _i32, _i32] + [_vp] * 4 + [_i32] + [_vp] * 6 + [_i32, _i32, _vp]),
    "pds_rollout_history_latency_supported": (_i32, [_vp, _i32]),
    "pds_rollout_history_latency": SIGNATURES["pds_rollout_history"],
}
# ... and of include/pds_history_latency_evaluate.h, the evaluation of history policies on the latency ring
# (tests/test_history_latency_evaluate_cpu.py): the rows of the three non-latency calls and of their two questions
HISTORY_LATENCY_EVALUATE_SIGNATURES = {
    "pds_evaluate_history_latency_supported": SIGNATURES["pds_evaluate_history_supported"],
    "pds_evaluate_history_latency_stats_supported": HISTORY_STATS_SIGNATURES["pds_evaluate_history_stats_supported"],
    "pds_evaluate_policies_history_latency": SIGNATURES["pds_evaluate_policies_history"],
    "pds_evaluate_policies_history_latency_record": HISTORY_RECORD_SIGNATURES["pds_evaluate_policies_history_record"],
    "pds_evaluate_policies_history_latency_stats": HISTORY_STATS_SIGNATURES["pds_evaluate_policies_history_stats"],
}
# ... and of include/pds_mlp_deep.h, the dense kernels for networks with 3 or 4 hidden layers (tests/test_mlp_deep_cpu.py); the
# struct pds_mlp_deep goes in by reference as a plain pointer (MlpDeep)
MLP_DEEP_SIGNATURES = {
    "pds_mlp_deep_supported": (_i32, [_vp]),
    "pds_mlp_deep_param_count": (_i32, [_vp]),
    "pds_mlp_deep_workspace_floats": (_i64, [_vp]),
    "pds_mlp_deep_forward": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _f32, _vp, _vp]),
    "pds_mlp_deep_ppo_policy_grad_step": (_i32, [_vp] * 6 + [_i64, _f32] + [_vp] * 3 + [_ap, _vp]),
    "pds_mlp_deep_value_grad_step": (_i32, [_vp] * 4 + [_i64] + [_vp] * 3 + [_ap, _vp]),
    "pds_mlp_deep_adam_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _vp]),
}
# ... and of include/pds_npg_deep.h, the natural-gradient kernels for actors with 3 or 4 hidden layers (tests/test_npg_deep_cpu.py):
# the rows of the three pds_npg_* calls that take a network, behind the struct pds_mlp_deep pointer
NPG_DEEP_SIGNATURES = {
    "pds_npg_deep_workspace_floats": (_i64, [_vp] + SIGNATURES["pds_npg_workspace_floats"][1][1:]),
    "pds_npg_deep_fisher_vector_product": (_i32, [_vp] + SIGNATURES["pds_npg_fisher_vector_product"][1][1:]),
    "pds_npg_deep_surrogate_kl": (_i32, [_vp] + SIGNATURES["pds_npg_surrogate_kl"][1][1:]),
}
# ... and of include/pds_evaluate_deep.h, the population evaluation for actors with 3 or 4 hidden layers
# (tests/test_evaluate_deep_cpu.py): pds_evaluate_policies_metrics' row behind the struct pds_mlp_deep pointer
EVALUATE_DEEP_SIGNATURES = {
    "pds_evaluate_deep_supported": (_i32, [_vp, _vp]),
    "pds_evaluate_policies_deep": (_i32, _eval[:3] + [_vp] + _eval[4:] + [_vp] * 2),
}
# ... and of include/pds_evaluate_deep_forms.h, the stats and the record form of that evaluation
# (tests/test_evaluate_deep_forms_cpu.py): pds_evaluate_policies_deep's row with what pds_evaluate_policies_stats / _record add
EVALUATE_DEEP_FORMS_SIGNATURES = {
    "pds_evaluate_deep_forms_supported": (_i32, [_vp, _vp, _i32]),
    "pds_evaluate_policies_deep_stats": (_i32, EVALUATE_DEEP_SIGNATURES["pds_evaluate_policies_deep"][1][:-1] + [_vp] * 2),
    "pds_evaluate_policies_deep_record": (_i32, EVALUATE_DEEP_SIGNATURES["pds_evaluate_policies_deep"][1][:-1] + [_i64, _vp, _vp, _vp]),
}
EVALUATE_DEEP_FORM_STATS, EVALUATE_DEEP_FORM_RECORD = 0, 1  # the `form` of pds_evaluate_deep_forms_supported
# ... and of include/pds_rollout_deep.h, the one-launch rollout for actors with 3 or 4 hidden layers (tests/test_rollout_deep_cpu.py):
# pds_rollout_history's row without the history, behind the struct pds_mlp_deep pointer
ROLLOUT_DEEP_SIGNATURES = {
    "pds_rollout_deep_supported": (_i32, [_vp, _vp]),
    "pds_rollout_deep": (_i32, SIGNATURES["pds_rollout_history"][1][:2] + [_vp] + SIGNATURES["pds_rollout_history"][1][4:]),
}

# ... and of include/pds_mlp_broad.h, the dense kernels and DDPG's update for two-hidden-layer networks with a hidden width above
# 64 (tests/test_mlp_broad_cpu.py): the rows of the include/pds.h entry points of the same names, on the same struct pds_mlp
MLP_BROAD_SIGNATURES = {
    "pds_mlp_broad_supported": (_i32, [_mp]),
    "pds_mlp_broad_param_count": SIGNATURES["pds_mlp_param_count"],
    "pds_mlp_broad_workspace_floats": SIGNATURES["pds_mlp_workspace_floats"],
    "pds_mlp_broad_forward": SIGNATURES["pds_mlp_forward"],
    "pds_mlp_broad_value_grad_step": SIGNATURES["pds_value_grad_step"],
    "pds_mlp_broad_adam_step": SIGNATURES["pds_adam_step"],
    "pds_ddpg_broad_supported": SIGNATURES["pds_ddpg_supported"],
    "pds_ddpg_broad_workspace_floats": SIGNATURES["pds_ddpg_workspace_floats"],
    "pds_ddpg_broad_policy_grad": SIGNATURES["pds_ddpg_policy_grad"],
    "pds_ddpg_broad_target": SIGNATURES["pds_ddpg_target"],
    "pds_polyak_broad": SIGNATURES["pds_polyak"],
}
MLP_BROAD_MAX_HIDDEN, MLP_BROAD_MAX_BATCH = 512, 65536  # PDS_MLP_BROAD_MAX_HIDDEN, PDS_MLP_BROAD_MAX_BATCH

_lib = None


def load():
    """dlopen libpds_hip.so (built by build.build_library / __graft_entry__.build) and give every entry point its SIGNATURES row."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The HIP extension is required; there is no fallback path.")
    lib = C.CDLL(path)
    if lib.pds_version() != 2:
        raise RuntimeError(f"{path} is version {lib.pds_version()}, this binding needs 2: rebuild it")
    # an OLDER build given through PDS_LIB for a same-box A/B (profiles/tools/ab_lib.sh) may lack the newer entry points: those
    # are skipped; the shipped library must have every name (AttributeError here, and tests/test_host_cpu.py)
    older = bool(os.environ.get("PDS_LIB"))
    for name, (restype, argtypes) in list(SIGNATURES.items()) + list(HISTORY_RECORD_SIGNATURES.items()) + list(HISTORY_STATS_SIGNATURES.items()) + list(COLLECT_CONTROL_SIGNATURES.items()) + list(HISTORY_LATENCY_SIGNATURES.items()) + list(HISTORY_LATENCY_EVALUATE_SIGNATURES.items()) + list(MLP_DEEP_SIGNATURES.items()) + list(NPG_DEEP_SIGNATURES.items()) + list(EVALUATE_DEEP_SIGNATURES.items()) + list(EVALUATE_DEEP_FORMS_SIGNATURES.items()) + list(ROLLOUT_DEEP_SIGNATURES.items()) + list(MLP_BROAD_SIGNATURES.items()):
        if older and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def default_config(task):
    cfg = Config()
    rc = load().pds_default_config(int(task), C.byref(cfg))
    if rc != OK:
        raise ValueError(f"pds_default_config({task}) -> {rc}")
    return cfg


def check(handle, rc, what):
    if rc == OK:
        return
    msg = load().pds_last_error(handle)
    msg = msg.decode() if msg else ""
    exc = {EINVAL: ValueError, EUNSUPPORTED: NotImplementedError, ENOMEM: MemoryError}.get(rc, RuntimeError)
    raise exc(f"{what} failed ({rc}): {msg}")


_MLP_POINTERS = ("w1", "b1", "w2", "b2", "w3", "b3")


def mlp(d_in, h1, h2, d_out, activation, tensors=None, base=None):
    """struct pds_mlp of a d_in -> h1 -> h2 -> d_out network.  Its six pointers come from `tensors` (W1, b1, W2, b2, W3, b3) or
    from `base`, the address of a flat float32 parameter row that holds them in that order (pds_mlp_param_count's layout)."""
    m = Mlp(int(d_in), int(h1), int(h2), int(d_out), ACTIVATIONS[activation])
    if tensors is not None:
        bind_mlp(m, tensors)
    else:
        for name, n in zip(_MLP_POINTERS, (h1 * d_in, h1, h2 * h1, h2, d_out * h2, d_out)):
            setattr(m, name, base)
            base += 4 * n
    return m


def bind_mlp(m, tensors):
    """Point the struct at where W1, b1, W2, b2, W3, b3 are now (an optimiser or a load may have moved them)."""
    m.w1, m.b1, m.w2, m.b2, m.w3, m.b3 = [t.data_ptr() for t in tensors]


def mlp_deep(d_in, hidden, d_out, activation, tensors=None, base=None):
    """struct pds_mlp_deep of a d_in -> hidden[0] -> ... -> hidden[-1] -> d_out network (3 or 4 hidden layers).  Its pointers come
    from `tensors` (W1, b1, ..., W(L+1), b(L+1)) or from `base`, the address of a flat float32 parameter row that holds them in
    that order (pds_mlp_deep_param_count's layout)."""
    hidden = [int(h) for h in hidden]
    if len(hidden) > MLP_DEEP_MAX_HIDDEN:
        raise ValueError(f"struct pds_mlp_deep holds up to {MLP_DEEP_MAX_HIDDEN} hidden layers, not {len(hidden)}")
    m = MlpDeep(int(d_in), len(hidden), (C.c_int32 * MLP_DEEP_MAX_HIDDEN)(*hidden), int(d_out), ACTIVATIONS[activation])
    if tensors is not None:
        bind_mlp_deep(m, tensors)
    elif base is not None:
        dims = [int(d_in)] + hidden + [int(d_out)]
        for l in range(len(hidden) + 1):
            m.w[l] = base
            base += 4 * dims[l + 1] * dims[l]
            m.b[l] = base
            base += 4 * dims[l + 1]
    return m


def bind_mlp_deep(m, tensors):
    """Point the struct at where W1, b1, ..., W(L+1), b(L+1) are now (an optimiser or a load may have moved them)."""
    for l in range(len(tensors) // 2):
        m.w[l], m.b[l] = tensors[2 * l].data_ptr(), tensors[2 * l + 1].data_ptr()


def _ptr(t, byte_offset=0):
    """A tensor's device pointer as a ctypes argument (None: NULL), for the direct calls; `call` converts tensors itself."""
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None



class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL = _NullCtx()
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # (device index) -> stream handle as int


def on_device(t):
    """Context that makes the device of `t` (a tensor or a torch.device) current if it is not: a process that holds envs /
    networks on several GPUs must not launch on, or take the stream of, whichever device happens to be current."""
    dev = t if isinstance(t, torch.device) else t.device
    return _NULL if dev.index is None or dev.index == torch.cuda.current_device() else torch.cuda.device(dev)


def current_stream(t):
    """hipStream_t, as an int, of torch's CURRENT stream on the device of `t` (a tensor or a torch.device)"""
    dev = t if isinstance(t, torch.device) else t.device
    if _RAW_STREAM is not None and dev.index is not None:
        return _RAW_STREAM(dev.index)
    return torch.cuda.current_stream(dev).cuda_stream


_SCALARS = (int, float)  # argument types `call` passes on without a look


def call(name, *args, on=None, handle=None):
    """THE way into an entry point that returns a code (value queries -- *_supported, *_workspace_floats, pds_tick ... -- are
    called on load() directly).  Of `args` a tensor goes in as its device pointer, an object that carries a struct pds_mlp
    whose pointers follow its parameters (fused.FusedMLP) is re-bound and goes in by reference, anything else as it is (None:
    NULL).  on: a tensor or device -- its device is current during the call and its current stream is appended as the last
    argument; None for entry points without a stream parameter.  A non-zero code raises: with `handle` what `check` raises (the
    handle's last-error text), without one NotImplementedError for PDS_EUNSUPPORTED and RuntimeError otherwise."""
    fn = getattr(load(), name)
    a = []
    for x in args:
        if x is not None and type(x) not in _SCALARS:
            if hasattr(x, "data_ptr"):
                x = x.data_ptr()
            elif hasattr(x, "_bind"):
                if getattr(x, "deep", False):  # a struct pds_mlp_deep: only its own entry points may read it
                    if name not in MLP_DEEP_SIGNATURES and name not in NPG_DEEP_SIGNATURES and name not in EVALUATE_DEEP_SIGNATURES and name not in EVALUATE_DEEP_FORMS_SIGNATURES and name not in ROLLOUT_DEEP_SIGNATURES:
                        raise NotImplementedError(f"{name} takes networks with 2 hidden layers (struct pds_mlp), not {x.n_hidden}")
                    x._bind()
                    x = C.byref(x.md)
                else:
                    if getattr(x, "broad", False) != (name in MLP_BROAD_SIGNATURES):  # a width above 64: only its own entry points
                        raise NotImplementedError(f"{name} takes networks with hidden widths " +
                                                  ("above 64 (include/pds_mlp_broad.h)" if name in MLP_BROAD_SIGNATURES else
                                                   "up to 64, not a network built with broad=True (include/pds_mlp_broad.h)"))
                    x._bind()
                    x = C.byref(x.m)
        a.append(x)
    if on is None:
        rc = fn(*a)
    else:
        a.append(current_stream(on))
        with on_device(on):
            rc = fn(*a)
    if rc != OK:
        if handle is not None:
            check(handle, rc, name)
        raise (NotImplementedError if rc == EUNSUPPORTED else RuntimeError)(f"{name} -> {rc}")

