"""ctypes binding of the C ABI declared in include/pds.h (libpds_hip.so).

The library is REQUIRED: importing works without it, but any attempt to create an environment
raises -- there is no CPU or PyTorch fallback on the product path.
"""
import ctypes as C
import os

from .build import library_path

TASK_HOVER, TASK_CIRCLE, TASK_TAKEOFF = 0, 1, 2
OK, EINVAL, ENODEVICE, EHIP, ENOMEM, EUNSUPPORTED = 0, -1, -2, -3, -4, -5
SAMPLE_FLOATS = 112
MAX_LATENCY_STEPS = 8
NOISE_FLOATS = 52
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

EXPORTS = ["pds_version", "pds_default_config", "pds_create", "pds_destroy", "pds_obs_dim",
           "pds_num_envs", "pds_reset", "pds_reset_from_samples", "pds_step", "pds_step_with_variates",
           "pds_field_width",
           "pds_get_state", "pds_set_state", "pds_tick", "pds_set_tick", "pds_sync_tick", "pds_count_nonfinite",
           "pds_bytes_per_env_step", "pds_bytes_per_env_step_k", "pds_last_error", "pds_step_k", "pds_step_k_fused", "pds_set_latency",
           "pds_latency_steps", "pds_philox4x32", "pds_noise_normals", "pds_box_muller", "pds_gae", "pds_history_advance",
           "pds_mlp_param_count", "pds_mlp_workspace_floats", "pds_mlp_forward", "pds_ppo_policy_grad",
           "pds_value_grad", "pds_ppo_policy_grad_step", "pds_value_grad_step", "pds_gaussian_sample", "pds_gaussian_sample_dev", "pds_counter_add", "pds_permutation", "pds_rollout_record",
           "pds_adam_step", "pds_rollout", "pds_rollout_history",
           "pds_npg_workspace_floats", "pds_npg_fisher_vector_product", "pds_npg_cg_step", "pds_npg_surrogate_kl",
           "pds_simopt_latency_steps", "pds_simopt_evaluate", "pds_evaluate_supported", "pds_evaluate_policies", "pds_evaluate_policies_metrics", "pds_evaluate_policies_stats",
           "pds_evaluate_history_supported", "pds_evaluate_policies_history",
           "pds_es_workspace_floats", "pds_es_perturb", "pds_es_gradient",
           "pds_ddpg_supported", "pds_ddpg_workspace_floats", "pds_ddpg_policy_grad", "pds_ddpg_target", "pds_polyak",
           "pds_sac_supported", "pds_sac_workspace_floats", "pds_sac_sample", "pds_sac_target", "pds_sac_policy_grad",
           "pds_collect_supported", "pds_collect", "pds_ddpg_explore"]


class Mlp(C.Structure):
    """struct pds_mlp (include/pds.h): 3-layer MLP, torch nn.Linear layout, device pointers."""
    _fields_ = [("d_in", C.c_int32), ("h1", C.c_int32), ("h2", C.c_int32), ("d_out", C.c_int32),
                ("activation", C.c_int32),
                ("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("w3", C.c_void_p), ("b3", C.c_void_p)]


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


_lib = None


def load():
    """dlopen libpds_hip.so (built by build.build_library / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). The HIP extension is required; there is no fallback path.")
    lib = C.CDLL(path)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.pds_version.restype = i32
    if lib.pds_version() != 2:
        raise RuntimeError(f"{path} is version {lib.pds_version()}, this binding needs 2: rebuild it")
    lib.pds_default_config.argtypes = [i32, C.POINTER(Config)]
    lib.pds_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.pds_destroy.argtypes = [vp]
    lib.pds_obs_dim.argtypes = [vp]
    lib.pds_num_envs.argtypes = [vp]
    lib.pds_num_envs.restype = i64
    lib.pds_reset.argtypes = [vp, vp, vp, vp]
    lib.pds_reset_from_samples.argtypes = [vp, vp, vp, vp, vp]
    lib.pds_step.argtypes = [vp] + [vp] * 8
    lib.pds_step_with_variates.argtypes = [vp] + [vp] * 9
    lib.pds_field_width.argtypes = [i32]
    lib.pds_get_state.argtypes = [vp, i32, vp, vp]
    lib.pds_set_state.argtypes = [vp, i32, vp, vp]
    lib.pds_tick.argtypes = [vp]
    lib.pds_tick.restype = C.c_uint64
    lib.pds_set_tick.argtypes = [vp, C.c_uint64]
    lib.pds_sync_tick.argtypes = [vp, vp]
    lib.pds_sync_tick.restype = C.c_uint64
    lib.pds_step_k.argtypes = [vp, i32] + [vp] * 8
    lib.pds_set_latency.argtypes = [vp, C.c_double]
    lib.pds_latency_steps.argtypes = [vp]
    lib.pds_bytes_per_env_step_k.argtypes = [vp, i32]
    lib.pds_philox4x32.argtypes = [vp, vp, i32, i64, vp, vp]
    lib.pds_count_nonfinite.argtypes = [vp, C.POINTER(C.c_int64), vp]
    lib.pds_bytes_per_env_step.argtypes = [vp]
    lib.pds_last_error.argtypes = [vp]
    lib.pds_last_error.restype = C.c_char_p
    lib.pds_gae.argtypes = [vp] * 6 + [C.c_float] * 4 + [i64, i64] + [vp] * 4
    lib.pds_history_advance.argtypes = [i64, C.c_int, C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 4
    mp = C.POINTER(Mlp)
    lib.pds_mlp_param_count.argtypes = [mp]
    lib.pds_mlp_workspace_floats.argtypes = [mp]
    lib.pds_mlp_workspace_floats.restype = i64
    lib.pds_mlp_forward.argtypes = [mp, vp, vp, i64, vp, vp, C.c_float, vp, vp]
    lib.pds_ppo_policy_grad.argtypes = [mp, vp, vp, vp, vp, vp, i64, C.c_float, vp, vp, vp, vp]
    lib.pds_value_grad.argtypes = [mp, vp, vp, vp, i64, vp, vp, vp, vp]
    ap = C.POINTER(Adam)
    u64 = C.c_uint64
    lib.pds_gaussian_sample.argtypes = [vp, vp, i64, i32, u64, u64, u64, i32, vp, vp, vp]
    lib.pds_rollout_record.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.pds_adam_step.argtypes = [mp, vp, vp, vp, i64, C.c_float, C.c_float, C.c_float, C.c_float, vp]

    def later(name, argtypes):
        # entry points added after round 2: absent from an OLDER build loaded through PDS_LIB for a same-box A/B of the
        # step kernels (profiles/tools/ab_lib.sh); the shipped library has them all (tests/test_host_cpu.py)
        if os.environ.get("PDS_LIB") and not hasattr(lib, name):
            return
        getattr(lib, name).argtypes = argtypes

    later("pds_ppo_policy_grad_step", [mp, vp, vp, vp, vp, vp, i64, C.c_float, vp, vp, vp, ap, vp])
    later("pds_value_grad_step", [mp, vp, vp, vp, i64, vp, vp, vp, ap, vp])
    later("pds_gaussian_sample_dev", [vp, vp, i64, i32, u64, vp, u64, u64, i32, vp, vp, vp])
    later("pds_counter_add", [vp, u64, vp])
    later("pds_noise_normals", [u64, u64, C.c_uint32, u64, i64, vp, vp])
    later("pds_box_muller", [vp, i64, vp, vp])
    later("pds_permutation", [vp, i64, u64, u64, vp])
    later("pds_rollout", [vp, i32, mp, mp, vp, vp, C.c_float, vp, u64, vp, u64, i32] + [vp] * 14)
    later("pds_rollout_history", [vp, i32, i32, mp, vp, vp, C.c_float, vp, u64, vp, u64, i32] + [vp] * 9 + [i32] + [vp] * 4)
    later("pds_step_k_fused", [vp])
    later("pds_npg_workspace_floats", [mp, i32])
    if hasattr(lib, "pds_npg_workspace_floats"):
        lib.pds_npg_workspace_floats.restype = i64
    later("pds_npg_fisher_vector_product", [mp, vp, vp, i64, vp, vp, C.c_float, vp, vp, vp])
    later("pds_npg_cg_step", [i64, vp, vp, vp, vp, vp, C.c_float, C.c_float, i32, vp])
    later("pds_npg_surrogate_kl", [mp, vp, vp, i32] + [vp] * 6 + [i64, vp, vp, vp, vp])
    later("pds_simopt_latency_steps", [vp, C.c_double])
    later("pds_simopt_evaluate", [vp, i64, vp, vp, i32, i64, i32, i32, C.c_double] + [vp] * 7)
    later("pds_evaluate_supported", [vp])
    later("pds_evaluate_policies", [vp, i64, i64, mp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp])
    later("pds_evaluate_policies_metrics", [vp, i64, i64, mp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp])
    later("pds_evaluate_policies_stats", [vp, i64, i64, mp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp, vp])
    later("pds_evaluate_history_supported", [vp, i32])
    later("pds_evaluate_policies_history", [vp, i32, i64, i64, mp, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp, vp])
    later("pds_es_workspace_floats", [i64, i64])
    if hasattr(lib, "pds_es_workspace_floats"):
        lib.pds_es_workspace_floats.restype = i64
    later("pds_es_perturb", [vp, i64, i64, C.c_float, u64, u64, u64, vp, vp])
    later("pds_es_gradient", [vp, vp, i64, i64, C.c_float, C.c_float, u64, u64, u64, vp, vp, vp])
    later("pds_ddpg_supported", [mp, mp])
    later("pds_ddpg_workspace_floats", [mp, mp])
    if hasattr(lib, "pds_ddpg_workspace_floats"):
        lib.pds_ddpg_workspace_floats.restype = i64
    later("pds_ddpg_policy_grad", [mp, mp, vp, vp, i64, C.c_float, vp, vp, vp, ap, vp])
    later("pds_ddpg_target", [mp, mp, vp, vp, i64, vp, vp, C.c_float, C.c_float, vp, vp])
    later("pds_polyak", [mp, mp, C.c_double, vp])
    later("pds_sac_supported", [mp, mp, mp])
    later("pds_sac_workspace_floats", [mp, mp, mp])
    if hasattr(lib, "pds_sac_workspace_floats"):
        lib.pds_sac_workspace_floats.restype = i64
    later("pds_sac_sample", [vp, i64, C.c_float, u64, u64, u64, i32, vp, vp, vp])
    later("pds_sac_target", [mp, mp, mp, vp, vp, i64, vp, vp, C.c_float, C.c_float, C.c_float, u64, u64, vp, vp])
    later("pds_sac_policy_grad", [mp, mp, mp, vp, vp, i64, C.c_float, C.c_float, u64, u64, vp, vp, vp, ap, vp])
    later("pds_collect_supported", [vp, mp, i32])
    later("pds_collect", [vp, i32, i32, mp, C.c_float, vp, u64, u64, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp])
    later("pds_ddpg_explore", [vp, vp, i64, C.c_float, u64, u64, u64, vp, vp])
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
