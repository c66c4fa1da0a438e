"""Every env configuration the constructor accepts, over the axes a kernel variant is chosen by, and for each whether the
one-launch kernels (pds_rollout, pds_evaluate_policies; pds_collect: collect_family) are built for it.  TEST INFRASTRUCTURE,
shared by tests/test_gpu_evaluate_variants.py, tests/test_gpu_evaluate_forms_variants.py, tests/test_gpu_collect_variants.py and the
rollout sweep of tests/test_trainer.py.

The axes: task (Hover, Circle, TakeOff) x motor dynamics x domain randomisation x thrust noise x observation noise x ground
effect x control mode (PWM, AttitudeRate, Attitude) x latency ring x Kalman hold (observation_frequency = 50 < sim_freq = 100; it
exists only WITH observation noise -- obs_rate is read in the noisy branch of compute_observation, envs/hover.py:134-156 -- so
the axis is enumerated there only).

What the constructor refuses (not enumerated): a PID control mode on TakeOff (envs/takeoff.py:225 fixes PWM); a PID control mode
with the ground effect together with the latency ring or the hold (pds_create: not built).

`supported` is the rule as DESIGN 8c and the comments of csrc/pds_types.h / csrc/pds_evaluate.h state it, written out here and
NOT read from the library.  With lean = no DR, no thrust noise, no observation noise and full = all three (the reference's
defaults):
  ground effect   TakeOff only: control_mode PWM, no latency ring, no hold, no motor dynamics; every noise setting          (8)
  hold            observation noise (by definition), DR and thrust noise both or neither, control_mode PWM, no latency ring;
                  with or without motor dynamics, TakeOff without                                                          (10)
  latency ring    lean or full; every control mode, with or without motor dynamics (TakeOff: PWM, both)                    (28)
  PID modes       (no latency ring) lean or full; Hover and Circle, with or without motor dynamics                         (16)
  PWM otherwise   EVERY setting of DR x thrust noise x observation noise; with or without motor dynamics, TakeOff without  (40)
and nothing else: 102 configurations."""
import itertools

HOVER, CIRCLE, TAKEOFF = "DroneHoverSimpleEnv-v0", "DroneCircleSimpleEnv-v0", "DroneTakeOffSimpleEnv-v0"
TASKS = (("hover", HOVER), ("circle", CIRCLE), ("takeoff", TAKEOFF))
CTRL = ("PWM", "AttitudeRate", "Attitude")
FAMILIES = ("pwm", "takeoff_ge", "latency", "pid", "hold")
FAMILY_COUNTS = {"pwm": 40, "takeoff_ge": 8, "latency": 28, "pid": 16, "hold": 10}  # literals: the sweep cannot shrink unnoticed


def family(task, motor, dr, tn, on, ge, ctrl, lat, hold):
    """the family whose kernels fly this configuration, or None where none is built (module docstring)"""
    lean, full = not (dr or tn or on), dr and tn and on
    takeoff = task == "takeoff"
    if ge:
        return "takeoff_ge" if takeoff and ctrl == "PWM" and not lat and not hold and not motor else None
    if hold:
        return "hold" if on and dr == tn and ctrl == "PWM" and not lat and not (takeoff and motor) else None
    if lat:
        return "latency" if (lean or full) and (ctrl == "PWM" or not takeoff) else None
    if ctrl != "PWM":
        return "pid" if (lean or full) and not takeoff else None
    return None if takeoff and motor else "pwm"


COLLECT_COUNT = 10  # literal: Hover and Circle x {lean, full} x {with, without motor dynamics}, TakeOff x {lean, full}


def collect_family(task, motor, dr, tn, on, ge, ctrl, lat, hold):
    """"collect" where the fused off-policy collection (pds_collect) is built for this configuration, else None.  The rule as
    the comment of csrc/pds_collect_args.h states it, written out here and NOT read from the library: control_mode PWM, no
    latency ring, no Kalman hold, no ground effect; noise all off or the reference's default (DR + thrust noise + observation
    noise); with and without motor dynamics, TakeOff without."""
    if ctrl != "PWM" or lat or hold or ge:
        return None
    if not ((dr and tn and on) or not (dr or tn or on)):
        return None
    if task == "takeoff" and motor:
        return None
    return "collect"


HISTORY_COUNT = 26  # literal: Hover and Circle x 3 control modes x {lean, full} x {with, without motor dynamics}, TakeOff x {lean, full}
HISTORY_WIDTHS = (64, 96, 128, 192)  # the input widths the history kernels are instantiated for: 4, 6, 8 and 12 tiles of 16


def history_family(task, motor, dr, tn, on, ge, ctrl, lat, hold):
    """"history" where the observation-history evaluation (pds_evaluate_policies_history: the env configurations of
    pds_rollout_history) is built for this configuration, else None.  The rule as the comments of include/pds.h
    (pds_rollout_history, pds_evaluate_policies_history) state it, written out here and NOT read from the library: no latency
    ring, no Kalman hold, no ground effect; noise all off or the reference's default; every control mode on Hover and Circle, with
    and without motor dynamics; TakeOff with control_mode PWM, without motor dynamics.  (And at most 192 network inputs:
    history_sizes.)"""
    if lat or hold or ge:
        return None
    if not ((dr and tn and on) or not (dr or tn or on)):
        return None
    if task == "takeoff" and (ctrl != "PWM" or motor):
        return None
    return "history"


def history_sizes(half):
    """one observation_history_size H per input width class of the history kernel: the largest H other than 2 (H = 2 flies
    pds_evaluate_policies) with H x half inputs inside the class -> [(H, class width)]"""
    return [(max(H for H in range(1, 193) if H != 2 and H * half <= width), width) for width in HISTORY_WIDTHS]


def kwargs_of(motor, dr, tn, on, ge, ctrl, lat, hold):
    """constructor kwargs; what is not named keeps the reference's default (DR 0.1, thrust noise 0.05, observation noise on)"""
    kw = {}
    if motor: kw["use_motor_dynamics"] = True
    if not dr: kw["domain_randomization"] = -1
    if not tn: kw["motor_thrust_noise"] = 0
    if not on: kw["observation_noise"] = -1
    if ge: kw["use_ground_effect"] = True
    if ctrl != "PWM": kw["control_mode"] = ctrl
    if lat: kw.update(use_latency=True, latency=0.02)
    if hold: kw["observation_frequency"] = 50
    return kw


def flags_of(env_id, kw):
    """(task, motor, dr, tn, on, ge, ctrl, lat, hold) of an env id + constructor kwargs (the inverse of kwargs_of, for kwargs
    written by hand: any positive noise level is on, any observation_frequency below sim_freq = 100 holds)"""
    task = {e: t for t, e in TASKS}[env_id]
    on = kw.get("observation_noise", 1) > 0
    return (task, bool(kw.get("use_motor_dynamics", False)), kw.get("domain_randomization", 0.1) > 0,
            kw.get("motor_thrust_noise", 0.05) > 0, on, bool(kw.get("use_ground_effect", False)), kw.get("control_mode", "PWM"),
            bool(kw.get("use_latency", False)), on and 100 // kw.get("observation_frequency", 100) != 1)


def accepted(task, motor, dr, tn, on, ge, ctrl, lat, hold):
    if hold and not on:
        return False  # (not a configuration of its own: without observation noise there is nothing to hold)
    if task == "takeoff" and ctrl != "PWM":
        return False
    if ctrl != "PWM" and ge and (lat or hold):
        return False
    return True


def _name(task, motor, dr, tn, on, ge, ctrl, lat, hold):
    noise = "lean" if not (dr or tn or on) else ("full" if dr and tn and on else "+".join(n for n, f in (("dr", dr), ("tn", tn), ("on", on)) if f))
    parts = [task, ctrl.lower(), noise] + [n for n, f in (("motor", motor), ("ge", ge), ("lat", lat), ("hold", hold)) if f]
    return "-".join(parts)


def variants():
    """[(id, env id, kwargs, family or None)] over every accepted combination; id = '<family>/<task>-<ctrl>-<noise>[-motor]...'
    for a supported one ('none/...' otherwise), so that `-k pwm/` runs one family"""
    out = []
    b = (False, True)
    for (task, env_id), motor, dr, tn, on, ge, ctrl, lat, hold in itertools.product(TASKS, b, b, b, b, b, CTRL, b, b):
        f = (task, motor, dr, tn, on, ge, ctrl, lat, hold)
        if not accepted(*f):
            continue
        fam = family(*f)
        out.append((f"{fam or 'none'}/{_name(*f)}", env_id, kwargs_of(*f[1:]), fam))
    return out


VARIANTS = variants()
SUPPORTED = [v for v in VARIANTS if v[3] is not None]


def collect_variants():
    """[(id, env id, kwargs)] of the configurations collect_family accepts"""
    out = []
    bb = (False, True)
    for (task, env_id), motor, dr, tn, on, ge, ctrl, lat, hold in itertools.product(TASKS, bb, bb, bb, bb, bb, CTRL, bb, bb):
        f = (task, motor, dr, tn, on, ge, ctrl, lat, hold)
        if accepted(*f) and collect_family(*f):
            out.append((_name(*f), env_id, kwargs_of(*f[1:])))
    return out


COLLECT_SUPPORTED = collect_variants()


def history_variants():
    """[(id, env id, kwargs)] of the configurations history_family accepts"""
    out = []
    bb = (False, True)
    for (task, env_id), motor, dr, tn, on, ge, ctrl, lat, hold in itertools.product(TASKS, bb, bb, bb, bb, bb, CTRL, bb, bb):
        f = (task, motor, dr, tn, on, ge, ctrl, lat, hold)
        if accepted(*f) and history_family(*f):
            out.append((_name(*f), env_id, kwargs_of(*f[1:])))
    return out


HISTORY_SUPPORTED = history_variants()
assert len({v[0] for v in VARIANTS}) == len(VARIANTS)


def random_rows(P, d_in, h1=32, h2=48, seed=0):
    """P seeded random actors as tests/test_gpu_evaluate.py _population builds them (nn.Linear's initialisation, tanh, 32 and 48
    hidden units, output biases spread from -0.6 to 0.6) -> float32 [P, param_count]"""
    import torch
    g = torch.Generator().manual_seed(1000 + seed)
    n = h1 * d_in + h1 + h2 * h1 + h2 + 4 * h2 + 4
    theta = torch.empty(P, n)
    for p in range(P):
        k = 0
        for fan_in, count in ((d_in, h1 * d_in), (d_in, h1), (h1, h2 * h1), (h1, h2), (h2, 4 * h2), (h2, 4)):
            theta[p, k:k + count] = (torch.rand(count, generator=g) * 2 - 1) / fan_in ** 0.5
            k += count
        theta[p, -4:] += -0.6 + 1.2 * p / max(P - 1, 1)
    return theta
