"""Simulation optimisation (sim-opt): fit (thrust_to_weight_ratio, motor_time_constant, latency) to logged flights.

Counterpart of the reference's simopt/ package (paths relative to phoenix_drone_simulation/):

  MiniTrajectories  <- RealWorldDataBuffer (simopt/core.py:34-178): battery compensation, slicing of a log into
                       mini-trajectories, the pre-inputs that warm the motor state up
  SimOptObjective   <- ObjectiveFunctionPyBullet (simopt/pybullet.py:26-248) on the SimplePhysics env with the PT1 motor
                       model on: evaluate / evaluate_once / loss_function / set_parameters

The reference evaluates one candidate at a time, N mini-trajectories x (pre_steps + T - 1) env.step() calls each.  Here ONE
launch of pds_simopt_evaluate (csrc/pds_simopt.hip) scores P candidates x M mini-trajectories; `fused=False` evaluates the same
objective through the per-step entry points (set_state / set_latency / step_k + torch for the loss): slow, and the path the
kernel is tested against.

Two stated differences from the reference: every sample runs its pre-steps from the env reset WITHOUT the reset distribution
(the reference's first evaluate_once of a process still has it on: the flag is cleared at simopt/pybullet.py:153), and the
objective is deterministic (motor_thrust_noise = 0; the reference's env keeps its default 0.05).

Importing this module needs no GPU; constructing a SimOptObjective does.
"""
import ctypes as C
import os

import numpy as np

from . import native

# ObjectiveFunctionPyBullet.__init__, simopt/pybullet.py:42-51
PARAMETER_LOW = np.array([1.5, 0.010, 0.000])
PARAMETER_HIGH = np.array([2.5, 0.500, 0.050])
# loggers' column names, simopt/core.py:95-104
OBS_COLUMNS = ['x', 'y', 'z', 'x_dot', 'y_dot', 'z_dot', 'roll', 'pitch', 'yaw', 'roll_dot', 'pitch_dot', 'yaw_dot']
PWM_COLUMNS = ['mot0', 'mot1', 'mot2', 'mot3']
G = 9.81  # envs/agents.py:150


# ---- pybullet's rotation helpers in float64 numpy, vectorised over the leading axis ----------------------------
def quat_from_euler(rpy):
    """pybullet.getQuaternionFromEuler: [x, y, z, w]."""
    h = 0.5 * np.asarray(rpy, np.float64)
    sr, sp, sy = np.sin(h[..., 0]), np.sin(h[..., 1]), np.sin(h[..., 2])
    cr, cp, cy = np.cos(h[..., 0]), np.cos(h[..., 1]), np.cos(h[..., 2])
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy,
                  cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], -1)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def matrix_from_quat(q):
    """pybullet.getMatrixFromQuaternion (btMatrix3x3::setRotation): [..., 3, 3]."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    s = 2.0 / (x * x + y * y + z * z + w * w)
    xs, ys, zs = x * s, y * s, z * s
    wx, wy, wz = w * xs, w * ys, w * zs
    xx, xy, xz = x * xs, x * ys, x * zs
    yy, yz, zz = y * ys, y * zs, z * zs
    R = np.stack([1.0 - (yy + zz), xy - wz, xz + wy,
                  xy + wz, 1.0 - (xx + zz), yz - wx,
                  xz - wy, yz + wx, 1.0 - (xx + yy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def euler_from_quat(q):
    """pybullet.getEulerFromQuaternion (gimbal guard at |sarg| >= 0.99999)."""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    sarg = -2.0 * (x * z - w * y)
    roll = np.arctan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z)
    pitch = np.arcsin(np.clip(sarg, -1.0, 1.0))
    yaw = np.arctan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)
    lo, hi = sarg <= -0.99999, sarg >= 0.99999
    roll = np.where(lo | hi, 0.0, roll)
    pitch = np.where(lo, -0.5 * np.pi, np.where(hi, 0.5 * np.pi, pitch))
    yaw = np.where(lo, 2.0 * np.arctan2(x, -y), np.where(hi, 2.0 * np.arctan2(-x, y), yaw))
    return np.stack([roll, pitch, yaw], -1)


def start_state(row0):
    """The env state evaluate_once's second reset produces from a logged row [x y z, xyz_dot, rpy, rpy_dot]
    (simopt/pybullet.py:139-156): init_rpy_dot = R @ rpy_dot, resetBaseVelocity(R.T @ init_rpy_dot)
    (envs/hover.py:237-243), and update_information's read-back rpy = Euler(Q(rpy)), rpy_dot = R.T @ world rates
    (envs/agents.py:443-453).  Same column order as the log."""
    row0 = np.asarray(row0, np.float64)
    rpy, w = row0[..., 6:9], row0[..., 9:12]
    q = quat_from_euler(rpy)
    R = matrix_from_quat(q)
    Rt = np.swapaxes(R, -1, -2)
    init_rpy_dot = np.einsum('...ij,...j->...i', R, w)
    world = np.einsum('...ij,...j->...i', Rt, init_rpy_dot)
    body = np.einsum('...ij,...j->...i', Rt, world)
    return np.concatenate([row0[..., 0:6], euler_from_quat(q), body], -1)


def latency_steps(latency, time_step):
    """buf_size of CrazyFlieAgent.set_latency (envs/agents.py:397-401) in its float64 form: 0 below one time step, else
    int(latency / time_step), the true division (not `//`: 0.03 // 0.01 is 2.0).  Same rule as pds_simopt_latency_steps."""
    lat = np.asarray(latency, np.float64)
    with np.errstate(invalid='ignore'):
        steps = np.where(lat < time_step, 0.0, np.floor(lat / time_step))
    return np.nan_to_num(np.clip(steps, 0, 1e6), nan=0.0).astype(np.int32)


class MiniTrajectories:
    """M mini-trajectories of length T with their pre-inputs: observations [M, T, 12] in the log's column order,
    actions [M, T, 4] in [-1, 1], pre_inputs [M, pre_steps, 4] (float64, on the host), and -- once an objective asks for
    them -- the device copies in the kernel's time-major layout."""

    def __init__(self, observations, actions, pre_inputs):
        self.observations = np.ascontiguousarray(observations, np.float64)
        self.actions = np.ascontiguousarray(actions, np.float64)
        self.pre_inputs = np.ascontiguousarray(pre_inputs, np.float64)
        M, T = self.observations.shape[:2]
        if self.observations.shape != (M, T, 12) or self.actions.shape != (M, T, 4) or T < 2 or M < 1:
            raise ValueError(f"observations [M, T, 12] and actions [M, T, 4] expected, got {self.observations.shape}, "
                             f"{self.actions.shape}")
        if self.pre_inputs.ndim != 3 or self.pre_inputs.shape[0] != M or self.pre_inputs.shape[2] != 4:
            raise ValueError(f"pre_inputs [M, pre_steps, 4] expected, got {self.pre_inputs.shape}")
        self.mini_trajectory_size = T
        self.pre_steps = int(self.pre_inputs.shape[1])
        self._device = {}

    def __len__(self):
        return self.observations.shape[0]

    # battery model of the logs (simopt/core.py:79-92): the motor voltage is duty x battery voltage, and the firmware's
    # thrust curve  volts = QUAD thrust^2 + LIN thrust  (thrust in grams, 60 g = full scale) is solved for the thrust
    BATTERY_QUAD, BATTERY_LIN = -0.0006239, 0.088

    @classmethod
    def exclude_battery_compensation(cls, pwms, voltages):
        """The PWMs a fully charged battery would have needed for the same thrust (operation order kept: the slices equal
        the reference's bit for bit, tests/test_simopt_cpu.py)."""
        qa, qb = cls.BATTERY_QUAD, cls.BATTERY_LIN
        motor_volts = pwms / 65535 * voltages
        disc = np.clip(qb ** 2 - 4 * qa * -motor_volts, qb ** 2 / (4 * qa), np.inf)
        grams = (-qb + np.sqrt(disc)) / (2 * qa)
        return np.clip(grams / 60, 0, 1) * 65535

    # -- simopt/core.py:47-77
    @staticmethod
    def create_trajectory_slices(obs, PWMs, T=35, pre_steps=5, skip=10):
        L = obs.shape[0]
        acs = PWMs / 30000.0 - 1
        if not L > T + pre_steps:
            raise ValueError(f"a log of {L} rows is too short for T = {T}, pre_steps = {pre_steps}")
        starts = range(pre_steps, L - T, skip)
        return (np.array([obs[i:i + T] for i in starts]), np.array([acs[i:i + T] for i in starts]),
                np.array([acs[i - pre_steps:i] for i in starts]).reshape(len(starts), pre_steps, 4))

    @classmethod
    def from_logs(cls, obs, pwms, voltages, T=35, pre_steps=5, skip=10):
        """One log: obs [L, 12], pwms [L, 4], voltages [L] or [L, 1] -> battery compensation, acs = PWM / 30000 - 1, slices
        of T rows every `skip` rows after `pre_steps`.  Several logs: lists of such arrays (concatenated like load_from_disk)."""
        if isinstance(obs, (list, tuple)):
            parts = [cls.from_logs(o, p, v, T, pre_steps, skip) for o, p, v in zip(obs, pwms, voltages)]
            return cls(*[np.concatenate([getattr(p, n) for p in parts]) for n in ("observations", "actions", "pre_inputs")])
        obs = np.asarray(obs, np.float64)
        pwms = np.asarray(pwms, np.float64)
        voltages = np.asarray(voltages, np.float64).reshape(-1, 1)
        cleaned = cls.exclude_battery_compensation(pwms, voltages)
        return cls(*cls.create_trajectory_slices(obs, cleaned, T, pre_steps, skip))

    @classmethod
    def from_csv_dir(cls, path, T=35, pre_steps=5, skip=10):
        """Every *.csv below `path` with the reference's columns (simopt/core.py:95-104, 131-171); logs that are too short for
        one mini-trajectory are left out."""
        import pandas as pd
        logs = []
        for dir_path, _, files in os.walk(path):
            for name in sorted(files):
                if name.endswith(".csv"):
                    df = pd.read_csv(os.path.join(dir_path, name))
                    o = df[OBS_COLUMNS].to_numpy(dtype=np.float64)
                    if o.shape[0] > T + pre_steps:
                        logs.append((o, df[PWM_COLUMNS].to_numpy(dtype=np.float64), df[['bat']].to_numpy(dtype=np.float64)))
        if not logs:
            raise FileNotFoundError(f"no usable CSV log below {path}")
        return cls.from_logs(*[list(x) for x in zip(*logs)], T=T, pre_steps=pre_steps, skip=skip)

    @classmethod
    def from_arrays(cls, obs, acs, pre_inputs):
        return cls(obs, acs, pre_inputs)

    def select(self, indices):
        """The mini-trajectories `indices` as a data set of their own (mini-batches)."""
        idx = np.asarray(indices, np.int64)
        return MiniTrajectories(self.observations[idx], self.actions[idx], self.pre_inputs[idx])

    def kernel_layout(self):
        """float32 host arrays in the layout pds_simopt_evaluate reads: actions [T, M, 4], observations [T, 3, M, 4] with row 0
        replaced by start_state(), pre_inputs [pre_steps, M, 4] -- every per-step load is 16 B per lane, coalesced."""
        M, T = len(self), self.mini_trajectory_size
        rows = self.observations.copy()
        rows[:, 0] = start_state(rows[:, 0])
        obs = rows.reshape(M, T, 3, 4).transpose(1, 2, 0, 3)
        return (np.ascontiguousarray(self.actions.transpose(1, 0, 2), np.float32), np.ascontiguousarray(obs, np.float32),
                np.ascontiguousarray(self.pre_inputs.transpose(1, 0, 2), np.float32))

    def to(self, device):
        """(actions, observations, pre_inputs) device tensors in the kernel's layout, made once per device."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in self.kernel_layout())
        return self._device[key]


class Candidates:
    """Parameter candidates prepared for the device: params [P, 3] float32, buf_size [P] int32 and its maximum.  Made by
    SimOptObjective.prepare; evaluate / losses / simulate accept it in place of an array, which keeps host work (and host to
    device copies) out of a captured graph."""

    def __init__(self, params, lat_steps, max_steps, host):
        self.params, self.lat_steps, self.max_steps, self.host = params, lat_steps, max_steps, host

    def __len__(self):
        return self.params.shape[0]


class SimOptObjective:
    """score(params) = mean over mini-trajectories of the discounted L1 + L2 mismatch between the replayed and the logged
    flight (simopt/pybullet.py:72-227).

    env_or_id: a DroneVecEnv whose configuration the objective uses (it must be the deterministic one: control_mode PWM, no
    thrust / observation noise, no domain randomisation; its state is not touched), or an env id -- then such an env is made,
    `aggregate_phy_steps` and `device` going to its constructor.
    """

    def __init__(self, env_or_id, data, gamma=0.95, fused=True, aggregate_phy_steps=1, device=None):
        from . import envs  # (needs torch; the module itself imports without)
        if isinstance(env_or_id, str):
            self.env = envs.make(env_or_id, num_envs=1, device=device, observation_noise=-1, domain_randomization=-1,
                                 motor_thrust_noise=0.0, enable_reset_distribution=False, use_motor_dynamics=True,
                                 aggregate_phy_steps=aggregate_phy_steps)
            self._env_id = env_or_id
        else:
            self.env = env_or_id
            self._env_id = next((i for i, (c, _) in envs.registry.items() if c is type(self.env)), 'DroneHoverSimpleEnv-v0')
        self.lib = self.env.lib
        self.device = self.env.device
        self.time_step = float(self.env.cfg.time_step)
        self.aggregate_phy_steps = int(self.env.cfg.aggregate_phy_steps)
        self.data = data
        self.gamma = float(gamma)
        self.fused = bool(fused)
        self.parameter_low, self.parameter_high = PARAMETER_LOW.copy(), PARAMETER_HIGH.copy()
        self.parameter_space = envs._box(self.parameter_low.astype(np.float32), self.parameter_high.astype(np.float32))
        self._composed = {}

    # ---- candidates ----
    def prepare(self, params):
        import torch
        if isinstance(params, Candidates):
            return params
        host = params.detach().cpu().numpy() if isinstance(params, torch.Tensor) else np.asarray(params)
        host = np.ascontiguousarray(host, np.float64).reshape(-1, 3)
        if host.shape[0] < 1:
            raise ValueError("no candidates")
        steps = latency_steps(np.clip(host[:, 2], 0, np.inf), self.time_step)
        return Candidates(torch.from_numpy(host.astype(np.float32)).to(self.device), torch.from_numpy(steps).to(self.device),
                          int(steps.max()), host)

    def _dataset(self, shrink=1, indices=None, shuffle=True):
        """The data the call runs on: `indices`, or (the reference's evaluate(shrink=...)) the first len // shrink entries of a
        shuffled index list."""
        if indices is None and shrink > 1:
            indices = np.arange(len(self.data))
            if shuffle:
                np.random.shuffle(indices)
            indices = indices[:len(self.data) // int(shrink)]
            if len(indices) < 1:
                raise ValueError(f"shrink = {shrink} leaves no mini-trajectory of {len(self.data)}")
        return self.data if indices is None else self.data.select(indices)

    # ---- public surface ----
    def evaluate(self, params, shrink=1, indices=None, shuffle=True):
        """[3] -> float, [P, 3] (array, tensor or Candidates) -> [P] device tensor of scores.  A caller that shards the
        candidates over devices passes each objective its slice: a score does not depend on the rest of the batch."""
        single = not isinstance(params, Candidates) and np.ndim(params) == 1
        _, score, _ = self._run(self.prepare(params), self._dataset(shrink, indices, shuffle), False)
        return float(score[0]) if single else score

    def losses(self, params, shrink=1, indices=None, shuffle=True):
        """[P, M]: evaluate_once of every (candidate, mini-trajectory)."""
        return self._run(self.prepare(params), self._dataset(shrink, indices, shuffle), False)[0]

    def simulate(self, params, indices=None):
        """[T - 1, P, M, 13]: xyz, quaternion, velocity, body rates after every replayed step."""
        return self._run(self.prepare(params), self._dataset(1, indices), True)[2]

    # ---- the two paths ----
    def _run(self, cand, data, want_sim):
        if cand.max_steps > native.MAX_LATENCY_STEPS and not self.fused:
            raise NotImplementedError(f"a candidate's latency is {cand.max_steps} time steps (limit {native.MAX_LATENCY_STEPS})")
        return self._run_fused(cand, data, want_sim) if self.fused else self._run_composed(cand, data, want_sim)

    def _run_fused(self, cand, data, want_sim):
        import torch
        acts, obs, pre = data.to(self.device)
        P, M, T = len(cand), len(data), data.mini_trajectory_size
        f32 = dict(dtype=torch.float32, device=self.device)
        loss, score = torch.empty(P, M, **f32), torch.empty(P, **f32)
        sim = torch.empty(T - 1, P, M, 13, **f32) if want_sim else None
        rc = self.lib.pds_simopt_evaluate(self.env._handle, P, cand.params.data_ptr(), cand.lat_steps.data_ptr(), cand.max_steps,
                                          M, T, data.pre_steps, self.gamma, acts.data_ptr(), obs.data_ptr(),
                                          pre.data_ptr() if data.pre_steps > 0 else None, loss.data_ptr(), score.data_ptr(),
                                          sim.data_ptr() if sim is not None else None, self.env._raw_stream())
        if rc != 0:
            native.check(self.env._handle, rc, "pds_simopt_evaluate")
        return loss, score, sim

    def motor_constants(self, cand):
        """update_motor_dynamics (envs/agents.py:208-224) in float64, rounded once: (A, K) [P] float32 -- the arithmetic of the
        kernel, for the composed path."""
        import torch
        p = cand.params.double().clamp(min=0.0)
        T = p[:, 1].clamp(min=self.time_step)
        return (1.0 - self.time_step / T).float(), (0.028 * G * p[:, 0] / 4).float()

    def _composed_env(self, n):
        """A handle whose per-env parameter arrays exist (domain randomisation on); every randomised field is overwritten."""
        from . import envs
        env = self._composed.get(n)
        if env is None:
            for old in self._composed.values():
                old.close()
            env = envs.make(self._env_id, num_envs=n, device=self.device, observation_noise=-1, domain_randomization=0.1,
                            motor_thrust_noise=0.0, enable_reset_distribution=False, use_motor_dynamics=True, auto_reset=False,
                            aggregate_phy_steps=self.aggregate_phy_steps, max_episode_steps=60000)
            env.reset()
            self._composed = {n: env}
        return env

    def _run_composed(self, cand, data, want_sim, max_envs=1 << 18):
        import torch
        acts, obs, pre = data.to(self.device)
        P, M, T = len(cand), len(data), data.mini_trajectory_size
        f32 = dict(dtype=torch.float32, device=self.device)
        loss = torch.empty(P, M, **f32)
        sim = torch.empty(T - 1, P, M, 13, **f32) if want_sim else None
        A, K = self.motor_constants(cand)
        steps = torch.from_numpy(latency_steps(np.clip(cand.host[:, 2], 0, np.inf), self.time_step))
        start = obs[0].permute(1, 0, 2).reshape(M, 12)  # x y z, xyz_dot, rpy, rpy_dot
        tgt = obs[1:].permute(0, 2, 1, 3).reshape(T - 1, 1, M, 12).double()
        disc = torch.tensor([self.gamma ** i for i in range(T - 1)], dtype=torch.float64, device=self.device)
        per = max(1, max_envs // M)
        # model constants as csrc/pds_api.hip fill_consts rounds them (envs/assets/cf21x_sys_eq.urdf)
        nominal = torch.tensor([self.time_step, 0.027, 1.7e-5, 1.7e-5, 2.9e-5, 5.96e-3], dtype=torch.float64).float()
        for b in sorted(set(steps.tolist())):
            group = torch.nonzero(steps == b).flatten()
            for c0 in range(0, len(group), per):
                idx = group[c0:c0 + per].to(self.device)
                Pg = len(idx)
                N = Pg * M
                env = self._composed_env(N)
                lat = (b + 0.5) * self.time_step if b > 0 else 0.0
                zeros4 = torch.zeros(N, 4, **f32)

                def clear(motor_x):
                    env.set_latency(lat)  # zeroes the delayed-action ring and its index
                    env.set_state("params", nominal.expand(N, 6))
                    env.set_state("motor_A", A[idx].repeat_interleave(M)[:, None].expand(N, 4))
                    env.set_state("motor_K", K[idx].repeat_interleave(M)[:, None].expand(N, 4))
                    env.set_state("motor_x", motor_x)
                    for name in ("last_action", "prev_action"):
                        env.set_state(name, zeros4)
                    for name in ("step_count", "quat_sign"):
                        env.set_state(name, torch.zeros(N, 1, dtype=torch.int32, device=self.device))

                # 1) pre-steps from a reset env (the pose does not reach the motor state)
                clear(zeros4)
                if data.pre_steps > 0:
                    env.step_k(pre[:, None].expand(data.pre_steps, Pg, M, 4).reshape(data.pre_steps, N, 4).contiguous())
                x = env.get_state("motor_x")
                # 2) + 3) the logged state, ring zeroed again, motor state kept
                clear(x)
                s = start[None].expand(Pg, M, 12).reshape(N, 12)
                env.set_state("pos", s[:, 0:3])
                env.set_state("vel", s[:, 3:6])
                env.set_state("rpy", s[:, 6:9])
                env.set_state("omega", s[:, 9:12])
                # 4) replay
                o = env.step_k(acts[:T - 1, None].expand(T - 1, Pg, M, 4).reshape(T - 1, N, 4).contiguous())[0]
                half = o.shape[-1] // 2
                so = o[:, :, half:half + 13].reshape(T - 1, Pg, M, 13)
                if sim is not None:
                    sim[:, idx] = so
                loss[idx] = self._loss_torch(so.double(), tgt, disc).float()
        score = loss.double().mean(1).float()
        return loss, score, sim

    @staticmethod
    def _loss_torch(so, tgt, disc):
        """loss_function + the discounted mean of evaluate_once (simopt/pybullet.py:166-227) in float64 torch."""
        import torch
        x, y, z, w = so[..., 3], so[..., 4], so[..., 5], so[..., 6]
        sarg = -2.0 * (x * z - w * y)
        roll = torch.atan2(2.0 * (y * z + w * x), w * w - x * x - y * y + z * z)
        pitch = torch.asin(sarg.clamp(-1.0, 1.0))
        yaw = torch.atan2(2.0 * (x * y + w * z), w * w + x * x - y * y - z * z)
        lo, hi = sarg <= -0.99999, sarg >= 0.99999
        zero = torch.zeros_like(roll)
        roll = torch.where(lo | hi, zero, roll)
        pitch = torch.where(lo, zero - 0.5 * np.pi, torch.where(hi, zero + 0.5 * np.pi, pitch))
        yaw = torch.where(lo, 2.0 * torch.atan2(x, -y), torch.where(hi, 2.0 * torch.atan2(-x, y), yaw))
        e = torch.cat([torch.stack([roll, pitch, yaw], -1) - tgt[..., 6:9], 100.0 * (so[..., 0:3] - tgt[..., 0:3]),
                       10.0 * (so[..., 7:10] - tgt[..., 3:6]), so[..., 10:13] - tgt[..., 9:12]], -1)
        L = e.abs().sum(-1) + e.pow(2).sum(-1).sqrt()
        return (L * disc[:, None, None]).mean(0)

    def close(self):
        for env in self._composed.values():
            env.close()
        self._composed = {}
