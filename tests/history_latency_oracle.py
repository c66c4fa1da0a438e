"""The reference env with observation_history_size = H on the latency ring, rebuilt around ONE env of the CPU oracle.  TEST
INFRASTRUCTURE: tests/test_history_latency_cpu.py holds it against the reference's own trajectories (tests/golden/history_latency.npz)
and against the closed-form rule the device implements; tests/test_gpu_history_latency.py holds the device against it.

Nothing here comes from phoenix_drone_simulation_amd, and nothing here knows the closed-form rule.  The oracle keeps H = 2: a row
of two halves [o, u].  This wrapper keeps what DroneBaseEnv keeps (envs/base.py:137, 303-319, 417-431): a deque of H observations
and a deque of H action entries.  An action entry is an array -- a copy, as apply_action leaves last_action (envs/agents.py:264) --
or the marker VIEW: the reference's `self.action_buffer[-1, :]` (envs/agents.py:386), a numpy view, which is what reset() leaves
in last_action and what DroneBaseEnv.reset puts H times into action_history.  A VIEW is resolved when the history is read, by
reading the oracle's action_buffer[buf_size - 1] at that moment: the reference's mechanism, whatever apply_action has written there
meanwhile.  set_latency allocates a NEW ring (envs/agents.py:403): the views keep the old array, which nothing writes any more, so
they become its values as they stand."""
from collections import deque

import numpy as np

from oracle import oracle

VIEW = "view of action_buffer[-1]"


class HistoryLatencyEnv:
    def __init__(self, task, H, precision="f64", **kwargs):
        self.env = oracle.OracleEnv(task, precision, **kwargs)
        self.H = int(H)
        self.half = self.env.obs_dim // 2
        self.obs_history = deque(maxlen=self.H)
        self.action_history = deque(maxlen=self.H)
        self.last_action = None
        self.row = None  # the oracle's own H = 2 row of the last reset / step

    # ---- the ring ----
    @property
    def buf_size(self):
        return int(self.env.get("buf_size"))

    def ring_last_row(self):
        return np.array(self.env.get("action_buffer")[self.buf_size - 1])

    def _entry(self, a):
        return self.ring_last_row() if a is VIEW else a

    # ---- envs/base.py:303-319 ----
    def _compute_history(self, obs_next):
        self.obs_history.append(obs_next)
        history = np.concatenate([np.concatenate([o, self._entry(a)]) for o, a in zip(self.obs_history, self.action_history)])
        self.action_history.append(self.last_action)
        return history

    def reset(self, sample=None):
        self.row = row = self.env.reset(sample)
        o = self.half - 4
        self.last_action = VIEW  # agents.py:386 (TakeOff writes -1 THROUGH it, takeoff.py:212; Hover / Circle point it at the new ring)
        for _ in range(self.H):
            self.obs_history.append(row[:o])
            self.action_history.append(self.last_action)
        return self._compute_history(row[self.half:self.half + o])

    def step(self, action):
        self.row, r, term, trunc, cost = self.env.step(action)
        self.last_action = np.array(action, dtype=self.row.dtype)  # agents.py:264, the RAW action (control.act clips its own copy)
        history = self._compute_history(self.row[self.half:2 * self.half - 4])
        return history, r, term, trunc, cost

    def set_latency(self, new_latency):
        old = self.ring_last_row()
        if not new_latency < self.env.cfg.time_step:  # agents.py:399-404: a new array; the views stay with the old one
            self.action_history = deque([old.copy() if a is VIEW else a for a in self.action_history], maxlen=self.H)
            if self.last_action is VIEW:
                self.last_action = old.copy()
        self.env.set_latency(new_latency)


def fixture_kwargs(g, name, task):
    """the oracle's keywords of one trajectory of tests/golden/history_latency.npz"""
    kw = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0.0, enable_reset_distribution=0, use_latency=1,
              latency=float(g[name + "_latency"]), max_episode_steps=int(g[name + "_max_steps"]))
    if task != "takeoff":
        kw["aggregate_phy_steps"] = int(g[name + "_agg"])
    return kw


def fly(env, actions, set_latency_at=-1, set_latency=0.0, reset_sample=None):
    """reset, then step `actions` [T, 4] with a reset behind every finished episode (the generator's loop).  Returns a dict: obs0,
    obs [T, H half], reward, terminated, truncated, cost, reset_obs [T, H half] (zero where no reset), and what the closed-form rule
    is fed with -- row0 / rows [T, 2 half] / reset_rows [T, 2 half], the oracle's own H = 2 rows -- and buf_size [T]."""
    T = len(actions)
    out = dict(obs0=env.reset(reset_sample() if reset_sample else None), row0=env.row.copy())
    keys = ("obs", "reward", "terminated", "truncated", "cost", "reset_obs", "rows", "reset_rows", "buf_size")
    log = {k: [] for k in keys}
    for t in range(T):
        if t == set_latency_at:
            env.set_latency(set_latency)
        h, r, te, tr, c = env.step(actions[t])
        log["obs"].append(h); log["reward"].append(r); log["terminated"].append(te); log["truncated"].append(tr); log["cost"].append(c)
        log["rows"].append(env.row.copy()); log["buf_size"].append(env.buf_size)
        if te or tr:
            log["reset_obs"].append(env.reset(reset_sample() if reset_sample else None))
            log["reset_rows"].append(env.row.copy())
        else:
            log["reset_obs"].append(np.zeros_like(h)); log["reset_rows"].append(np.zeros_like(env.row))
    out.update({k: np.array(v) for k, v in log.items()})
    return out
