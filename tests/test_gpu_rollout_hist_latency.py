"""pds_rollout_history_latency (include/pds_history_latency.h): the reference's experiments/04_history_of_state_action_inputs
(observation_history_size 1 .. 8) crossed with the latency of experiments/07_control_structures is one launch per rollout on an env
created with history_latency=True, bit for bit the per-step rollout (step_once on the ring in memory, the views of the ring's last
row resolved in the env wave), and what is not built is refused before the handle is touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HOVER, CIRCLE, TAKEOFF = "DroneHoverSimpleEnv-v0", "DroneCircleSimpleEnv-v0", "DroneTakeOffSimpleEnv-v0"
LEAN = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0)
RING = dict(use_latency=True, history_latency=True)

# every input width (<= 64 / 96 / 128 / 192 inputs) and every translation unit (pds_rollout_hist_{hover,circle}[_pid]_lat.hip),
# lean and full noise, with and without motor dynamics, rings of 1, 2 and 3 rows, 1 and 2 sub-steps, H = 1 (no shift)
CASES = [
    (HOVER, dict(RING, latency=0.02, observation_history_size=4), 200),                                             # 68 inputs, full
    (CIRCLE, dict(RING, **LEAN, latency=0.03, control_mode="Attitude", aggregate_phy_steps=2, use_motor_dynamics=True,
                  observation_history_size=8), 130),                                                                 # 160, lean
    (CIRCLE, dict(RING, latency=0.02, control_mode="AttitudeRate", observation_history_size=3), 64 * 5 - 3),        # 60, full
    (HOVER, dict(RING, **LEAN, latency=0.035, control_mode="AttitudeRate", use_motor_dynamics=True,
                 observation_history_size=6), 64 * 300),                                                             # 102, > 256 tiles
    (HOVER, dict(RING, **LEAN, latency=0.015, observation_history_size=1), 130),                                    # 21, lean
    (CIRCLE, dict(RING, **LEAN, latency=0.025, observation_history_size=4), 130),                                   # 80, the PWM unit of Circle
]


@pytest.mark.parametrize("task,kw,n", CASES)
def test_fused_history_rollout_equals_per_step_rollout_bitwise_on_the_ring(task, kw, n, monkeypatch):
    """every rollout buffer, the env's own history and state, V(final history) where pds_gae reads it, over two consecutive
    rollouts with episodes of 9 steps (the helper asserts fused_rollout is True on the one-launch side) -- and, read off the two
    envs as the helper closes them, the ring, its index and the step counts of the rule"""
    import phoenix_drone_simulation_amd as pds
    from test_trainer import _fused_rollout_against_per_step_rollout
    seen = []
    make = pds.make

    def make_and_watch(*a, **k):
        env = make(*a, **k)
        close = env.close

        def close_and_keep():
            if env._handle:
                seen.append({f: env.get_state(f).clone() for f in ("action_buffer", "action_idx", "step_count")})
                seen[-1]["hist_steps"] = env._hist_steps.clone()
            close()
        env.close = close_and_keep
        return env
    monkeypatch.setattr(pds, "make", make_and_watch)
    _fused_rollout_against_per_step_rollout(task, kw, n, rollouts=2)
    assert len(seen) == 2
    for f in seen[0]:
        assert torch.equal(seen[0][f], seen[1][f]), f
    assert torch.equal(seen[0]["hist_steps"], seen[0]["step_count"].view(-1).to(torch.int32))


def test_three_epochs_of_learning_leave_the_same_parameters():
    """three epochs of learn() on Circle AttitudeRate on the ring with H = 4 leave every actor and critic parameter bit for bit
    where the per-step rollout leaves it"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    mk = lambda fr: PPOTrainer(pds.make(CIRCLE, num_envs=256, seed=3, control_mode="AttitudeRate", observation_history_size=4,  # noqa: E731
                                        latency=0.02, **RING),
                               rollout_len=16, epochs=3, train_pi_iterations=4, train_v_iterations=1, seed=5, fused_rollout=fr)
    a, b = mk(FUSED_BY_DEFAULT), mk(False)
    a.learn(); b.learn()
    torch.cuda.synchronize()
    assert a.fused_rollout is True and b.fused_rollout is False
    for (ka, pa), (kb, pb) in zip(a.ac.state_dict().items(), b.ac.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb), ka
    a.env.close(); b.env.close()


FUSED_BY_DEFAULT = None  # (None: the trainer finds the one-launch rollout by itself)


@pytest.mark.parametrize("task,kw", [
    (TAKEOFF, dict(latency=0.035)),                                       # TakeOff on the ring
    (HOVER, dict(latency=0.025, observation_frequency=50)),               # Kalman hold
    (HOVER, dict(latency=0.025, use_ground_effect=True)),                 # ground effect
    (CIRCLE, dict(latency=0.025, motor_thrust_noise=0)),                  # partial noise
])
def test_the_one_launch_entry_still_refuses_and_leaves_the_handle_untouched(task, kw):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.fused import rollout_history_latency_supported
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    env = pds.make(task, num_envs=128, seed=3, observation_history_size=4, **RING, **kw)
    assert not rollout_history_latency_supported(env)
    tr = PPOTrainer(env, rollout_len=4, epochs=2, seed=5, fused=True, fused_rollout=True)
    before = dict(tick=env.tick, **{f: env.get_state(f).clone() for f in ("pos", "action_buffer", "action_idx")})
    with pytest.raises(NotImplementedError):
        tr.roll_out()
    assert env.tick == before["tick"] and all(torch.equal(env.get_state(f), before[f]) for f in ("pos", "action_buffer", "action_idx"))
    env.close()
    # ... and the trainer left to itself steps such an env per step
    env = pds.make(task, num_envs=128, seed=3, observation_history_size=4, **RING, **kw)
    tr = PPOTrainer(env, rollout_len=4, epochs=2, seed=5, fused=True, graph_rollout=False)
    tick = env.tick
    tr.roll_out()
    assert tr.fused_rollout is False and env.tick == tick + 4
    env.close()


def test_the_plain_entry_and_a_frozen_env_are_answered_as_before():
    """the queries of the plain entry points answer a ring handle as they did (the switch is the new entry point, not a new answer
    of the old ones); after set_latency in the middle of an episode the views are frozen, which the kernel's step count does not know:
    rollout_history_latency_supported is False until the next full reset"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.fused import rollout_history_latency_supported
    env = pds.make(HOVER, num_envs=64, seed=1, observation_history_size=4, latency=0.025, **RING)
    env.reset()
    assert rollout_history_latency_supported(env) and env.lib.pds_evaluate_history_supported(env._handle, 4) == 0
    env.step(torch.zeros(64, 4, device=env.device))
    env.set_latency(0.015)
    assert not rollout_history_latency_supported(env)
    env.reset()
    assert rollout_history_latency_supported(env)
    env.close()
    plain = pds.make(HOVER, num_envs=64, seed=1, observation_history_size=4)
    assert not rollout_history_latency_supported(plain)  # (no switch, no ring)
    plain.close()
