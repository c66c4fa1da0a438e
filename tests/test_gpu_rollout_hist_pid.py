"""pds_rollout_history under the PID control modes: the reference's experiments/04_history_of_state_action_inputs
(observation_history_size 1 .. 8) crossed with experiments/07_control_structures (AttitudeRate / Attitude) is one launch per
rollout, bit for bit the per-step rollout (step_once with the PID state in the env wave's registers: the device functions of
pds_step), and what is not built is refused before the handle is touched."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HOVER, CIRCLE = "DroneHoverSimpleEnv-v0", "DroneCircleSimpleEnv-v0"
LEAN = dict(observation_noise=-1, domain_randomization=-1, motor_thrust_noise=0)

# every input-tile count the kernel is built for (<= 64 / 96 / 128 / 192 inputs), both modes, both tasks, lean and full noise,
# with and without motor dynamics, H = 1 (no shift), 16-byte aligned halves (Circle 20) and unaligned ones (Hover 17)
CASES = [
    (HOVER, dict(control_mode="AttitudeRate", aggregate_phy_steps=4, observation_history_size=4), 200),           # 68 inputs, full
    (CIRCLE, dict(LEAN, control_mode="Attitude", aggregate_phy_steps=2, use_motor_dynamics=True,
                  observation_history_size=8), 130),                                                               # 160, lean
    (CIRCLE, dict(control_mode="AttitudeRate", observation_history_size=3), 64 * 5 - 3),                           # 60, full
    (HOVER, dict(LEAN, control_mode="Attitude", use_motor_dynamics=True, observation_history_size=6), 64 * 300),   # 102, > 256 tiles
    (HOVER, dict(LEAN, control_mode="AttitudeRate", observation_history_size=1), 130),                             # 17, lean
]


@pytest.mark.parametrize("task,kw,n", CASES)
def test_fused_history_rollout_equals_per_step_rollout_bitwise_pid(task, kw, n):
    """every rollout buffer, the env's own history and state, V(final history) where pds_gae reads it: over two consecutive
    rollouts with short episodes (the helper asserts fused_rollout is True on the one-launch side)"""
    from test_trainer import _fused_rollout_against_per_step_rollout
    _fused_rollout_against_per_step_rollout(task, kw, n, rollouts=2)


def test_trainer_takes_the_one_launch_history_rollout_under_a_pid_mode():
    """PPOTrainer finds the one-launch rollout by itself (fused_rollout=None) on Circle AttitudeRate with H = 4, and three
    epochs of learn() leave every actor and critic parameter bit for bit where the per-step rollout leaves it."""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    mk = lambda fr: PPOTrainer(pds.make(CIRCLE, num_envs=256, seed=3, control_mode="AttitudeRate", observation_history_size=4),
                               rollout_len=16, epochs=3, train_pi_iterations=4, train_v_iterations=1, seed=5, fused_rollout=fr)
    a, b = mk(None), mk(False)
    a.learn(); b.learn()
    torch.cuda.synchronize()
    assert a.fused_rollout is True and b.fused_rollout is False
    for (ka, pa), (kb, pb) in zip(a.ac.state_dict().items(), b.ac.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb), ka
    a.env.close(); b.env.close()


@pytest.mark.parametrize("task,kw", [
    (CIRCLE, dict(control_mode="AttitudeRate", motor_thrust_noise=0)),       # partial noise
    (HOVER, dict(control_mode="AttitudeRate", observation_frequency=50)),    # Kalman hold
    (HOVER, dict(control_mode="AttitudeRate", use_ground_effect=True)),      # ground effect
])
def test_history_rollout_still_refuses_and_leaves_the_handle_untouched_pid(task, kw):
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ppo import PPOTrainer
    env = pds.make(task, num_envs=128, seed=3, observation_history_size=4, **kw)
    tr = PPOTrainer(env, rollout_len=4, epochs=2, seed=5, fused=True, fused_rollout=True)
    tick, pos = env.tick, env.get_state("pos").clone()
    with pytest.raises(NotImplementedError):
        tr.roll_out()
    assert env.tick == tick and torch.equal(env.get_state("pos"), pos)
    env.close()
