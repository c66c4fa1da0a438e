"""Case table, float64 references and the error measure for the kernels of include/pds_mlp_broad.h (two hidden layers with a width
above 64): shared by tests/test_gpu_ddpg_broad_kernels.py, tests/test_gpu_ddpg_broad_trainer.py and
profiles/tools/ddpg_broad_margins.py, which measured the units the tests' bars are built from
(profiles/ddpg_broad_parity_margins.txt).

The measure.  Per parameter tensor: max|x - want| / max|want|.  For the forward output and the Bellman target: per sample
|x - want| / (|want| + 1), the largest over the samples; for a sum over the batch (sum Q, the sum of squared errors):
|x - want| / (sum|want_g| + B).  `want` is float64 autograd of the reference's compute_loss_pi / compute_loss_q
(algs/ddpg/ddpg.py:316-340).  The UNIT of a quantity is that measure for torch's own float32 arithmetic (the fused=False path)
against float64, the largest over the whole case table; the bar is BAR_UNITS = 4 units (the project's margin for a device path
against float64, tests/flight_oracle.py: one more differently ordered float32 chain may sit a small multiple of another's distance
from float64), and never below FLOOR, the least the existing bars of tests/test_gpu_ddpg_kernels.py admit in this measure
(gradient: atol 2e-6 of the largest entry; forward and target: atol 2e-6 per sample)."""
from collections import namedtuple

import torch

import mlp_cases as mc

DEV = "cuda:0"
BAR_UNITS = 4.0
FLOOR = 2e-6
TENSORS = ("W1", "b1", "W2", "b2", "W3", "b3")

Shape = namedtuple("Shape", "name pi q pact qact")
SHAPES = [
    Shape("default", (400, 300), (400, 300), "relu", "relu"),       # the reference's default for DDPG
    Shape("one-over", (65, 64), (65, 64), "relu", "relu"),          # one unit over the old limit, one layer still narrow
    Shape("one-over-second", (64, 65), (64, 65), "tanh", "relu"),
    Shape("corner", (512, 512), (512, 512), "tanh", "tanh"),        # the range's corner
    Shape("odd-first", (300, 400), (300, 400), "relu", "tanh"),     # a width that is no multiple of 16, first
    Shape("mixed", (400, 300), (65, 512), "relu", "tanh"),          # actor and Q of different shapes
]
BATCHES = (1, 17, 128, 1000)  # a partial tile, one block of 16, several blocks; 1000 >= 512 runs the two-tile chain block and
                              # two parts of the weight-gradient sum
Case = namedtuple("Case", "shape D B index limit")


def _table():
    out = []
    for i, sh in enumerate(SHAPES):
        for j, B in enumerate(BATCHES):
            k = i + j  # every shape meets every B, both D, and an index of each kind
            out.append(Case(sh, (34, 60)[(j + i // 2) % 2], B, (None, "rep", "perm", "rep")[k % 4], (1.0, 0.5)[(k // 2) % 2]))
    return out


CASES = _table()


def case_id(c):
    return f"{c.shape.name}-D{c.D}-B{c.B}-{c.index}-lim{c.limit}"


# ---- the measure --------------------------------------------------------------------------------------------------------------
def tensor_error(x, want):
    """max|x - want| / max|want| (0 / inf when want is all zero)"""
    err, scale = float((x.double() - want).abs().max()), float(want.abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def sample_error(x, want):
    return float(((x.double() - want).abs() / (want.abs() + 1.0)).max())


def sum_error(x, want_terms):
    return abs(float(x) - float(want_terms.sum())) / (float(want_terms.abs().sum()) + want_terms.numel())


def split_flat(flat, net):
    """the flat gradient (torch parameter order) -> {W1, b1, ...}"""
    out, off = {}, 0
    for name, p in zip(TENSORS, net.parameters()):
        out[name] = flat[off:off + p.numel()]
        off += p.numel()
    return out


def bar(units, key):
    return max(BAR_UNITS * units[key], FLOOR)


# ---- nets and inputs ----------------------------------------------------------------------------------------------------------
def nets(c, seed=0, broad=True):
    from phoenix_drone_simulation_amd.fused import FusedMLP
    sh = c.shape
    pi = mc.make_net(c.D, sh.pi[0], sh.pi[1], 4, sh.pact, seed)
    q = mc.make_net(c.D + 4, sh.q[0], sh.q[1], 1, sh.qact, seed + 1)
    return pi, q, FusedMLP(pi, sh.pact, broad=broad), FusedMLP(q, sh.qact, broad=broad)


def rows(c, seed=3):
    """-> oa [rows, D + 4], obs2 [rows, D], rew, done [rows], index or None"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = c.B if c.index is None else 2 * c.B + 3
    oa = torch.randn(n, c.D + 4, device=DEV, generator=g)
    obs2 = torch.randn(n, c.D, device=DEV, generator=g)
    rew = torch.randn(n, device=DEV, generator=g)
    done = (torch.rand(n, device=DEV, generator=g) < 0.3).float()
    idx = None if c.index is None else mc.make_index(c.index, n, c.B, seed + 1)
    return oa, obs2, rew, done, idx


def _take(t, idx):
    return t if idx is None else t[idx]


def _flat_grad(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


def policy_grad_ref(pi, q, oa, idx, D, limit, dtype):
    """autograd of compute_loss_pi in `dtype` on copies of the nets -> (flat actor gradient, Q values)"""
    import copy
    p, qq = copy.deepcopy(pi).to(dtype), copy.deepcopy(q).to(dtype)
    o = _take(oa, idx)[:, :D].to(dtype)
    qv = qq(torch.cat([o, limit * torch.tanh(p(o))], dim=-1)).squeeze(-1)
    (-qv.mean()).backward()
    return _flat_grad(p), qv.detach()


def value_grad_ref(q, oa, target_rows, idx, dtype):
    """autograd of mse_loss(q(oa[idx]), target[idx]) in `dtype` -> (flat gradient, squared errors)"""
    import copy
    qq = copy.deepcopy(q).to(dtype)
    v = qq(_take(oa, idx).to(dtype)).squeeze(-1)
    se = (v - _take(target_rows, idx).to(dtype)) ** 2
    se.mean().backward()
    return _flat_grad(qq), se.detach()


def forward_ref(net, x, idx, mean, std, eps, dtype):
    import copy
    n = copy.deepcopy(net).to(dtype)
    xs = _take(x, idx).to(dtype)
    if mean is not None:
        xs = (xs - mean.to(dtype)) / (std.to(dtype) + eps)
    with torch.no_grad():
        return n(xs)


def target_ref(pi, q, obs2, rew, done, gamma, limit, dtype):
    """the Bellman backup of compute_loss_q for EVERY row, in `dtype`"""
    import copy
    p, qq = copy.deepcopy(pi).to(dtype), copy.deepcopy(q).to(dtype)
    with torch.no_grad():
        o = obs2.to(dtype)
        qv = qq(torch.cat([o, limit * torch.tanh(p(o))], dim=-1)).squeeze(-1)
        return rew.to(dtype) + gamma * (1 - done.to(dtype)) * qv


def standardisation(c, seed=9):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(c.D, device=DEV, generator=g), torch.rand(c.D, device=DEV, generator=g) + 0.5


# ---- one case, every quantity: {quantity: (kernel error, float32-torch error)} --------------------------------------------------
def measure(c):
    from phoenix_drone_simulation_amd.fused import ddpg_target
    pi, q, fpi, fq = nets(c)
    oa, obs2, rew, done, idx = rows(c)
    out = {}
    # policy gradient and sum Q
    st = fpi.ddpg_policy_grad(fq, oa, idx, c.limit).clone()
    got = split_flat(fpi.flat_grad.clone(), pi)
    want, qv = policy_grad_ref(pi, q, oa, idx, c.D, c.limit, torch.float64)
    f32, qv32 = policy_grad_ref(pi, q, oa, idx, c.D, c.limit, torch.float32)
    for name in TENSORS:
        out["pi_grad." + name] = (tensor_error(got[name], split_flat(want, pi)[name]), tensor_error(split_flat(f32, pi)[name], split_flat(want, pi)[name]))
    out["sum_q"] = (sum_error(st[0].double(), qv), sum_error(qv32.double().sum(), qv))
    # value gradient and the sum of squared errors
    target_rows = torch.randn(oa.shape[0], device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    st = fq.value_grad(oa, target_rows, index=idx).clone()
    got = split_flat(fq.flat_grad.clone(), q)
    want, se = value_grad_ref(q, oa, target_rows, idx, torch.float64)
    f32, se32 = value_grad_ref(q, oa, target_rows, idx, torch.float32)
    for name in TENSORS:
        out["q_grad." + name] = (tensor_error(got[name], split_flat(want, q)[name]), tensor_error(split_flat(f32, q)[name], split_flat(want, q)[name]))
    out["sum_sq_err"] = (sum_error(st[0].double(), se), sum_error(se32.double().sum(), se))
    # forward (the actor, standardised input) and the Bellman target
    mean, std = standardisation(c)
    y = fpi.forward(oa[:, :c.D].contiguous(), index=idx, mean=mean, std=std)
    want = forward_ref(pi, oa[:, :c.D], idx, mean, std, 1e-5, torch.float64)
    out["forward"] = (sample_error(y, want), sample_error(forward_ref(pi, oa[:, :c.D], idx, mean, std, 1e-5, torch.float32), want))
    sel = torch.ones_like(done, dtype=torch.bool) if idx is None else torch.zeros_like(done, dtype=torch.bool).index_fill_(0, idx, True)
    t = torch.full_like(rew, 7.0)
    ddpg_target(fpi, fq, obs2, idx, rew, done, 0.99, c.limit, t)
    want = target_ref(pi, q, obs2, rew, done, 0.99, c.limit, torch.float64)
    out["target"] = (sample_error(t[sel], want[sel]), sample_error(target_ref(pi, q, obs2, rew, done, 0.99, c.limit, torch.float32)[sel], want[sel]))
    return out


QUANTITIES = ["pi_grad." + n for n in TENSORS] + ["sum_q"] + ["q_grad." + n for n in TENSORS] + ["sum_sq_err", "forward", "target"]


# ---- the trainer: three updates on fixed indices ----------------------------------------------------------------------------
TRAINER_HIDDEN = (400, 300)


def trainer(fused, broad_fused, hidden=TRAINER_HIDDEN, state=None, seed=0):
    """DDPGTrainer on Hover, 64 envs, mini-batch 128, a ring of 4096 random rows (the same for every trainer)"""
    import phoenix_drone_simulation_amd as pds
    from phoenix_drone_simulation_amd.ddpg import DDPGTrainer
    env = pds.make("DroneHoverSimpleEnv-v0", num_envs=64, seed=1)
    kw = {"pi": {"hidden_sizes": hidden}, "q": {"hidden_sizes": hidden}}
    tr = DDPGTrainer(env, ac_kwargs=kw, seed=seed, fused=fused, broad_fused=broad_fused, buffer_size=4096, mini_batch_size=128)
    if state is not None:
        with torch.no_grad():  # in place: the fused views point at these tensors
            for net in (tr.ac, tr.ac_targ):
                for k, v in net.state_dict().items():
                    v.copy_(state[k])
    g = torch.Generator(device=env.device).manual_seed(1)
    b = tr.buffer
    b.oa.copy_(torch.randn(b.oa.shape, device=env.device, generator=g))
    b.oa[:, tr.D:].clamp_(-1.0, 1.0)
    b.obs2.copy_(torch.randn(b.obs2.shape, device=env.device, generator=g))
    b.rew.copy_(torch.randn(b.capacity, device=env.device, generator=g))
    b.done.copy_((torch.rand(b.capacity, device=env.device, generator=g) < 0.05).float())
    b.size = b.capacity
    return tr


def trainer_indices(n=3, B=128, rows=4096):
    g = torch.Generator(device=DEV).manual_seed(21)
    return [torch.randint(0, rows, (B,), device=DEV, generator=g) for _ in range(n)]


def updated(tr, indices):
    for idx in indices:
        tr.update(idx)
    return {k: v.detach().clone() for k, v in tr.ac.state_dict().items()}


def float64_updates(tr, state, indices):
    """the reference's update (ddpg.autograd_update) in float64 from `state` on the trainer's ring -> state_dict"""
    from copy import deepcopy
    from phoenix_drone_simulation_amd import ddpg
    ac = ddpg.DDPGActorCritic(tr.D, tr.env.act_dim, tr.ac.ac_kwargs, tr.act_limit).to(DEV)
    ac.load_state_dict(state)
    ac = ac.double()
    ac_targ = deepcopy(ac)
    for p in ac_targ.parameters():
        p.requires_grad = False
    pi_opt = torch.optim.Adam(ac.pi.parameters(), lr=tr.pi_lr)
    q_opt = torch.optim.Adam(ac.q.parameters(), lr=tr.q_lr)
    for idx in indices:
        data = {k: v.double() for k, v in tr.buffer.batch(idx).items()}
        ddpg.autograd_update(ac, ac_targ, pi_opt, q_opt, data, tr.gamma, tr.polyak)
    return {k: v.detach().clone() for k, v in ac.state_dict().items()}
