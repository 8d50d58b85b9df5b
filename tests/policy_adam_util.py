"""Shared cases of the device learner step's tests (test_policy_adam_cpu.py,
test_policy_adam_gpu.py): the nets and gradients of the Adam comparison and
the rows of the loss comparison, built from seeds so that every device sees
the same numbers."""
import numpy as np
import torch

GROUPS = 9            # x 4 nets of >= 10 tensors each: more descriptors than one launch carries (64)
IDLE_GROUP = 3        # rows == 0: untouched
SHARED_GROUP = 1      # one net for all four species
STEPS = 3
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


def make_net(mb, rng, H, device, memory=False, unaligned=False):
    """A PolicyNet over fresh leaf tensors: H = 16 with one trunk layer, or
    (memory) H = 48 with memory_in (85 inputs), a memory head and a gate.
    unaligned: the first trunk weight lies 4 bytes into its storage."""
    def P(*shape):
        a = torch.from_numpy((rng.standard_normal(shape) * 0.1).astype(np.float32))
        if unaligned and len(shape) == 2 and shape[1] in (69, 85):
            base = torch.zeros(a.numel() + 1, device=device)
            base[1:] = a.reshape(-1).to(device)
            t = base[1:].view(*shape).detach()
            assert t.data_ptr() % 16 == 4
            return t.requires_grad_()
        return a.to(device).requires_grad_()
    trunk = [(P(H, 85 if memory else 69), P(H), 3)]
    actor = [(P(H, H), P(H), 0), (P(6, H), P(6), 0)]
    critic = [(P(H, H), P(H), 0), (P(1, H), P(1), 0)]
    if not memory:
        return mb.PolicyNet(trunk, actor, critic)
    return mb.PolicyNet(trunk, actor, critic, (P(16, H), P(16), 0), True, (P(16, H), P(16), 0))


def make_groups(mb, device, seed=7):
    """GROUPS groups of nets: group 0 mixes both architectures, group
    SHARED_GROUP is one net for all four species, group 2 holds the unaligned
    tensor; the others four H = 16 nets each."""
    rng = np.random.default_rng(seed)
    groups = []
    for u in range(GROUPS):
        if u == 0:
            groups.append([make_net(mb, rng, 16, device), make_net(mb, rng, 48, device, memory=True),
                           make_net(mb, rng, 16, device), make_net(mb, rng, 48, device, memory=True)])
        elif u == SHARED_GROUP:
            groups.append(make_net(mb, rng, 16, device))
        else:
            groups.append([make_net(mb, rng, 16, device, unaligned=(u == 2 and s == 1)) for s in range(4)])
    return groups


def gradients(opt, step, seed=11):
    """Step `step`'s gradient of every parameter as float32 numpy: normal
    numbers of many magnitudes; parameter 0 all zeros (of both signs);
    parameter 1 with subnormal squares; parameter 5 None at step 1 (skipped)."""
    rng = np.random.default_rng(seed + 1000 * step)
    out = []
    for i, p in enumerate(opt.params):
        g = (rng.standard_normal(p.numel()) * 10.0 ** rng.integers(-6, 2, p.numel())).astype(np.float32)
        if i == 0:
            g[:] = 0.0
            g[::3] = -0.0
        elif i == 1:
            g *= np.float32(1e-22)
        out.append(None if i == 5 and step == 1 else g.reshape(tuple(p.shape)))
    return out


def set_gradients(opt, grads):
    """Bind the numpy gradients as .grad; an unaligned parameter gets an
    unaligned gradient too."""
    for p, g in zip(opt.params, grads):
        if g is None:
            p.grad = None
            continue
        t = torch.from_numpy(g).to(p.device)
        if p.data_ptr() % 16:
            base = torch.zeros(t.numel() + 1, device=p.device)
            base[1:] = t.reshape(-1)
            t = base[1:].view(p.shape)
        p.grad = t


def rows_of(device):
    rows = torch.arange(1, GROUPS + 1, dtype=torch.int64)
    rows[IDLE_GROUP] = 0
    return rows.to(device)


def run_adam(mb, device):
    """STEPS steps of PolicyAdam on `device`; returns the optimiser and, per
    step, (params, state_dict) as CPU copies -- and the parameters before."""
    opt = mb.PolicyAdam(make_groups(mb, device), **HYPER)
    before = [p.detach().cpu().clone() for p in opt.params]
    rows = rows_of(device)
    trace = []
    for k in range(STEPS):
        set_gradients(opt, gradients(opt, k))
        opt.step(rows)
        sd = {key: t.cpu() for key, t in opt.state_dict().items()}
        trace.append(([p.detach().cpu().clone() for p in opt.params], sd))
    return opt, before, trace


def slices(opt, flat):
    """The parameters' slices of a state_dict's m or v, as numpy."""
    flat = flat.numpy()
    return [flat[o:o + p.numel()].reshape(tuple(p.shape)) for o, p in zip(opt.offsets, opt.params)]


# ---- the loss ----
LOSS_G = 3
LOSS_N = 2600


def loss_case(seed=3):
    """(columns, end, segments, rows): G = 3 over 2600 rows -- group 0 with a
    257-row segment (past one round of the accumulators), an empty one, a
    1-row one and 41 rows; rows 299..310 in no segment; group 1 with 30 rows,
    a segment of exactly 2 x 256 and one of 1298 (past the 4 x 256 rows a
    block of the kernel has in flight); group 2 with rows == 0 (scale 0)
    although it has segments; the rows from 2260 on in no segment.  END_RESET
    rows are spread through all of it."""
    rng = np.random.default_rng(seed)
    cols = [(rng.standard_normal(LOSS_N) * s).astype(np.float32) for s in (2.0, 5.0, 1.0, 3.0, 5.0)]
    end = rng.integers(0, 4, LOSS_N).astype(np.int32)
    segments = np.array([[[0, 257], [257, 257], [257, 258], [258, 299]],
                         [[310, 340], [340, 340], [340, 852], [852, 2150]],
                         [[2200, 2210], [2210, 2210], [2210, 2260], [2260, 2260]]], np.int32)
    rows = np.array([299, 1840, 0], np.int64)
    return cols, end, segments, rows
