"""Shared cases of the recurrent device update's tests
(test_policy_seq_loss_cpu.py, test_policy_clip_cpu.py,
test_policy_seq_update_gpu.py), built from seeds so that every device sees the
same numbers, and the raw calls of mbots_policy_adam / mbots_policy_adam_clip
over tensors of any length."""
import ctypes

import numpy as np
import torch

# ---- the sequence loss ----
SEQ_L, SEQ_G, SEQ_B = 3, 3, 2400
LAST_TABLE = 4
DEAD_GROUP = 2        # no kept element under LAST_TABLE: rows == 0
# columns per (group, species): one pair of 1100 (the 256 accumulators wrap four times and the 4 x 256 columns a
# block has in flight are exceeded), an empty one, one of 257, one of 1; 246 columns with no net
PAIRS = [[1100, 0, 257, 1], [300, 256, 100, 50], [40, 30, 0, 20]]
OUTSIDE = [-1, -7, 12, 13, 99, 2 ** 31 - 1]


def seq_case(seed=5):
    """dict of numpy arrays: net_id, length, t0, end int32 [B] and logp,
    value, entropy, adv, ret float32 [L, B].  Lengths 0..L and every end code
    all through; t0 0..5, so that LAST_TABLE = 4 cuts columns at every depth;
    DEAD_GROUP's columns are of length 0, a reset's single row, or start at
    LAST_TABLE or later."""
    rng = np.random.default_rng(seed)
    ids = [4 * g + s for g in range(SEQ_G) for s in range(4) for _ in range(PAIRS[g][s])]
    ids += [OUTSIDE[i % len(OUTSIDE)] for i in range(SEQ_B - len(ids))]
    net_id = np.array(ids, np.int64)[rng.permutation(SEQ_B)].astype(np.int32)
    length = rng.integers(0, SEQ_L + 1, SEQ_B).astype(np.int32)
    t0 = rng.integers(0, 6, SEQ_B).astype(np.int32)
    end = rng.integers(0, 4, SEQ_B).astype(np.int32)
    dead = np.nonzero((net_id >= 4 * DEAD_GROUP) & (net_id < 4 * DEAD_GROUP + 4))[0]
    for j, b in enumerate(dead):
        if j % 3 == 0:
            length[b] = 0
        elif j % 3 == 1:
            length[b], end[b], t0[b] = 1, 2, 0
        else:
            t0[b] = LAST_TABLE + j % 2
    case = dict(net_id=net_id, length=length, t0=t0, end=end)
    for name, scale in (("logp", 2.0), ("value", 5.0), ("entropy", 1.0), ("adv", 3.0), ("ret", 5.0)):
        case[name] = (rng.standard_normal((SEQ_L, SEQ_B)) * scale).astype(np.float32)
    return case


def seq_tensors(case, device):
    return {k: torch.from_numpy(v).to(device) for k, v in case.items()}


def seq_run(mb, case, device, last_table, loss=None):
    """(order, segments, rows, g_logp, g_value, g_entropy, loss) of the three
    calls on `device`, as CPU numpy."""
    c = seq_tensors(case, device)
    order, seg = mb.sequence_segments(c["net_id"], SEQ_G)
    rows = mb.sequence_group_rows(c["length"], c["t0"], c["end"], order, seg,
                                  torch.zeros(SEQ_G, dtype=torch.int64, device=device), last_table)
    if loss is not None:
        loss = torch.from_numpy(loss.copy()).to(device)
    out = mb.a2c_loss_sequences(c["logp"], c["value"], c["entropy"], c["adv"], c["ret"], c["length"], c["t0"],
                                c["end"], order, seg, rows, last_table, 0.5, 0.01, loss=loss)
    return tuple(x.cpu().numpy() for x in (order, seg, rows) + tuple(out))


# ---- the clipped Adam ----
CLIP_SIZES = [1, 3, 1023, 1024, 1025, 4100]
CLIP_TENSORS = 70     # more descriptors than one launch carries (64)
CLIP_GROUPS = 4
CLIPPED, UNCLIPPED, IDLE, INF = 0, 1, 2, 3
UNALIGNED = 4         # tensor 4 (1025 elements, group CLIPPED): param and grad 4 bytes into their storage
CLIP_HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
MAX_NORM = 1.0
CLIP_STEPS = 3


def clip_sizes():
    return [CLIP_SIZES[i % len(CLIP_SIZES)] for i in range(CLIP_TENSORS)]


def clip_groups():
    # 6 sizes x 4 groups: i // 6 walks the groups while i % 6 walks the sizes, so every group has every size
    return [(i // len(CLIP_SIZES)) % CLIP_GROUPS for i in range(CLIP_TENSORS)]


def clip_params(seed=17):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in clip_sizes()]


def clip_gradients(step, seed=23):
    """Step `step`'s gradients: group CLIPPED of norm about 14, UNCLIPPED of
    about 0.01, INF with one +inf element in its 4100-element tensor at step 0
    (and finite, large, afterwards)."""
    rng = np.random.default_rng(seed + 1000 * step)
    out = []
    for n, u in zip(clip_sizes(), clip_groups()):
        g = (rng.standard_normal(n) * (1e-4 if u == UNCLIPPED else 0.1)).astype(np.float32)
        if u == INF and n == 4100 and step == 0:
            g[4097] = np.inf
        out.append(g)
    return out


def clip_rows(device="cpu"):
    rows = torch.ones(CLIP_GROUPS, dtype=torch.int64)
    rows[IDLE] = 0
    return rows.to(device)


class RawAdam:
    """m, v, state and descriptors over plain tensors, for the raw calls."""

    def __init__(self, mb, params, groups, n_groups, device, unaligned=()):
        self.mb, self.device, self.G = mb, device, n_groups
        self.groups = list(groups)

        def place(a, off):
            base = torch.zeros(a.size + 4, dtype=torch.float32, device=device)
            view = base[off:off + a.size]
            view.copy_(torch.from_numpy(a))
            assert view.data_ptr() % 16 == 4 * off
            return view
        self.p = [place(a, 1 if i in unaligned else 0) for i, a in enumerate(params)]
        self.g = [place(np.zeros_like(a), 1 if i in unaligned else 0) for i, a in enumerate(params)]
        self.m = [place(np.zeros_like(a), 0) for a in params]
        self.v = [place(np.zeros_like(a), 0) for a in params]
        self.state = torch.tensor([[0, 0x3F800000, 0x3F800000]] * n_groups, dtype=torch.int32, device=device)
        self.grad_norm = torch.full((n_groups,), -1.0, dtype=torch.float32, device=device)
        self.desc = (mb._AdamTensor * len(params))()
        for i, d in enumerate(self.desc):
            d.param, d.grad, d.m, d.v = (x[i].data_ptr() for x in (self.p, self.g, self.m, self.v))
            d.n, d.group = params[i].size, self.groups[i]
        need = ctypes.c_uint64()
        mb._check(mb._lib.mbots_policy_adam_clip_workspace(self.desc, len(params), n_groups, ctypes.byref(need)))
        self.ws_bytes = need.value
        self.ws = torch.zeros((need.value + 7) // 8, dtype=torch.float64, device=device)

    def set_gradients(self, grads):
        for dst, g in zip(self.g, grads):
            dst.copy_(torch.from_numpy(g))

    def step_clip(self, rows, weight_decay, max_norm, **hyper):
        mb, h = self.mb, hyper
        mb._on_device(self.state.device, lambda d, st: mb._lib.mbots_policy_adam_clip(
            self.desc, len(self.p), mb._ptr(self.state), self.G, mb._ptr(rows), h["lr"], h["betas"][0], h["betas"][1],
            h["eps"], weight_decay, max_norm, mb._ptr(self.grad_norm), mb._ptr(self.ws), self.ws_bytes, d, st))

    def step_plain(self, rows, **hyper):
        mb, h = self.mb, hyper
        mb._on_device(self.state.device, lambda d, st: mb._lib.mbots_policy_adam(
            self.desc, len(self.p), mb._ptr(self.state), self.G, mb._ptr(rows), h["lr"], h["betas"][0], h["betas"][1],
            h["eps"], d, st))

    def snapshot(self):
        """(params, m, v, state, grad_norm) as CPU numpy copies."""
        cp = lambda xs: [x.cpu().numpy().copy() for x in xs]
        return cp(self.p), cp(self.m), cp(self.v), self.state.cpu().numpy().copy(), self.grad_norm.cpu().numpy().copy()


def run_clip(mb, device, weight_decay=0.01, max_norm=MAX_NORM, steps=CLIP_STEPS):
    """`steps` clipped steps on `device`; returns the snapshots after each."""
    opt = RawAdam(mb, clip_params(), clip_groups(), CLIP_GROUPS, device, unaligned=(UNALIGNED,))
    rows = clip_rows(device)
    trace = []
    for k in range(steps):
        opt.set_gradients(clip_gradients(k))
        opt.step_clip(rows, weight_decay, max_norm, **CLIP_HYPER)
        trace.append(opt.snapshot())
    return trace
