"""TEST INFRASTRUCTURE shared by the grouped evaluate_sequences tests (DESIGN.md
"Grouped evaluate_sequences"): the one fixture -- three groups of mixed
recurrent nets whose columns are interleaved through one padded batch, with
segments of every size at which the kernels take another path --, the per-net
evaluate_sequences loop over index_select slices that is the reference, and
the runners.  Not a product path."""
import functools
import hashlib

import numpy as np
import torch

import policy_ref as pr
import policy_grad_ref as gr
import policy_seq_ref as sr

L = 5
# group: (H, trunk activation codes); every net has a memory head and memory_in
ARCH = [(16, [3]),                # Tanh
        (128, [4, 4, 4]),         # ELU
        (64, [2, 2])]             # LeakyReLU; species 4 has no net
ABSENT = (2, 3)
G = len(ARCH)
TILE = 64
# columns of every (group, species): {0, 1, 63, 64, 65, 16385}; 16385 = 64 * 256
# + 1 is 257 tiles, so accumulator 0 wraps and continues its chain (on the H =
# 16 net, its lengths at most 2)
SIZES = [[16385, 0, 65, 1], [64, 63, 1, 65], [65, 64, 63, 64]]
BIG = (0, 0)
SHORT_TILE = (1, 3)     # its first tile's largest length is L - 1
EMPTY_TILE = (2, 0)     # every column of its first tile has length 0
N_NONE = 9              # columns with net_id -1 or >= 4 G


class _Lcg:
    """A 32-bit linear congruential generator: every fill is a pure function of its seed."""

    def __init__(self, seed):
        self.s = np.uint64(seed)

    def u32(self, n):
        out = np.empty(n, np.uint32)
        s = int(self.s)
        for i in range(n):
            s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = s
        self.s = np.uint64(s)
        return out


def net_ids():
    """int32 [B]: the columns' net ids, interleaved so that `order` is far from
    the identity: the big segment's columns alternate with everybody else's."""
    small = []
    for g in range(G):
        for s in range(4):
            if (g, s) != BIG:
                small += [4 * g + s] * SIZES[g][s]
    none = [-1, 4 * G, -7, 4 * G + 3, 1 << 20, -1, 255, 4 * G, -2][:N_NONE]
    perm = _Lcg(99).u32(len(small)).argsort(kind="stable")
    small = [small[i] for i in perm]
    rest = small + none
    # one of the rest after every 23 of the big segment's, the remainder at the front
    big = SIZES[BIG[0]][BIG[1]]
    out, k = [], 0
    lead = len(rest) - big // 23
    out += rest[:max(lead, 0)]
    k = max(lead, 0)
    for i in range(big):
        out.append(4 * BIG[0] + BIG[1])
        if i % 23 == 22 and k < len(rest):
            out.append(rest[k])
            k += 1
    out += rest[k:]
    return np.asarray(out, np.int32)


def segments_ref(net_id, groups):
    """The nonzero construction: (order int32 [B] with the tail -1, segments int32 [groups, 4, 2])."""
    t = torch.from_numpy(np.asarray(net_id))
    order = torch.full((t.shape[0],), -1, dtype=torch.int32)
    seg = torch.zeros(groups, 4, 2, dtype=torch.int32)
    at = 0
    for e in range(4 * groups):
        cols = torch.nonzero(t == e)[:, 0].to(torch.int32)
        order[at:at + len(cols)] = cols
        seg[e // 4, e % 4, 0], seg[e // 4, e % 4, 1] = at, at + len(cols)
        at += len(cols)
    return order, seg


@functools.lru_cache(maxsize=None)
def fixture():
    """nets[g][s] (make_net dicts, None where absent), net_id [B], obs [L, B,
    69], action [L, B], length [B], hidden0 [B, 16], g (three dyadic [L, B]
    arrays): numpy, built once and never changed."""
    rng = np.random.default_rng(20261)
    net_id = net_ids()
    B = len(net_id)
    obs, _, action = gr.random_rows(rng, L * B, False)
    obs, action = np.ascontiguousarray(obs.reshape(L, B, 69)), np.ascontiguousarray(action.reshape(L, B))
    hidden0 = rng.uniform(-1.0, 1.0, (B, 16)).astype(np.float32)
    probe = gr.net_input(*gr.random_rows(rng, 256, True)[:2])
    nets = [[None if (g, s) == ABSENT else
             pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, True, True, pr.in_scale(probe)), probe)
             for s in range(4)] for g, (H, codes) in enumerate(ARCH)]
    length = rng.integers(0, L + 1, B).astype(np.int32)
    order, seg = segments_ref(net_id, G)
    order, seg = order.numpy(), seg.numpy()

    def cols(pair):
        lo, hi = seg[pair[0], pair[1]]
        return order[lo:hi]
    big = cols(BIG)
    length[big] = rng.integers(0, 3, len(big))          # at most 2: the 257 tiles stay cheap
    length[big[:TILE]] = rng.integers(1, 3, TILE)       # tile 0 and tile 256 share accumulator 0: both with steps
    length[big[-1]] = 2
    length[cols(SHORT_TILE)[:TILE]] = rng.integers(0, L, TILE)
    length[cols(SHORT_TILE)[0]] = L - 1
    length[cols(EMPTY_TILE)[:TILE]] = 0
    length[cols(EMPTY_TILE)[TILE]] = L
    length[cols((1, 0))[:3]] = [0, L, 1]
    scale = -int(np.ceil(np.log2(L * B)))
    grads = [sr.dyadic(rng, (L, B), scale) for _ in range(3)]
    return nets, net_id, obs, action, length, hidden0, grads


def policy_nets(nets, device="cpu"):
    """(PolicyNet or None per [g][s], the parameter tensors per [g][s], memory head last)."""
    made = [[(None, None) if d is None else sr.policy_net(d, device) for d in four] for four in nets]
    return [[p for p, _ in four] for four in made], [[ps for _, ps in four] for four in made]


def to(device, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def grads_of(params):
    return [[None if ps is None else [None if q is None else (torch.zeros_like(q) if q.grad is None else q.grad)
                                      for q in ps] for ps in four] for four in params]


def run_loop(nets, net_id, obs, action, length, hidden0, g, device="cpu", pn_params=None):
    """The reference: per (group, species) the nonzero / index_select slices
    through PolicyNet.evaluate_sequences, every loss term's backward.  (logp,
    value, entropy [L, B], hidden [L, B, 16] with +0 outside the evaluated
    columns, grads[g][s])."""
    pn, params = pn_params or policy_nets(nets, device)
    net_id, obs, action, length, hidden0, *g = to(device, net_id, obs, action, length, hidden0, *g)
    Ln, B = obs.shape[:2]
    out = [torch.zeros(Ln, B, device=device) for _ in range(3)] + [torch.zeros(Ln, B, 16, device=device)]
    loss = []
    for gi, four in enumerate(pn):
        for s, net in enumerate(four):
            if net is None:
                continue
            cols = torch.nonzero(net_id == 4 * gi + s)[:, 0]
            o = net.evaluate_sequences(obs.index_select(1, cols), action.index_select(1, cols), length[cols],
                                       hidden0[cols], return_hidden=True)
            for dst, src in zip(out, o):
                dst[:, cols] = src.detach()
            loss.append(sum((t.index_select(1, cols) * oi).sum() for t, oi in zip(g, o) if t is not None))
    sum(loss).backward()
    return out, grads_of(params)


def run_grouped(nets, net_id, obs, action, length, hidden0, g, device="cpu", pn_params=None, order_seg=None):
    """The same through sequence_segments, one evaluate_sequences_groups and one backward."""
    import madrona_bots as mb
    pn, params = pn_params or policy_nets(nets, device)
    net_id, obs, action, length, hidden0, *g = to(device, net_id, obs, action, length, hidden0, *g)
    order, seg = order_seg or mb.sequence_segments(net_id, len(pn))
    out = mb.evaluate_sequences_groups(pn, obs, action, length, hidden0, order, seg, return_hidden=True)
    sum((t * oi).sum() for t, oi in zip(g, out) if t is not None).backward()
    return [o.detach() for o in out], grads_of(params)


def assert_same(a, b, where):
    """Outputs, hidden and every gradient, with torch.equal."""
    (out_a, grads_a), (out_b, grads_b) = a, b
    for k, x, y in zip(("logp", "value", "entropy", "hidden"), out_a, out_b):
        assert x.shape == y.shape and torch.equal(x.cpu(), y.cpu()), (where, k, int((x.cpu() != y.cpu()).sum()))
    for g, (fa, fb) in enumerate(zip(grads_a, grads_b)):
        for s, (pa, pb) in enumerate(zip(fa, fb)):
            assert (pa is None) == (pb is None), (where, g, s)
            for i, (x, y) in enumerate(zip(pa or [], pb or [])):
                assert (x is None) == (y is None), (where, g, s, i)
                if x is not None:
                    assert x.shape == y.shape and torch.equal(x.cpu(), y.cpu()), (where, g, s, i)


def outside_columns(net_id, nets):
    """bool [B]: the columns no evaluated segment names."""
    out = np.ones(len(net_id), bool)
    for g, four in enumerate(nets):
        for s, d in enumerate(four):
            if d is not None:
                out[np.asarray(net_id) == 4 * g + s] = False
    return out


def digest(result):
    """A hash of every bit of (outputs, grads)."""
    h = hashlib.sha256()
    out, grads = result
    for t in out:
        h.update(t.cpu().numpy().tobytes())
    for four in grads:
        for ps in four:
            for q in ps or []:
                if q is not None:
                    h.update(q.cpu().numpy().tobytes())
    return h.hexdigest()


def check_window_bits_groups(exec_mode):
    """tests/test_policy_seq_cpu.py's check_window_bits on a manager with two
    policy groups of different recurrent nets: through a window in which agents
    are born, die and are reset, one evaluate_sequences_groups reproduces
    act()'s logp, value and HiddenState bits for every group."""
    import madrona_bots as mb
    sim = mb.SimManager(0, 16, 77, 32, exec_mode=exec_mode, episode_length=7)
    for t in range(4):
        sim.write_synthetic_actions(4321, t, True)
        sim.step()
    starts = [0, 7]
    sim.set_policy_groups(starts)
    x = pr.inputs(sim, True)
    rng = np.random.default_rng(31)
    nets = [[pr.policy_net(pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, True, True, pr.in_scale(x)), x),
                           sim.device) for _ in range(4)] for H, codes in ((48, [3, 1]), (16, [4]))]
    for u in range(2):
        sim.set_policy(nets[u], group=u)
    T = 6
    win = sim.trajectory_window(T, max_rows=sim.num_worlds * sim.agent_capacity, record_obs=True, record_state=True)
    keep = {"action": [], "logp": [], "value": [], "hidden": [], "species": []}
    for t in range(T):
        win.push()
        keep["hidden"].append(sim.hidden_state_tensor().to_torch().clone())
        o = sim.act()
        for k in ("action", "logp", "value"):
            keep[k].append(o[k])
        count = sim.species_count_tensor().to_torch().sum(dim=0).to(torch.int64)
        keep["species"].append(torch.repeat_interleave(torch.arange(4, device=count.device), count)
                               .to(torch.int32).reshape(-1, 1))
        if t + 1 < T:
            sim.step()
    out = win.compute(gamma=0.99)
    win.sequences()
    b = {k: v.clone() for k, v in win.batch().items()}
    got = {k: win.gather(v) for k, v in keep.items()}
    world = win.gather([w.to(torch.int32) for w in out["world"]])[0, :, 0].to(torch.int64)
    win.close()
    Ln, B = b["rows"].shape
    length, end, t0 = b["len"].cpu().numpy(), b["end"].cpu().numpy(), b["t0"].cpu().numpy()
    assert ((end == 1) & (t0 + length < Ln)).any(), "no sequence ends by death before the last table"
    assert (t0 > 0).any(), "no sequence starts after table 0"
    assert (end == 2).any(), "no sequence ends by reset"
    group = torch.bucketize(world, torch.tensor(starts, device=world.device), right=True) - 1
    net_id = (group * 4 + got["species"][0, :, 0].to(torch.int64)).to(torch.int32)
    assert len(set(net_id.cpu().tolist())) == 8, "a (group, species) pair without a sequence"
    order, seg = mb.sequence_segments(net_id, 2)
    logp, value, _, hidden = mb.evaluate_sequences_groups(nets, b["obs"], got["action"][:, :, 0].contiguous(), b["len"],
                                                          b["hidden0"], order, seg, return_hidden=True)
    m = torch.arange(Ln, device=b["len"].device)[:, None] < b["len"][None, :]
    assert int(m.sum()) > 64
    for name, a, w in (("logp", logp, got["logp"][:, :, 0]), ("value", value, got["value"][:, :, 0]),
                       ("hidden", hidden, got["hidden"])):
        assert torch.equal(a[m].view(torch.int32), w[m].view(torch.int32)), name
        assert not a[~m].view(torch.int32).any(), name


@functools.lru_cache(maxsize=None)
def cpu_grouped():
    """The fixture through the CPU path, computed once and shared."""
    return run_grouped(*fixture())
