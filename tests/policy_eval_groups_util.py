"""TEST INFRASTRUCTURE shared by the grouped-evaluate tests (DESIGN.md "Grouped
evaluate"): the one fixture -- three groups of mixed nets over segments of every
length at which the kernels take another path --, the per-net evaluate() loop
over .tolist() slices that is the reference, and the runners.  Not a product
path."""
import functools

import numpy as np
import torch

import policy_ref as pr
import policy_grad_ref as gr
from test_policy_grad_cpu import dyadic

# group: (H, trunk activation codes, memory_in, memory head)
ARCH = [(16, [3], False, False),            # Tanh
        (128, [4, 4, 4], True, True),       # ELU, memory_in; its memory head is ignored
        (64, [2, 2], False, False)]         # LeakyReLU; species 4 has no net
ABSENT = (2, 3)
# rows of every (group, species): {0, 1, 63, 64, 65, 16385}; 16385 = 64 * 256 + 1
# wraps an accumulator and continues its chain, on the H = 16 net
LENGTHS = [[16385, 0, 65, 1], [64, 63, 1, 65], [65, 64, 63, 64]]
# the order in which the segments lie in the table (not the index order), after
# a one-row gap; GAP_AFTER rows follow the last
ORDER = [(1, 3), (2, 0), (0, 2), (2, 3), (1, 0), (0, 0), (0, 1), (2, 2), (1, 1), (0, 3), (1, 2), (2, 1)]
GAP_BEFORE, GAP_AFTER = 1, 7


def segments_of(lengths=LENGTHS, order=ORDER):
    """(int32 [G, 4, 2], n)."""
    seg = np.zeros((len(lengths), 4, 2), np.int32)
    at = GAP_BEFORE
    for g, s in order:
        seg[g, s] = (at, at + lengths[g][s])
        at += lengths[g][s]
    return seg, at + GAP_AFTER


@functools.lru_cache(maxsize=None)
def fixture():
    """nets[g][s] (make_net dicts, None where absent), segments, n, obs, hidden,
    action, g (three dyadic [n] arrays): numpy, built once and never changed."""
    rng = np.random.default_rng(20260)
    seg, n = segments_of()
    obs, hidden, action = gr.random_rows(rng, n, True)
    probe = gr.net_input(obs[:256], hidden[:256])
    nets = []
    for g, (H, codes, mi, mh) in enumerate(ARCH):
        x = probe if mi else np.ascontiguousarray(probe[:, :69])
        nets.append([None if (g, s) == ABSENT else
                     pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, mi, mh, pr.in_scale(x)), x)
                     for s in range(4)])
    scale = -int(np.ceil(np.log2(n)))
    grads = [dyadic(rng, n, scale) for _ in range(3)]
    return nets, seg, n, obs, hidden, action, grads


def policy_nets(nets, device="cpu"):
    """(PolicyNet or None per [g][s], the parameter tensors per [g][s])."""
    made = [[(None, None) if d is None else gr.policy_net(d, device) for d in four] for four in nets]
    return [[p for p, _ in four] for four in made], [[ps for _, ps in four] for four in made]


def to(device, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]


def grads_of(params):
    return [[None if ps is None else [None if q is None else (torch.zeros_like(q) if q.grad is None else q.grad)
                                      for q in ps] for ps in four] for four in params]


def run_loop(nets, seg, obs, hidden, action, g, device="cpu"):
    """The reference: one PolicyNet.evaluate per (group, species) over the
    .tolist() slices, every loss term's backward.  (logp, value, entropy [n]
    with +0 outside the evaluated rows, grads[g][s])."""
    pn, params = policy_nets(nets, device)
    obs, hidden, action, *g = to(device, obs, hidden, action, *g)
    out = [torch.zeros(obs.shape[0], device=device) for _ in range(3)]
    loss = []
    for four, sg in zip(pn, np.asarray(seg).tolist()):
        for net, (lo, hi) in zip(four, sg):
            if net is None:
                continue
            o = net.evaluate(obs[lo:hi], action[lo:hi], hidden[lo:hi] if net.memory_in else None)
            for dst, src in zip(out, o):
                dst[lo:hi] = src.detach()
            loss.append(sum((gi[lo:hi] * oi).sum() for gi, oi in zip(g, o)))
    sum(loss).backward()
    return out, grads_of(params)


def run_grouped(nets, seg, obs, hidden, action, g, device="cpu"):
    """The same through one evaluate_groups and one backward."""
    import madrona_bots as mb
    pn, params = policy_nets(nets, device)
    obs, hidden, action, seg, *g = to(device, obs, hidden, action, seg, *g)
    out = mb.evaluate_groups(pn, obs, action, seg, hidden)
    sum((gi * oi).sum() for gi, oi in zip(g, out)).backward()
    return [o.detach() for o in out], grads_of(params)


def assert_same(a, b, where):
    """Outputs and every gradient, with torch.equal."""
    (out_a, grads_a), (out_b, grads_b) = a, b
    for k, x, y in zip(("logp", "value", "entropy"), out_a, out_b):
        assert torch.equal(x.cpu(), y.cpu()), (where, k, int((x.cpu() != y.cpu()).sum()))
    for g, (fa, fb) in enumerate(zip(grads_a, grads_b)):
        for s, (pa, pb) in enumerate(zip(fa, fb)):
            assert (pa is None) == (pb is None), (where, g, s)
            for i, (x, y) in enumerate(zip(pa or [], pb or [])):
                assert (x is None) == (y is None), (where, g, s, i)
                if x is not None:
                    assert x.shape == y.shape and torch.equal(x.cpu(), y.cpu()), (where, g, s, i)


def outside_rows(seg, n, nets):
    """bool [n]: the rows in no segment, or in the segment of a pair without a net."""
    out = np.ones(n, bool)
    for g, four in enumerate(np.asarray(seg).tolist()):
        for s, (lo, hi) in enumerate(four):
            if nets[g][s] is not None:
                out[lo:hi] = False
    return out


def digest(result):
    """A hash of every bit of (outputs, grads)."""
    import hashlib
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
