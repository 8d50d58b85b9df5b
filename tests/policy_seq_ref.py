"""TEST INFRASTRUCTURE: torch autograd restatements of
PolicyNet.evaluate_sequences (DESIGN.md "Backpropagation through HiddenState")
-- in float64, the reference of the gradient tests, and in float32, the
yardstick their tolerance is a multiple of -- over the nets of
tests/policy_ref.py, the chain's version of away_from_kinks, and the cases the
CPU and GPU tests share.  Not a product path."""
import numpy as np
import torch

import policy_ref as pr
import policy_grad_ref as gr

G = 256                      # kPolGradAcc
TILE = 64                    # kPolGradRows


def param_names(net):
    """evaluate's parameters, then the memory head's."""
    return gr.param_names(net) + ["memory.w", "memory.b"]


def params_of(net):
    return gr.params_of(net) + list(net["memory"])


def strip_biases(net, which):
    net = gr.strip_biases(net, which)
    if "memory" in which:
        net["memory"] = (net["memory"][0], None)
    return net


def policy_net(net, device="cpu"):
    """(madrona_bots.PolicyNet, its parameter tensors in param_names() order)."""
    p, ps = gr.policy_net(net, device)
    return p, ps + [p.memory[0], p.memory[1]]


def evaluate_seq_torch(net, obs, action, length, hidden0, dtype, g=None):
    """(logp, value, entropy [L, B], hidden [L, B, 16], grads) by torch autograd
    in `dtype` with a Python loop over the steps, all as float64 numpy; grads
    (g = (g_logp, g_value, g_entropy) [L, B], any None) in param_names() order."""
    F = torch.nn.functional
    ps = [None if a is None else torch.from_numpy(a).to(dtype).requires_grad_(True) for a in params_of(net)]
    T = len(net["trunk"])
    L, B = obs.shape[:2]
    h = torch.from_numpy(np.ascontiguousarray(hidden0)).to(dtype)
    n = torch.from_numpy(np.asarray(length, np.int64))
    outs = [[], [], [], []]
    for k in range(L):
        x = torch.cat([torch.from_numpy(np.ascontiguousarray(obs[k])).to(dtype), h], dim=1)
        t = x
        for i in range(T):
            t = pr.act_torch(net["trunk"][i][2], F.linear(t, ps[2 * i], ps[2 * i + 1]))

        def head(o):
            return F.linear(F.relu(F.linear(t, ps[o], ps[o + 1])), ps[o + 2], ps[o + 3])
        z, value = head(2 * T), head(2 * T + 4)[:, 0]
        lsm = torch.log_softmax(z, dim=1)
        logp = lsm.gather(1, torch.from_numpy(np.asarray(action[k], np.int64)).clamp(0, 5).reshape(-1, 1))[:, 0]
        entropy = -(lsm.exp() * lsm).sum(dim=1)
        m = k < n
        zero = torch.zeros((), dtype=dtype)
        for dst, v in zip(outs, (logp, value, entropy)):
            dst.append(torch.where(m, v, zero))
        outs[3].append(torch.where(m[:, None], h, zero).detach())
        h = torch.tanh(F.linear(t, ps[-2], ps[-1]))     # (an absent element's state is never read by a present one)
    stack = lambda v, tail: torch.stack(v) if L else torch.zeros((0, B) + tail, dtype=dtype)
    logp, value, entropy, hidden = stack(outs[0], ()), stack(outs[1], ()), stack(outs[2], ()), stack(outs[3], (16,))
    grads = None
    if g is not None:
        loss = sum((torch.from_numpy(np.asarray(gi)).to(dtype) * o).sum()
                   for gi, o in zip(g, (logp, value, entropy)) if gi is not None)
        live = [p for p in ps if p is not None]
        if L * B == 0 or not torch.is_tensor(loss) or not loss.requires_grad:
            got = [torch.zeros_like(p) for p in live]
        else:
            got = torch.autograd.grad(loss, live, allow_unused=True)
            got = [torch.zeros_like(p) if q is None else q for p, q in zip(live, got)]
        it = iter(got)
        grads = [None if p is None else next(it).double().numpy() for p in ps]
    d = lambda v: v.detach().double().numpy()
    return d(logp), d(value), d(entropy), d(hidden), grads


def step64(net, x):
    """(rows away from every ReLU / LeakyReLU kink, the memory head's output) of one step in float64."""
    ok = gr.away_from_kinks(net, x)
    h = x.astype(np.float64)
    for w, b, c in net["trunk"]:
        h = pr.act64(c, h @ w.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64)))
    w, b = net["memory"]
    return ok, np.tanh(h @ w.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64)))


def chain_away_from_kinks(net, obs, hidden0):
    """gr.away_from_kinks along the chain: the sequences whose every step (all
    L of them, so any length may be given to them afterwards) stays away from
    the kinks in the float64 chain."""
    ok = np.ones(obs.shape[1], bool)
    h = hidden0.astype(np.float64)
    for k in range(obs.shape[0]):
        o, h = step64(net, np.concatenate([obs[k].astype(np.float64), h], axis=1))
        ok &= o
    return ok


# ---- the cases ----
# (H, trunk codes, layers without a bias, L, B, length pattern, which of g_logp / g_value / g_entropy)
CASES = [
    (16, [3], (), 1, 1, "full", "lve"),
    (16, [1, 2], ("memory",), 2, 63, "ragged", "l"),
    (48, [4, 5, 3], (), 5, 64, "full", "v"),
    (128, [0, 3, 1, 5], (), 5, 65, "ragged", "e"),
    (128, [0, 3, 1], ("trunk1", "actor1"), 2, 3 * TILE + 9, "tileshort", "lve"),
    (128, [4, 2], (), 5, 3 * TILE + 9, "tilezero", "lve"),
    (48, [2, 4], ("trunk0",), 2, TILE * G + 1, "ragged", "lve"),
    (16, [5, 1, 4, 2], ("critic0",), 5, 3 * TILE + 9, "ragged", "lve"),
    (48, [3, 1], (), 1, 65, "full", "lve"),
    (16, [2], (), 1, 3 * TILE + 9, "full", "lve"),
    (48, [1, 4, 3], (), 1, TILE * G + 1, "full", "lve"),
    (16, [4], (), 1, 63, "full", "lve"),
    (48, [5, 2], (), 1, 64, "full", "lve"),
    # accumulator 0 holds tiles 0 and 256: one of them without a step, the other with
    (16, [3, 1], (), 2, TILE * G + 1, "tilezero", "lve"),
    (16, [2], (), 2, TILE * G + 1, "wrapzero", "lve"),
]


def case_id(c):
    return f"H{c[0]}-d{len(c[1])}-L{c[3]}-B{c[4]}-{c[5]}-{c[6]}"


def lengths(rng, pattern, L, B):
    if pattern == "full":
        return np.full(B, L, np.int32)
    n = rng.integers(0, L + 1, B).astype(np.int32)
    if pattern == "ragged":
        n[rng.permutation(B)[:3]] = [0, 1, L][:min(B, 3)]
    elif pattern == "tileshort":          # tile 1 never reaches L; the others do
        n[:] = L
        n[TILE:2 * TILE] = rng.integers(0, L, TILE)
    elif pattern == "tilezero":           # tile 0, the first of its accumulator, has no step at all
        n[:] = rng.integers(1, L + 1, B)
        n[:TILE] = 0
        n[-1] = L
    elif pattern == "wrapzero":           # the tiles past the first G, each the second of its accumulator, have none
        n[:] = rng.integers(1, L + 1, B)
        n[TILE * G:] = 0
    return n


def dyadic(rng, shape, scale_log2):
    """Multiples of 2^-8 in [-1, 1] times 2^scale_log2 (tests/test_policy_grad_cpu.py's dyadic())."""
    return (rng.integers(-256, 257, shape).astype(np.float32) / np.float32(256.0)) * np.float32(2.0 ** scale_log2)


def random_batch(rng, net, L, B):
    """B kink-free sequences of L steps: (obs [L, B, 69], hidden0 [B, 16], action [L, B])."""
    got, have = [], 0
    for _ in range(64):
        n = B + B // 2 + 64
        obs, _, action = gr.random_rows(rng, L * n, False)
        obs, action = obs.reshape(L, n, 69), action.reshape(L, n)
        hidden0 = rng.uniform(-1.0, 1.0, (n, 16)).astype(np.float32)
        ok = np.nonzero(chain_away_from_kinks(net, obs, hidden0))[0]
        got.append((obs[:, ok], hidden0[ok], action[:, ok]))
        have += len(ok)
        if have >= B:
            break
    assert have >= B
    obs = np.concatenate([q[0] for q in got], axis=1)[:, :B]
    hidden0 = np.concatenate([q[1] for q in got], axis=0)[:B]
    action = np.concatenate([q[2] for q in got], axis=1)[:, :B]
    return np.ascontiguousarray(obs), np.ascontiguousarray(hidden0), np.ascontiguousarray(action)


_built = {}


def build(case, seed=0):
    """The case's net, batch and upstream gradients (None where the case leaves
    one out); built once and shared -- nobody writes into it."""
    key = (CASES.index(case), seed)
    if key in _built:
        return _built[key]
    H, codes, nobias, L, B, pattern, which = case
    rng = np.random.default_rng(7000 + key[0] + 100 * seed)
    probe = gr.net_input(*gr.random_rows(rng, 256, True)[:2])
    net = pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, True, True, pr.in_scale(probe)), probe)
    net = strip_biases(net, nobias)
    obs, hidden0, action = random_batch(rng, net, L, B)
    length = lengths(rng, pattern, L, B)
    s = -int(np.ceil(np.log2(max(L * B, 1))))
    g = [dyadic(rng, (L, B), s) if k in which else None for k in "lve"]
    _built[key] = (net, obs, action, length, hidden0, g)
    return _built[key]


def run_sequences(net, obs, action, length, hidden0, g, device="cpu"):
    """(logp, value, entropy, hidden, grads in param_names() order) of the library, as numpy."""
    p, ps = policy_net(net, device)
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)
    out = p.evaluate_sequences(t(obs), t(action), t(length), t(hidden0), return_hidden=True)
    terms = [(t(gi) * o).sum() for gi, o in zip(g, out[:3]) if gi is not None]
    sum(terms).backward()
    grads = [None if q is None else (torch.zeros_like(q) if q.grad is None else q.grad).cpu().numpy() for q in ps]
    return tuple(o.detach().cpu().numpy() for o in out) + (grads,)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def flat(o):
    return list(o[:4]) + o[4]
