"""TEST INFRASTRUCTURE: the gated memory head (DESIGN.md "Gated memory head")
restated for the tests -- evaluate_seq_torch of tests/policy_seq_ref.py with
h = (1 - z) h + z c and torch.sigmoid, in float64 (the reference) and float32
(the yardstick) --, gated nets over those of tests/policy_ref.py, and the cases
the CPU and GPU tests share.  Not a product path."""
import numpy as np
import torch

import policy_ref as pr
import policy_grad_ref as gr
import policy_seq_ref as sr
from policy_seq_ref import G, TILE, bits, same_bits, flat   # noqa: F401  (shared with the tests)


def add_gate(rng, net, bias=True, gain=1.0):
    """`net` (a make_net() dict with a memory head and memory_in) with a gate
    head Linear(H, 16): pre-activations of O(1), so z spreads over (0, 1)."""
    H = net["trunk"][0][0].shape[0]
    a = gain * np.sqrt(3.0 / H)
    net = dict(net)
    net["gate"] = (rng.uniform(-a, a, (16, H)).astype(np.float32),
                   rng.uniform(-0.3, 0.3, 16).astype(np.float32) if bias else None)
    return net


def const_gate(net, bias):
    """`net` with a gate of zero weights and the bias `bias`: z is sigmoid(bias) on every row."""
    H = net["trunk"][0][0].shape[0]
    net = dict(net)
    net["gate"] = (np.zeros((16, H), np.float32), np.full(16, bias, np.float32))
    return net


def param_names(net):
    """evaluate_sequences' parameters, then the gate head's."""
    return sr.param_names(net) + (["gate.w", "gate.b"] if net.get("gate") is not None else [])


def params_of(net):
    return sr.params_of(net) + (list(net["gate"]) if net.get("gate") is not None else [])


def policy_net(net, device="cpu", requires_grad=True):
    """(madrona_bots.PolicyNet, its parameter tensors in param_names() order)."""
    import madrona_bots as mb

    def t(a):
        return None if a is None else torch.from_numpy(a.copy()).to(device).requires_grad_(requires_grad)
    ps = [t(a) for a in params_of(net)]
    T = len(net["trunk"])
    trunk = [(ps[2 * i], ps[2 * i + 1], net["trunk"][i][2]) for i in range(T)]
    heads = [[(ps[2 * (T + 2 * h + i)], ps[2 * (T + 2 * h + i) + 1], 0) for i in range(2)] for h in range(2)]
    o = 2 * (T + 4)
    mem = (ps[o], ps[o + 1], 0)
    gate = (ps[o + 2], ps[o + 3], 0) if net.get("gate") is not None else None
    return mb.PolicyNet(trunk, heads[0], heads[1], mem, True, gate), ps


def evaluate_seq_torch(net, obs, action, length, hidden0, dtype, g=None):
    """sr.evaluate_seq_torch for a gated net: (logp, value, entropy [L, B],
    hidden [L, B, 16], grads in param_names() order), all float64 numpy."""
    F = torch.nn.functional
    ps = [None if a is None else torch.from_numpy(a).to(dtype).requires_grad_(True) for a in params_of(net)]
    T = len(net["trunk"])
    o = 2 * (T + 4)
    L, B = obs.shape[:2]
    h = torch.from_numpy(np.ascontiguousarray(hidden0)).to(dtype)
    n = torch.from_numpy(np.asarray(length, np.int64))
    outs = [[], [], [], []]
    for k in range(L):
        t = torch.cat([torch.from_numpy(np.ascontiguousarray(obs[k])).to(dtype), h], dim=1)
        for i in range(T):
            t = pr.act_torch(net["trunk"][i][2], F.linear(t, ps[2 * i], ps[2 * i + 1]))

        def head(q):
            return F.linear(F.relu(F.linear(t, ps[q], ps[q + 1])), ps[q + 2], ps[q + 3])
        z, value = head(2 * T), head(2 * T + 4)[:, 0]
        lsm = torch.log_softmax(z, dim=1)
        logp = lsm.gather(1, torch.from_numpy(np.asarray(action[k], np.int64)).clamp(0, 5).reshape(-1, 1))[:, 0]
        entropy = -(lsm.exp() * lsm).sum(dim=1)
        m = k < n
        zero = torch.zeros((), dtype=dtype)
        for dst, v in zip(outs, (logp, value, entropy)):
            dst.append(torch.where(m, v, zero))
        outs[3].append(torch.where(m[:, None], h, zero).detach())
        c = torch.tanh(F.linear(t, ps[o], ps[o + 1]))
        zg = torch.sigmoid(F.linear(t, ps[o + 2], ps[o + 3]))
        h = (1 - zg) * h + zg * c
    stack = lambda v, tail: torch.stack(v) if L else torch.zeros((0, B) + tail, dtype=dtype)
    logp, value, entropy, hidden = stack(outs[0], ()), stack(outs[1], ()), stack(outs[2], ()), stack(outs[3], (16,))
    grads = None
    if g is not None:
        loss = sum((torch.from_numpy(np.asarray(gi)).to(dtype) * q).sum()
                   for gi, q in zip(g, (logp, value, entropy)) if gi is not None)
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


def next_h(net, x, dtype):
    """h_{k+1} of the rows x = obs | h_k [n, 85] by torch in `dtype`, as float64 numpy."""
    F = torch.nn.functional
    c = lambda a: None if a is None else torch.from_numpy(a).to(dtype)
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    t = xt
    for w, b, code in net["trunk"]:
        t = pr.act_torch(code, F.linear(t, c(w), c(b)))
    m = torch.tanh(F.linear(t, c(net["memory"][0]), c(net["memory"][1])))
    z = torch.sigmoid(F.linear(t, c(net["gate"][0]), c(net["gate"][1])))
    return ((1 - z) * xt[:, 69:85] + z * m).double().numpy()


def chain_away_from_kinks(net, obs, hidden0):
    """sr.chain_away_from_kinks along the gated chain."""
    ok = np.ones(obs.shape[1], bool)
    h = hidden0.astype(np.float64)
    for k in range(obs.shape[0]):
        x = np.concatenate([obs[k].astype(np.float64), h], axis=1)
        ok &= gr.away_from_kinks(net, x)
        h = next_h(net, x, torch.float64)
    return ok


# ---- the cases ----
# (H, trunk codes, layers without a bias, L, B, length pattern, which of g_logp / g_value / g_entropy)
CASES = [
    (16, [3], (), 1, 1, "full", "lve"),
    (16, [1, 2], (), 2, 63, "ragged", "lve"),
    (48, [4, 5, 3], (), 5, 64, "full", "lve"),
    (128, [0, 3, 1, 5], (), 5, 65, "ragged", "lve"),
    (128, [0, 3, 1], (), 2, 3 * TILE + 9, "tileshort", "lve"),
    (16, [2], (), 2, TILE * G + 1, "wrapzero", "lve"),
    (16, [3, 1], (), 2, TILE * G + 1, "tilezero", "lve"),
    (48, [3, 1], ("gate", "memory"), 5, 65, "ragged", "lve"),      # the gate's bias absent
]


def case_id(c):
    return f"H{c[0]}-d{len(c[1])}-L{c[3]}-B{c[4]}-{c[5]}" + ("-nobias" if c[2] else "")


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
    cat = lambda i, ax: np.ascontiguousarray(np.concatenate([q[i] for q in got], axis=ax))
    return cat(0, 1)[:, :B].copy(), cat(1, 0)[:B].copy(), cat(2, 1)[:, :B].copy()


_built = {}


def build(case, seed=0):
    """The case's gated net, batch and upstream gradients; built once and
    shared -- nobody writes into it."""
    key = (CASES.index(case), seed)
    if key in _built:
        return _built[key]
    H, codes, nobias, L, B, pattern, which = case
    rng = np.random.default_rng(9100 + key[0] + 100 * seed)
    probe = gr.net_input(*gr.random_rows(rng, 256, True)[:2])
    net = pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, True, True, pr.in_scale(probe)), probe)
    net = add_gate(rng, sr.strip_biases(net, nobias), bias="gate" not in nobias)
    obs, hidden0, action = random_batch(rng, net, L, B)
    length = sr.lengths(rng, pattern, L, B)
    s = -int(np.ceil(np.log2(max(L * B, 1))))
    g = [sr.dyadic(rng, (L, B), s) if k in which else None for k in "lve"]
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


def value_equal(a, b):
    """Equal as values (a -0 against a +0 passes), and bit for bit where nonzero."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b)) and \
        bool(np.array_equal(bits(a)[np.asarray(a) != 0], bits(b)[np.asarray(a) != 0]))
