"""TEST INFRASTRUCTURE: torch autograd restatements of PolicyNet.evaluate
(DESIGN.md "Differentiable evaluate") -- in float64, the reference of the
gradient tests, and in float32, the yardstick their tolerance is a multiple of
-- over the nets of tests/policy_ref.py.  Not a product path."""
import numpy as np
import torch

import policy_ref as pr


def param_names(net):
    """Names of evaluate's parameters in its order: trunk, actor, critic; weight then bias."""
    names = []
    for grp, k in (("trunk", len(net["trunk"])), ("actor", 2), ("critic", 2)):
        for i in range(k):
            names += [f"{grp}{i}.w", f"{grp}{i}.b"]
    return names


def params_of(net):
    """The float32 numpy arrays behind param_names() (None for a missing bias)."""
    out = []
    for w, b, _ in net["trunk"]:
        out += [w, b]
    for grp in ("actor", "critic"):
        for w, b in net[grp]:
            out += [w, b]
    return out


def strip_biases(net, which):
    """`net` with the biases of the named layers (e.g. "trunk1", "actor1") removed."""
    net = dict(net)
    net["trunk"] = [(w, None if f"trunk{i}" in which else b, c) for i, (w, b, c) in enumerate(net["trunk"])]
    for grp in ("actor", "critic"):
        net[grp] = [(w, None if f"{grp}{i}" in which else b) for i, (w, b) in enumerate(net[grp])]
    return net


def policy_net(net, device="cpu", requires_grad=True):
    """(madrona_bots.PolicyNet, its parameter tensors in param_names() order)."""
    import madrona_bots as mb

    def t(a):
        return None if a is None else torch.from_numpy(a.copy()).to(device).requires_grad_(requires_grad)
    ps = [t(a) for a in params_of(net)]
    T = len(net["trunk"])
    trunk = [(ps[2 * i], ps[2 * i + 1], net["trunk"][i][2]) for i in range(T)]
    heads = [[(ps[2 * (T + 2 * h + i)], ps[2 * (T + 2 * h + i) + 1], 0) for i in range(2)] for h in range(2)]
    mem = None
    if net["memory"] is not None:
        mem = tuple(t(a) for a in net["memory"]) + (0,)
    return mb.PolicyNet(trunk, heads[0], heads[1], mem, net["memory_in"]), ps


def evaluate_torch(net, x, action, dtype, g=None):
    """(logp, value, entropy, grads) by torch autograd in `dtype`, all as
    float64 numpy; grads (g = (g_logp, g_value, g_entropy), any None) are those
    of sum(g_logp logp + g_value value + g_entropy entropy) in param_names()
    order, None without g or for a missing bias."""
    F = torch.nn.functional
    ps = [None if a is None else torch.from_numpy(a).to(dtype).requires_grad_(True) for a in params_of(net)]
    T = len(net["trunk"])
    h = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    for i in range(T):
        h = pr.act_torch(net["trunk"][i][2], F.linear(h, ps[2 * i], ps[2 * i + 1]))

    def head(o):
        return F.linear(F.relu(F.linear(h, ps[o], ps[o + 1])), ps[o + 2], ps[o + 3])
    z, value = head(2 * T), head(2 * T + 4)[:, 0]
    lsm = torch.log_softmax(z, dim=1)
    logp = lsm.gather(1, torch.from_numpy(np.asarray(action, np.int64)).reshape(-1, 1))[:, 0]
    entropy = -(lsm.exp() * lsm).sum(dim=1)
    grads = None
    if g is not None:
        loss = sum((torch.from_numpy(np.asarray(gi)).to(dtype) * o).sum()
                   for gi, o in zip(g, (logp, value, entropy)) if gi is not None)
        live = [p for p in ps if p is not None]
        if len(x) == 0 or not torch.is_tensor(loss):
            got = [torch.zeros_like(p) for p in live]
        else:
            got = torch.autograd.grad(loss, live, allow_unused=True)
            got = [torch.zeros_like(p) if q is None else q for p, q in zip(live, got)]
        it = iter(got)
        grads = [None if p is None else next(it).double().numpy() for p in ps]
    d = lambda v: v.detach().double().numpy()
    return d(logp), d(value), d(entropy), grads


def random_rows(rng, n, memory_in):
    """Observation-like rows (bytes, positions, a subnormal health column), hidden floats, actions."""
    obs = np.abs(rng.normal(0.0, 30.0, (n, 69))).astype(np.float32)
    obs[:, 32] = (rng.integers(0, 100, n).astype(np.int32)).view(np.float32)
    hidden = rng.uniform(-1.0, 1.0, (n, 16)).astype(np.float32) if memory_in else None
    action = rng.integers(0, 6, n).astype(np.int32)
    return obs, hidden, action


def away_from_kinks(net, x, margin=1e-4):
    """Rows none of whose ReLU / LeakyReLU inputs (float64) lies within
    `margin` of 0.  The derivative jumps there, so a row whose f32 input falls
    on the other side than its float64 one changes a gradient by a whole row's
    share: neither torch's f32 nor the library's is wrong, and float64 is no
    reference for such a row."""
    h = x.astype(np.float64)
    ok = np.ones(len(x), bool)
    for w, b, c in net["trunk"]:
        pre = h @ w.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64))
        if c in (1, 2):
            ok &= np.abs(pre).min(axis=1) >= margin
        h = pr.act64(c, pre)
    for grp in ("actor", "critic"):
        w, b = net[grp][0]
        pre = h @ w.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64))
        ok &= np.abs(pre).min(axis=1) >= margin
    return ok


def net_input(obs, hidden):
    return obs if hidden is None else np.concatenate([obs, hidden], axis=1)
