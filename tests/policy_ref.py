"""TEST INFRASTRUCTURE: a numpy float64 restatement of the device actor
(DESIGN.md "Device actor") -- layers as float64 matmuls, numpy's own
activations, the counter RNG through the oracle's exact threefry -- plus the
random nets, the torch f32 yardstick and the helpers the policy tests share.
Not a product path."""
import numpy as np
import torch

import pyoracle

CODES = {0: "Identity", 1: "ReLU", 2: "LeakyReLU", 3: "Tanh", 4: "ELU", 5: "LogSigmoid"}


def act64(code, x):
    if code == 0:
        return x
    if code == 1:
        return np.maximum(x, 0.0)
    if code == 2:
        return np.where(x >= 0, x, 0.01 * x)
    if code == 3:
        return np.tanh(x)
    if code == 4:
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    if code == 5:
        return -np.logaddexp(0.0, -x)
    raise ValueError(code)


def act_torch(code, x):
    F = torch.nn.functional
    return [lambda v: v, F.relu, F.leaky_relu, torch.tanh, F.elu, F.logsigmoid][code](x)


def make_net(rng, H, depth, codes, memory_in, memory_head, in_scale):
    """One species' random net as float32 numpy arrays.  The first layer is
    scaled by 1 / in_scale (the inputs are unnormalised: bytes up to 255,
    positions up to 128), the others keep activations O(1), so the logits are
    O(1) and no action's probability vanishes."""
    def lin(n_in, n_out, gain):
        a = gain * np.sqrt(3.0 / n_in)
        return (rng.uniform(-a, a, (n_out, n_in)).astype(np.float32),
                rng.uniform(-0.3, 0.3, n_out).astype(np.float32))
    n_in = 85 if memory_in else 69
    trunk = []
    for l in range(depth):
        w, b = lin(n_in if l == 0 else H, H, 1.6)
        if l == 0:
            w = (w / np.float32(in_scale)).astype(np.float32)
        trunk.append((w, b, int(codes[l])))
    return {"trunk": trunk, "actor": [lin(H, H, 1.6), lin(H, 6, 1.6)], "critic": [lin(H, H, 1.6), lin(H, 1, 1.0)],
            "memory": lin(H, 16, 1.0) if memory_head else None, "memory_in": bool(memory_in)}


def calibrate_actor(net, x):
    """Rescale the actor's last layer so that, over the rows x, every logit
    has mean 0 and the logits' spread is 1: no action's share vanishes."""
    z, _, _ = forward64(net, x)
    mean, std = z.mean(axis=0), max(float((z - z.mean(axis=0)).std()), 1e-6)
    w, b = net["actor"][1]
    net["actor"][1] = ((w / np.float32(std)).astype(np.float32), ((b - mean) / std).astype(np.float32))
    return net


def policy_net(net, device="cpu"):
    """The madrona_bots.PolicyNet of a make_net() dict."""
    import madrona_bots as mb
    t = lambda a: torch.from_numpy(a).to(device)
    trunk = [(t(w), t(b), c) for w, b, c in net["trunk"]]
    heads = [[(t(w), t(b), 0) for w, b in net[k]] for k in ("actor", "critic")]
    mem = None if net["memory"] is None else (t(net["memory"][0]), t(net["memory"][1]), 0)
    return mb.PolicyNet(trunk, heads[0], heads[1], mem, net["memory_in"])


def forward64(net, x):
    """(logits [n, 6], value [n], memory [n, 16] or None) in float64."""
    h = x.astype(np.float64)
    for w, b, c in net["trunk"]:
        h = act64(c, h @ w.astype(np.float64).T + b.astype(np.float64))

    def head(layers):
        (w0, b0), (w1, b1) = layers
        a = np.maximum(h @ w0.astype(np.float64).T + b0.astype(np.float64), 0.0)
        return a @ w1.astype(np.float64).T + b1.astype(np.float64)
    mem = None
    if net["memory"] is not None:
        w, b = net["memory"]
        mem = np.tanh(h @ w.astype(np.float64).T + b.astype(np.float64))
    return head(net["actor"]), head(net["critic"])[:, 0], mem


def forward_torch32(net, x):
    """The same nets in torch's own f32 arithmetic: the yardstick of the
    tolerance.  Returns float64 copies of (logits, value, memory)."""
    F = torch.nn.functional
    t = torch.from_numpy
    h = t(np.ascontiguousarray(x, dtype=np.float32))
    for w, b, c in net["trunk"]:
        h = act_torch(c, F.linear(h, t(w), t(b)))

    def head(layers):
        (w0, b0), (w1, b1) = layers
        return F.linear(F.relu(F.linear(h, t(w0), t(b0))), t(w1), t(b1))
    mem = None
    if net["memory"] is not None:
        mem = torch.tanh(F.linear(h, t(net["memory"][0]), t(net["memory"][1]))).double().numpy()
    return head(net["actor"]).double().numpy(), head(net["critic"]).double().numpy()[:, 0], mem


def logp64(z):
    """log-softmax of float64 logits."""
    m = z.max(axis=1, keepdims=True)
    return (z - m) - np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def row_keys(species_count, world_offset=0):
    """(global world, species 1..4, k) of every exported row, in table order
    (species-major, world-major inside a species, then slot order)."""
    sc = np.asarray(species_count)
    gw, sp, k = [], [], []
    for s in range(4):
        for w in range(sc.shape[0]):
            n = int(sc[w, s])
            gw += [world_offset + w] * n
            sp += [s + 1] * n
            k += list(range(n))
    return np.array(gw, np.int64), np.array(sp, np.int64), np.array(k, np.int64)


def uniforms(seed, draw, gw, sp, k):
    """u01(threefry2x32(seed, draw, gw, (species - 1) << 16 | k).x), exact."""
    u = np.empty(len(gw), np.float64)
    for i in range(len(gw)):
        x, _ = pyoracle.threefry2x32((seed & 0xFFFFFFFF, draw & 0xFFFFFFFF),
                                     (int(gw[i]), ((int(sp[i]) - 1) << 16) | int(k[i])))
        u[i] = (x >> 8) / 16777216.0
    return u


def sample64(z, u):
    """(action, distance of u to the nearest CDF edge) from float64 logits:
    the first i with u < CDF_i, else 5."""
    m = z.max(axis=1, keepdims=True)
    c = np.cumsum(np.exp(z - m), axis=1)
    cdf = c / c[:, -1:]
    a = np.where((u[:, None] < cdf).any(axis=1), (u[:, None] < cdf).argmax(axis=1), 5)
    return a.astype(np.int64), np.abs(u[:, None] - cdf).min(axis=1)


def inputs(sim, memory_in):
    """[N, 69 or 85] float32 inputs of the exported rows, from the public views."""
    x = sim.construct_obs().cpu().numpy()
    if memory_in:
        x = np.concatenate([x, sim.hidden_state_tensor().to_torch().cpu().numpy()], axis=1)
    return np.ascontiguousarray(x, dtype=np.float32)


def in_scale(x):
    """RMS of the inputs' columns' norm: what make_net divides its first layer by."""
    v = x.astype(np.float64)
    v = v[np.isfinite(v).all(axis=1)] if len(v) else v
    return float(max(1.0, np.sqrt((v * v).sum(axis=1).mean() / max(1, v.shape[1])))) if len(v) else 1.0
