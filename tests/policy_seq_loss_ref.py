"""The recurrent update on the device restated in numpy (DESIGN.md "Device
learner step", the sequence loss and the clipped Adam): the kept elements from
their definition, mbots_policy_seq_a2c_loss and mbots_policy_adam_clip operation
for operation -- float32 per element, float64 sums in the stated orders, the
chunk tree by reshapes -- so that every path is compared with it bit for bit;
and the clipped step once more in float64 with the bound on the distance."""
import numpy as np

from policy_adam_ref import ACC, END_RESET, f32

CHUNK = 1024        # kAdamChunk


def keep_mask(L, length, t0, end, last_table):
    """bool [L, B]: the harness's keep, from the definition."""
    k = np.arange(L, dtype=np.int64)[:, None]
    length, t0, end = (np.asarray(a, np.int64)[None, :] for a in (length, t0, end))
    keep = k < length
    if last_table >= 0:
        keep &= t0 + k < last_table
    return keep & ~((end == END_RESET) & (k == length - 1))


def group_rows(L, length, t0, end, order, segments, last_table):
    """int64 [G]: the kept elements of the columns the groups' segments name."""
    per_col = keep_mask(L, length, t0, end, last_table).sum(axis=0)
    return np.array([sum(int(per_col[order[lo:hi]].sum()) for lo, hi in four) for four in segments], np.int64)


def seq_loss_f32(logp, value, entropy, adv, ret, length, t0, end, order, segments, rows, last_table, value_coef=0.5,
                 entropy_coef=0.01, loss=None):
    """(g_logp, g_value, g_entropy, loss, per) as mbots_policy_seq_a2c_loss
    leaves them -- float32 [L, B] x 3, float64 [G] -- and per, float32 [L, B]:
    every counted element's share of the loss, 0 elsewhere."""
    L, B = logp.shape
    G = len(segments)
    vc, ec = f32(value_coef), f32(entropy_coef)
    keep = keep_mask(L, length, t0, end, last_table)
    g = [np.zeros((L, B), f32) for _ in range(3)]
    per = np.zeros((L, B), f32)
    loss = np.zeros(G, np.float64) if loss is None else loss.copy()
    for u in range(G):
        if not rows[u]:
            continue
        w = f32(1.0) / f32(int(rows[u]))
        group_sum = 0.0
        for s in range(4):
            lo, hi = int(segments[u][s][0]), int(segments[u][s][1])
            acc = [0.0] * ACC
            for i, b in enumerate(order[lo:hi].tolist()):
                ks = np.nonzero(keep[:, b])[0]
                na = -adv[ks, b]
                d = value[ks, b] - ret[ks, b]
                g[0][ks, b] = na * w
                g[1][ks, b] = ((f32(2.0) * vc) * d) * w
                g[2][ks, b] = (-ec) * w
                row = ((na * logp[ks, b] + vc * (d * d)) - ec * entropy[ks, b]) * w
                assert row.dtype == f32
                per[ks, b] = row
                for x in row.tolist():          # ascending k into accumulator i mod 256
                    acc[i % ACC] += x
            q = 0.0
            for a in acc:
                q += a
            group_sum += q
        loss[u] += group_sum
    return g[0], g[1], g[2], loss, per


def chunk_sq(g):
    """The squared norm of one chunk (<= 1024 float32): 256 accumulators of
    four exact squares each, then the tree."""
    x = np.zeros(CHUNK, np.float64)
    x[:len(g)] = np.asarray(g, np.float64)
    x = (x * x).reshape(CHUNK // 4, 4)
    a = ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]
    h = CHUNK // 8
    while h:
        a = a[:h] + a[h:2 * h]
        h //= 2
    return float(a[0])


def tensor_sq(g):
    g = np.asarray(g, f32).reshape(-1)
    total = 0.0
    for base in range(0, len(g), CHUNK):
        total += chunk_sq(g[base:base + CHUNK])
    return total


def group_normsq(tensors, groups):
    """float64 [groups]: tensors [(param, grad, m, v, group)], grad None passed over."""
    n2 = [0.0] * groups
    for _, g, _, _, u in tensors:
        if g is not None and g.size:
            n2[u] += tensor_sq(g)
    return np.array(n2, np.float64)


def clip_coef(normsq, max_norm):
    """(nrm, coef) float32 of one group."""
    nrm = f32(np.sqrt(np.float64(normsq)))
    coef = f32(1.0)
    if max_norm is not None and 0.0 < max_norm < float("inf"):
        with np.errstate(over="ignore", invalid="ignore"):
            c = f32(max_norm) / (nrm + f32(1e-6))
        if c < f32(1.0):
            coef = c
    return nrm, coef


def adam_clip_f32(tensors, state, rows, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None):
    """One mbots_policy_adam_clip call in place (policy_adam_ref.adam_f32's
    arguments); returns grad_norm float32 [G]."""
    G = len(state)
    lr32, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    om1, om2 = f32(1.0) - b1, f32(1.0) - b2
    lw = lr32 * f32(weight_decay)
    clip = max_norm is not None and 0.0 < max_norm < float("inf")
    n2 = group_normsq(tensors, G)
    norms, coefs = zip(*(clip_coef(x, max_norm) for x in n2))
    live = [bool(np.isfinite(n2[u])) and (rows is None or bool(rows[u])) for u in range(G)]
    for p, g, m, v, u in tensors:
        if g is None or not live[u]:
            continue
        _, b1t, b2t = state[u]
        c1, c2 = f32(1.0) - b1t * b1, f32(1.0) - b2t * b2
        gc = g * coefs[u] if clip else g
        if weight_decay:
            p[...] = p - lw * p
        m[...] = b1 * m + om1 * gc
        v[...] = b2 * v + (om2 * gc) * gc
        p[...] = p - (lr32 * (m / c1)) / (np.sqrt(v / c2) + eps)
        assert all(a.dtype == f32 for a in (p, m, v, gc))
    for u, (t, b1t, b2t) in enumerate(state):
        if live[u]:
            state[u] = (t + 1, b1t * b1, b2t * b2)
    return np.array(norms, f32)


def adam_clip_f64(p, g, m, v, t, normsq, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None):
    """(p', bound) of step t + 1 of one tensor in float64 from the float32
    state and the group's real squared norm: the real powers of the betas and
    the real clip factor; bound is DESIGN.md's on |p'_f32 - p'|."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2, lr, eps = float(f32(betas[0])), float(f32(betas[1])), float(f32(lr)), float(f32(eps))
    lw = float(f32(lr) * f32(weight_decay))
    coef = 1.0
    if max_norm is not None and 0.0 < max_norm < float("inf"):
        coef = min(1.0, float(f32(max_norm)) / (np.sqrt(normsq) + float(f32(1e-6))))
    gc = g * coef
    p1 = p - lw * p
    c1, c2 = 1.0 - b1 ** (t + 1), 1.0 - b2 ** (t + 1)
    m1 = b1 * m + (1.0 - b1) * gc
    v1 = b2 * v + (1.0 - b2) * gc * gc
    den = np.sqrt(v1 / c2) + eps
    out = p1 - lr * (m1 / c1) / den
    scale = lr * (np.abs(b1 * m) + np.abs((1.0 - b1) * gc)) / c1 / den
    bound = 2.0 * 2.0 ** -24 * (np.abs(out) + np.abs(p1) + np.abs(lw * p) + 24.0 * scale)
    return out, bound
