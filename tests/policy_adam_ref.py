"""The device learner step restated in numpy (DESIGN.md "Device learner
step"): mbots_policy_a2c_loss and mbots_policy_adam operation for operation in
float32 -- numpy's f32 + - * / and sqrt round correctly, so the restatement is
exact and the library is compared with it bit for bit -- and both once more in
float64, for the distance to the real-number result."""
import numpy as np

f32 = np.float32
END_RESET = 2       # MBOTS_TRAJ_END_RESET
ACC = 256           # the f64 accumulators of a (group, species) segment


def loss_f32(logp, value, entropy, adv, ret, end, segments, rows, value_coef=0.5, entropy_coef=0.01, loss=None):
    """(g_logp, g_value, g_entropy, loss) as mbots_policy_a2c_loss leaves them:
    float32 [n] x 3 and float64 [G] (added to `loss` when given)."""
    n, G = len(logp), len(segments)
    vc, ec = f32(value_coef), f32(entropy_coef)
    g = [np.zeros(n, f32) for _ in range(3)]
    loss = np.zeros(G, np.float64) if loss is None else loss.copy()
    for u in range(G):
        scale = f32(1.0) / f32(int(rows[u])) if rows[u] else f32(0.0)
        group_sum = 0.0
        for s in range(4):
            lo, hi = int(segments[u][s][0]), int(segments[u][s][1])
            r = slice(lo, hi)
            keep = np.ones(hi - lo, f32) if end is None else (np.asarray(end[r]) != END_RESET).astype(f32)
            w = keep * scale
            na = -adv[r]
            d = value[r] - ret[r]
            g[0][r] = na * w
            g[1][r] = ((f32(2.0) * vc) * d) * w
            g[2][r] = (-ec) * w
            per_row = ((na * logp[r] + vc * (d * d)) - ec * entropy[r]) * w
            assert per_row.dtype == f32 and g[1].dtype == f32
            # row i into accumulator i mod 256 in ascending i (the +0 padding changes no accumulator)
            pad = np.zeros((len(per_row) + ACC - 1) // ACC * ACC, np.float64)
            pad[:len(per_row)] = per_row
            acc = np.zeros(ACC, np.float64)
            for chunk in pad.reshape(-1, ACC):
                acc = acc + chunk
            q = 0.0
            for a in acc.tolist():
                q += a
            group_sum += q
        loss[u] += group_sum
    return g[0], g[1], g[2], loss


def loss_f64(logp, value, entropy, adv, ret, end, segments, rows, value_coef=0.5, entropy_coef=0.01):
    """The same quantities in float64 from the float32 inputs."""
    n, G = len(logp), len(segments)
    c = [np.asarray(a, np.float64) for a in (logp, value, entropy, adv, ret)]
    g = [np.zeros(n) for _ in range(3)]
    loss = np.zeros(G)
    for u in range(G):
        scale = 1.0 / float(rows[u]) if rows[u] else 0.0
        for s in range(4):
            r = slice(int(segments[u][s][0]), int(segments[u][s][1]))
            keep = 1.0 if end is None else (np.asarray(end[r]) != END_RESET).astype(np.float64)
            w = keep * scale
            d = c[1][r] - c[4][r]
            g[0][r], g[1][r], g[2][r] = -c[3][r] * w, 2.0 * value_coef * d * w, -entropy_coef * w
            loss[u] += float(np.sum((-c[3][r] * c[0][r] + value_coef * d * d - entropy_coef * c[2][r]) * w))
    return g[0], g[1], g[2], loss


def adam_state(groups):
    """struct mbots_policy_adam_state [groups] at the start: (t, b1t, b2t)."""
    return [(0, f32(1.0), f32(1.0)) for _ in range(groups)]


def adam_f32(tensors, state, rows, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
    """One mbots_policy_adam call in place: tensors [(param, grad, m, v,
    group)] float32 arrays (grad None: passed over), state adam_state()'s
    list, rows a [G] sequence or None."""
    lr, b1, b2, eps = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)
    om1, om2 = f32(1.0) - b1, f32(1.0) - b2
    for p, g, m, v, u in tensors:
        if g is None or (rows is not None and not rows[u]):
            continue
        _, b1t, b2t = state[u]
        c1, c2 = f32(1.0) - b1t * b1, f32(1.0) - b2t * b2
        m[...] = b1 * m + om1 * g
        v[...] = b2 * v + (om2 * g) * g
        p[...] = p - (lr * (m / c1)) / (np.sqrt(v / c2) + eps)
        assert all(a.dtype == f32 for a in (p, m, v)) and type(c1) is f32
    for u, (t, b1t, b2t) in enumerate(state):
        if rows is None or rows[u]:
            state[u] = (t + 1, b1t * b1, b2t * b2)


def adam_f64(p, g, m, v, t, lr=3e-4, betas=(0.9, 0.999), eps=1e-8):
    """(p', delta) of step t + 1 in float64 from the float32 state: the real
    powers of the betas, no rounding that float32 would see."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = float(f32(betas[0])), float(f32(betas[1]))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    delta = float(f32(lr)) * (m1 / (1.0 - b1 ** (t + 1))) / (np.sqrt(v1 / (1.0 - b2 ** (t + 1))) + float(f32(eps)))
    return p - delta, delta
