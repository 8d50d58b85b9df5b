"""numpy restatements of PPO on the device (include/mbots.h "PPO on the
device"): the per-row arithmetic operation for operation in float32 -- the
device actor's exp included -- and the two-level order of the float64 sums, so
that the library's results are compared bit for bit; with dtype=np.float64 the
same formulas serve as the accurate reference."""
import numpy as np

CHUNK = 4096          # kPpoChunk: rows of a chunk
SEQ_CHUNK = 512       # kPpoSeqChunk: column positions of a chunk
ACC = 256             # kLossAcc
END_RESET = 2
F = np.float32


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the device actor's exp (mbots_policy.hpp pol_exp) ----
def fma32(a, b, c):
    """fmaf: a * b + c of float32 arrays rounded once.  The product is exact in
    float64; the sum is rounded to odd there (its error term from TwoSum), after
    which the rounding to float32 is the only one that counts."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


LN2_HI, LN2_LO, LOG2E = F(0.693145751953125), F(1.42860654e-6), F(1.44269504)


def pow2(n):
    return ((n.astype(np.int64) + 127) << 23).astype(np.uint32).view(np.float32)


def pol_exp(x):
    x = np.asarray(x, np.float32)
    safe = np.where((x == x) & (x <= F(88.72284)) & (x >= F(-104.0)), x, F(0.0))
    t = safe * LOG2E
    n = (t + np.where(t < 0, F(-0.5), F(0.5))).astype(np.int32)      # truncates, as the C cast
    nf = n.astype(np.float32)
    r = fma32(nf, -LN2_LO, fma32(nf, -LN2_HI, safe))
    q = np.full_like(r, F(1.0) / F(40320.0))
    for c in (F(1.0) / F(5040.0), F(1.0) / F(720.0), F(1.0) / F(120.0), F(1.0) / F(24.0), F(1.0) / F(6.0), F(0.5)):
        q = fma32(q, r, c)
    p = fma32(r * r, q, r) + F(1.0)
    n1 = n >> 1
    with np.errstate(over="ignore"):
        y = (p * pow2(n1)) * pow2(n - n1)
    y = np.where(x > F(88.72284), F(np.inf), np.where(x < F(-104.0), F(0.0), y))
    return np.where(x == x, y, x).astype(np.float32)


# ---- the per-row arithmetic (pol_ppo_row) ----
def norm_constants(moments, g, dtype=np.float32):
    """(mean, inv) of group g from moments [G, 3] (None: no normalisation)."""
    if moments is None:
        return None
    n, s1, s2 = (np.float64(v) for v in moments[g])
    if not n >= 2.0:
        return dtype(0.0), dtype(1.0)
    mu = s1 / n
    var = (s2 - s1 * mu) / (n - 1.0)
    if not var > 0.0:
        var = np.float64(0.0)
    if dtype is np.float32:
        return F(mu), F(1.0) / (F(np.sqrt(var)) + F(1e-8))
    return mu, 1.0 / (np.sqrt(var) + 1e-8)


def ppo_rows(logp, value, entropy, old_logp, old_value, adv, ret, w, norm, clip, value_clip, value_coef, entropy_coef,
             dtype=np.float32):
    """pol_ppo_row over arrays: (g_logp, g_value, g_entropy, st [n, 6], aux).
    min(a, b) is b < a ? b : a and max(a, b) is b > a ? b : a."""
    T = dtype
    logp, value, entropy, old_logp, adv, ret, w = (np.asarray(x, T) for x in (logp, value, entropy, old_logp, adv, ret, w))
    if T is np.float32:
        lo_c, hi_c = F(1.0) - F(clip), F(1.0) + F(clip)
        vcoef, ecoef = F(value_coef), F(entropy_coef)
        exp = pol_exp
    else:
        lo_c, hi_c, vcoef, ecoef = 1.0 - float(F(clip)), 1.0 + float(F(clip)), float(F(value_coef)), float(F(entropy_coef))
        exp = np.exp

    def mn(a, b):
        return np.where(b < a, b, a)

    def mx(a, b):
        return np.where(b > a, b, a)
    A = adv if norm is None else (adv - T(norm[0])) * T(norm[1])
    lr = logp - old_logp
    ratio = exp(lr)
    s1 = ratio * A
    rc = mn(mx(ratio, lo_c), hi_c)
    s2 = rc * A
    pol = -mn(s1, s2)
    g_logp = np.where(s2 < s1, T(0.0), -s1) * w
    d = value - ret
    v1 = d * d
    vclip = value_clip is not None and value_clip > 0 and old_value is not None
    aux = dict(A=A, ratio=ratio, rc=rc, s1=s1, s2=s2, v1=v1, lr=lr)
    if vclip:
        old_value = np.asarray(old_value, T)
        vc = T(F(value_clip))
        dv = value - old_value
        dc = mn(mx(dv, -vc), vc)
        d2 = (old_value + dc) - ret
        v2 = d2 * d2
        vl = np.where(v2 > v1, v2, v1)
        g_value = (vcoef * np.where(v2 > v1, np.where(dc == dv, T(2.0) * d2, T(0.0)), T(2.0) * d)) * w
        aux.update(v2=v2, dv=dv, dc=dc)
    else:
        vl = v1
        g_value = ((T(2.0) * vcoef) * d) * w
    g_entropy = np.broadcast_to(-ecoef, w.shape) * w
    st = np.stack([((pol + vcoef * vl) - ecoef * entropy) * w, pol * w, vl * w, entropy * w,
                   ((ratio - T(1.0)) - lr) * w, np.where(rc != ratio, T(1.0), T(0.0)) * w], axis=-1)
    return g_logp.astype(T), g_value.astype(T), g_entropy.astype(T), st.astype(T), aux


# ---- the two-level order ----
def two_level(X, chunk):
    """X [K, n, S] float64: element i's K shares (in ascending k) of S sums.
    Element i into accumulator i mod 256 of chunk i // chunk; the accumulators
    ascending; the chunks ascending.  (Shares that are +0 change nothing: an
    accumulator starts as +0 and never becomes -0.)"""
    K, n, S = X.shape
    seg = np.zeros(S)
    for first in range(0, n, chunk):
        blk = X[:, first:first + chunk]
        acc = np.zeros((ACC, S))
        for r0 in range(0, blk.shape[1], ACC):
            part = blk[:, r0:r0 + ACC]
            for k in range(K):
                acc[:part.shape[1]] += part[k]
        q = np.zeros(S)
        for j in range(ACC):
            q = q + acc[j]
        seg = seg + q
    return seg


def group_sum(out, g, per_species):
    tot = np.zeros(out.shape[1])
    for q in per_species:
        tot = tot + q
    out[g] = out[g] + tot


def scale_of(rows_g):
    return F(1.0) / F(rows_g) if rows_g != 0 else F(0.0)


def moments_rows(adv, end, segments, moments=None, chunk=CHUNK):
    G = segments.shape[0]
    out = np.zeros((G, 3)) if moments is None else moments.copy()
    a = np.asarray(adv, np.float32).reshape(-1).astype(np.float64)
    keep = np.ones(a.shape, bool) if end is None else np.asarray(end).reshape(-1) != END_RESET
    X = np.where(keep[:, None], np.stack([np.ones_like(a), a, a * a], -1), 0.0)
    for g in range(G):
        group_sum(out, g, [two_level(X[None, lo:hi], chunk) for lo, hi in segments[g]])
    return out


def loss_rows(cols, end, segments, rows, clip=0.2, value_clip=None, value_coef=0.5, entropy_coef=0.01, moments=None,
              stats=None, chunk=CHUNK, dtype=np.float32):
    """mbots_policy_ppo_loss: cols = (logp, value, entropy, old_logp, old_value
    or None, adv, ret).  Returns (g_logp, g_value, g_entropy, stats, aux) -- aux:
    per row A, ratio, rc, s1, s2, v1 (v2, dv, dc), and `seg`, the rows that lie
    in a segment."""
    n, G = len(cols[0]), segments.shape[0]
    out = np.zeros((G, 6)) if stats is None else stats.copy()
    g3 = [np.zeros(n, dtype) for _ in range(3)]
    aux = {"seg": np.zeros(n, bool)}
    for g in range(G):
        per = []
        for lo, hi in segments[g]:
            sl = slice(lo, hi)
            keep = np.ones(hi - lo, dtype) if end is None else (np.asarray(end)[sl] != END_RESET).astype(dtype)
            w = keep * dtype(scale_of(rows[g]))
            c = [None if x is None else np.asarray(x)[sl] for x in cols]
            gl, gv, ge, st, ax = ppo_rows(*c, w, norm_constants(moments, g, dtype), clip, value_clip, value_coef,
                                          entropy_coef, dtype)
            g3[0][sl], g3[1][sl], g3[2][sl] = gl, gv, ge
            aux["seg"][sl] = True
            for k, v in ax.items():
                aux.setdefault(k, np.zeros(n, dtype))[sl] = v
            per.append(two_level(st.astype(np.float64)[None], chunk))
        group_sum(out, g, per)
    return g3[0], g3[1], g3[2], out, aux


# ---- the sequence twins ----
def seq_kept(length, t0, end, last_table, L):
    m = np.minimum(np.asarray(length, np.int64), L)
    full = m.copy()
    if last_table >= 0:
        m = np.minimum(m, np.maximum(np.int64(last_table) - np.asarray(t0, np.int64), 0))
    m = m - ((np.asarray(end) == END_RESET) & (m == full))
    return np.where(full <= 0, 0, m)


def _seq_positions(order, lo, hi, kept, B):
    cols = np.asarray(order[lo:hi], np.int64)
    ok = (cols >= 0) & (cols < B)
    cols = np.where(ok, cols, 0)
    return cols, np.where(ok, kept[cols], 0)


def moments_seq(adv, length, t0, end, order, segments, last_table=-1, moments=None, chunk=SEQ_CHUNK):
    L, B = adv.shape
    G = segments.shape[0]
    out = np.zeros((G, 3)) if moments is None else moments.copy()
    kept = seq_kept(length, t0, end, last_table, L)
    a = np.asarray(adv, np.float32).astype(np.float64)
    for g in range(G):
        per = []
        for lo, hi in segments[g]:
            cols, nk = _seq_positions(order, lo, hi, kept, B)
            x = a[:, cols]
            X = np.where((np.arange(L)[:, None] < nk[None, :])[..., None], np.stack([np.ones_like(x), x, x * x], -1), 0.0)
            per.append(two_level(X.reshape(L, len(cols), 3), chunk))
        group_sum(out, g, per)
    return out


def loss_seq(cols, length, t0, end, order, segments, rows, last_table=-1, clip=0.2, value_clip=None, value_coef=0.5,
             entropy_coef=0.01, moments=None, stats=None, chunk=SEQ_CHUNK):
    """mbots_policy_seq_ppo_loss over [L, B] arrays: (g_logp, g_value,
    g_entropy, stats)."""
    L, B = cols[0].shape
    G = segments.shape[0]
    out = np.zeros((G, 6)) if stats is None else stats.copy()
    g3 = [np.zeros((L, B), np.float32) for _ in range(3)]
    kept = seq_kept(length, t0, end, last_table, L)
    for g in range(G):
        if rows[g] == 0:
            continue
        per = []
        for lo, hi in segments[g]:
            pos, nk = _seq_positions(order, lo, hi, kept, B)
            mask = np.arange(L)[:, None] < nk[None, :]
            c = [None if x is None else np.asarray(x)[:, pos] for x in cols]
            w = np.full((L, len(pos)), scale_of(rows[g]), np.float32)
            gl, gv, ge, st, _ = ppo_rows(*c, w, norm_constants(moments, g), clip, value_clip, value_coef, entropy_coef)
            kk, pp = np.nonzero(mask)
            for dst, src in zip(g3, (gl, gv, ge)):
                dst[kk, pos[pp]] = src[kk, pp]
            per.append(two_level(np.where(mask[..., None], st.astype(np.float64), 0.0), chunk))
        group_sum(out, g, per)
    return g3[0], g3[1], g3[2], out


def gate(gate_in, rows, stats, target_kl):
    kl = stats[:, 4]
    with np.errstate(invalid="ignore"):
        return np.where((gate_in != 0) & (rows != 0) & (kl <= target_kl), rows, 0).astype(np.int64)
