"""float64 geometry of the sensor's spec, independent of the
oracle's float32 predicates: the single-pair helpers the known-answer tests
use (ref_disc / ref_box) and a whole-scene renderer built on the same
geometry (render_scene), which says per ray what it sees -- an agent's
species, food, a wall, nothing -- and whether the ray is too close to a
decision boundary to hold float32 code to it."""
import numpy as np

R_AGENT, NEAR = 0.92, 1.1
IN_LO, IN_HI_X, IN_HI_Y = 0.2, 127.8, 95.8        # the wall boxes' inner faces
OUT_LO, OUT_HI_X, OUT_HI_Y = -0.2, 128.2, 96.2    # ... and outer faces
RAY_U = np.array([(2 * k - 23) / 24 for k in range(24)] + [(2 * (k - 24) - 7) / 8 for k in range(24, 32)] + [0.0])
RAY_SIGN = np.array([1.0] * 24 + [-1.0] * 8 + [1.0])
SEM_WALL, SEM_FOOD, SEM_MISS = 5, 6, -1
MARGIN = 1e-4


def dirs(heading):
    """World directions of the 33 rays (float64): 24 forward, 8 backward, finder."""
    hx, hy = heading
    out = []
    for k in range(33):
        u = (2 * k - 23) / 24 if k < 24 else ((2 * (k - 24) - 7) / 8 if k < 32 else 0.0)
        sg = -1.0 if 24 <= k < 32 else 1.0
        out.append((sg * (hx + u * hy), sg * (hy - u * hx)))
    return np.array(out)


def ref_disc(agent, heading, centre, R=R_AGENT):
    """Independent float64 restatement: ray k sees the disc iff it leaves it at
    distance >= 1.1; returns (hit[33], margin[33]) -- margin: how far the ray
    is from either decision boundary (tangency, t_exit = 1.1)."""
    d = dirs(heading)
    d /= np.linalg.norm(d, axis=1)[:, None]
    v = np.array(centre, np.float64) - np.array(agent, np.float64)
    tm = d @ v
    dist2 = v @ v - tm * tm
    half = np.sqrt(np.maximum(R * R - dist2, 0.0))
    hit = (dist2 <= R * R) & (tm + half >= NEAR)
    margin = np.minimum(np.abs(R * R - dist2), np.where(dist2 <= R * R, np.abs(tm + half - NEAR), 1.0))
    return hit, margin


def ref_box(agent, heading, centre, rot22):
    """float64 slab restatement for a food square (rotation = quarter-turn
    fraction * pi/2): hit iff the ray's parameter interval in the square is
    non-empty and it exits at distance >= 1.1."""
    w = rot22 * (np.pi / 2) / 4194304.0
    a1 = np.array([np.cos(w), np.sin(w)])
    a2 = np.array([-np.sin(w), np.cos(w)])
    d = dirs(heading)
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = np.array(agent, np.float64) - np.array(centre, np.float64)
    lo = np.full(33, -np.inf)
    hi = np.full(33, np.inf)
    for ax in (a1, a2):
        b = d @ ax
        m = o @ ax
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (-1.0 - m) / b, (1.0 - m) / b
        lo = np.maximum(lo, np.where(b != 0, np.minimum(t1, t2), np.where(abs(m) <= 1, -np.inf, np.inf)))
        hi = np.minimum(hi, np.where(b != 0, np.maximum(t1, t2), np.where(abs(m) <= 1, np.inf, -np.inf)))
    hit = (lo <= hi) & (hi >= NEAR)
    margin = np.minimum(np.abs(hi - lo), np.abs(hi - NEAR))
    return hit, margin


def quantum(z):
    """the spacing of the 14-bit-mantissa depth grid (zq) at depth z"""
    z = np.maximum(np.asarray(z, np.float64), 1e-30)
    return np.exp2(np.floor(np.log2(z)) - 14.0)


def zq(z):
    q = quantum(z)
    return np.where(np.asarray(z) > 0, np.floor(z / q) * q, 0.0)


def render_scene(position, rotation_wz, species, food):
    """What each of every agent's 32 pixels sees: (sem[n, 32] int -- species
    1..4, 6 food, 5 wall, -1 nothing --, skip[n, 32] bool).  Per ray: discs of
    radius 0.92 and rotated +-1 squares it leaves beyond the near sphere, each
    at its one view depth (f - R; the nearest corner's), the lexicographic
    minimum of (quantised depth, order), then the walls by the near point's
    class.  skip: a predicate that could change the winner lies within 1e-4 of
    its boundary, the best two depths are less than a depth quantum apart
    (unless both sit well inside one bucket of the quantised depth, where the
    order decides), or the winner is within 1e-4 of the wall comparison."""
    pos = np.asarray(position, np.float64)
    rot = np.asarray(rotation_wz, np.float64)
    n = len(pos)
    vx = 1.0 - 2.0 * rot[:, 1] ** 2
    vy = 2.0 * rot[:, 1] * rot[:, 0]
    ln = np.hypot(vx, vy)
    H = np.stack([vx / ln, vy / ln], axis=1)
    food = np.asarray(food).reshape(-1, 4)
    sem = np.zeros((n, 32), np.int64)
    skip = np.zeros((n, 32), bool)
    for i in range(n):
        a, h = pos[i], H[i]
        D = dirs(h)[:32]                            # per unit view depth
        Dn = D / np.linalg.norm(D, axis=1)[:, None]
        sg = RAY_SIGN[:32]
        zs, hits, margins, kinds, orders = [], [], [], [], []
        others = np.array([j for j in range(n) if j != i], np.int64)
        if len(others):
            V = pos[others] - a                     # [m, 2]
            tm = V @ Dn.T                           # [m, 32]
            d2 = (V * V).sum(1)[:, None] - tm * tm
            half = np.sqrt(np.maximum(R_AGENT ** 2 - d2, 0.0))
            hit = (d2 <= R_AGENT ** 2) & (tm + half >= NEAR)
            mg = np.minimum(np.abs(R_AGENT ** 2 - d2), np.where(d2 <= R_AGENT ** 2, np.abs(tm + half - NEAR), 1.0))
            f = V @ h
            raw = sg[None, :] * f[:, None] - R_AGENT
            zs.append(raw); hits.append(hit); margins.append(mg); kinds.append(np.asarray(species)[others])
            orders.append(64 + others)
        for kf, (c, X, Y, r) in enumerate(food):
            hit, mg = ref_box(a, h, (float(X), float(Y)), int(r))
            w = r * (np.pi / 2) / 4194304.0
            p = np.cos(w) * h[0] + np.sin(w) * h[1]
            q = np.cos(w) * h[1] - np.sin(w) * h[0]
            f = (np.array([X, Y], np.float64) - a) @ h
            raw = sg * f - (abs(p) + abs(q))
            zs.append(raw[None, :]); hits.append(hit[None, :32]); margins.append(mg[None, :32])
            kinds.append(np.array([SEM_FOOD]))
            orders.append(np.array([1 + kf]))
        if zs:
            RAW, Hh, M, K = np.concatenate(zs), np.concatenate(hits), np.concatenate(margins), np.concatenate(kinds)
            ORD = np.concatenate(orders)
        else:
            RAW, Hh, M, K = np.zeros((0, 32)), np.zeros((0, 32), bool), np.ones((0, 32)), np.zeros(0, np.int64)
            ORD = np.zeros(0, np.int64)
        Z = np.maximum(RAW, 0.0)                    # view depths clamp at 0
        P0 = a[None, :] + NEAR * Dn                 # the rays' near points
        for k in range(32):
            sure = Hh[:, k] & (M[:, k] > MARGIN)
            unsure = M[:, k] <= MARGIN
            zk = Z[:, k]
            obj, bad = None, False
            if sure.any():
                idx = np.nonzero(sure)[0]
                o = idx[np.argsort(zk[idx], kind="stable")]
                obj = o[0]
                zb = zk[obj]
                close = o[zk[o] - zb < quantum(zb)]
                if (K[close] != K[obj]).any():
                    # less than a quantum apart: a doubt, unless all of them sit
                    # well inside one depth bucket (both clamped to 0, say) --
                    # then the order decides, as the spec says
                    zc, rc = zk[close], RAW[close, k]
                    b = zq(zc)
                    eps = 1e-6 * (1.0 + zc)
                    firm = np.where(zc > 0, (zc - b > eps) & (b + quantum(zc) - zc > eps), rc < -1e-6)
                    if firm.all() and (b == b[0]).all():
                        obj = close[np.argmin(ORD[close])]
                    else:
                        bad = True
                if (unsure & (zk < zb + quantum(zb))).any():
                    bad = True
            elif unsure.any():
                bad = True
            px, py = P0[k]
            edges = [abs(px - e) for e in (IN_LO, IN_HI_X, OUT_LO, OUT_HI_X, 0.0, 128.0)] + \
                    [abs(py - e) for e in (IN_LO, IN_HI_Y, OUT_LO, OUT_HI_Y, 0.0, 96.0)]
            if min(edges) < MARGIN:
                bad = True
            dx, dy = D[k]
            inner = IN_LO <= px <= IN_HI_X and IN_LO <= py <= IN_HI_Y
            xs, ys = 0.0 <= px <= 128.0, 0.0 <= py <= 96.0
            bx = OUT_LO <= px <= IN_LO or IN_HI_X <= px <= OUT_HI_X
            by = OUT_LO <= py <= IN_LO or IN_HI_Y <= py <= OUT_HI_Y
            if inner:
                out = SEM_WALL
                if obj is not None:
                    z = float(zq(zk[obj]))
                    beats = True
                    for d, o_, lo_, hi_ in ((dx, a[0], IN_LO, IN_HI_X), (dy, a[1], IN_LO, IN_HI_Y)):
                        if d != 0.0:
                            T = (hi_ if d > 0 else lo_) - o_
                            if abs(z * d - T) < MARGIN:
                                bad = True
                            beats &= abs(z * d) < abs(T)
                    if beats:
                        out = K[obj]
            elif (bx and ys) or (by and xs):
                out = SEM_WALL
                bad = min(edges) < MARGIN           # objects cannot change a wall-box ray
            else:
                out = K[obj] if obj is not None else SEM_MISS
            sem[i, k] = out
            skip[i, k] = bad
    return sem, skip
