"""Exact-geometry scenes for the sensor and the K1 finder cull (pure numpy).

A scene is a function (n, rng) -> (position[n, 2] f32, rotation_wz[n, 2] f32,
food[k, 4] i32 of (chunk, x, y, rotation)) for a world of n agents, written
with set_world_state on both the product and the oracle.  Slots 0..7 -- one
key chunk of the HIP sensor -- are the cameras a scene is aimed at; every
other agent is a camera too, and is compared all the same.

The sensor's cull constants are restated here on purpose (never imported): a
constant changed in the kernel without a changed test then shows in review.
Every heading is one the simulator produces: k rotation steps applied to
(1, 0) in float32.  Every placement that is about a threshold is checked in
float32 with the oracle's own expression order (v = c - a, f = vx hx + vy hy,
l = vx hy - vy hx) before it is returned: `solve` searches the float32
neighbours of the intended point for one whose quantity is below / equal to /
above the threshold and asserts the relation it returns.  Equality is returned
only where some neighbour attains it (the two sides are always there).
"""
import numpy as np

F = np.float32

# ---- restated constants, one reason each -----------------------------------
ROT_C, ROT_S = F(0.99875026039496624), F(0.04997916927067833)  # actionSystem's rotation step
R_AGENT = F(0.92)          # disc radius of an agent in the rays' plane
NEAR = F(1.1)              # near sphere: a ray sees what it leaves beyond this
SQ_HALF_DIAG = 1.42        # the cull's bound of a food square's half diagonal (sqrt 2)
WEDGE_PAD = 0.05           # P1 wedge: |l| <= |f| + sqrt(2) R' + 0.05
FAR_CULL = F(5.0)          # P1 angular cull applies from this |f| on
CULL_U = 1e-4              # ... with this margin in u
U_EPS = 2e-3               # root-interval margin in u of the far-pair pixel range
CIRCLE_FAR = F(1.5)        # discs: near (exact per pixel) / far (root interval) switch in |f|
FOOD_FAR = F(2.55)         # squares: the same switch
INSIDE_NEAR = F(0.17)      # disc centres this close are wholly inside the near sphere
TOUCH = F(F(1.1) - F(0.92))  # a disc straight ahead starts to reach past the near sphere here
FINDER_L, FINDER_F = F(1.45), F(-0.35)  # K1 finder pass: keeps |l| <= 1.45 and f >= -0.35
KEY_AGENTS = 8             # cameras per key chunk
LX, LY = 127.0, 95.0       # actionSystem's clamp: x in [0, 127], y in [0, 95]
IN_LO, IN_HI_X, IN_HI_Y = F(0.2), F(F(128.0) - F(0.2)), F(F(96.0) - F(0.2))  # inner wall faces

HEADINGS = (0, 16, 8, 37)  # rotation steps: +x, ~+y (axis-swapped, 1.6 rad), two oblique (0.8, 3.7 rad)


def ray_u(k):
    """pixel k's offset (24 forward, 8 backward, 32: the finder ray)"""
    if k < 24:
        return F(2 * k - 23) * F(1.0 / 24.0)
    if k < 32:
        return F(2 * (k - 24) - 7) * F(0.125)
    return F(0.0)


def rot_wz(k):
    """(rw, rz) after k left rotation steps from (1, 0), float32 as actionSystem"""
    assert 0 <= k <= 125
    w, z = F(1.0), F(0.0)
    for _ in range(k):
        w, z = F(w * ROT_C) - F(z * ROT_S), F(w * ROT_S) + F(z * ROT_C)
    return w, z


def heading(w, z):
    """the sensor's heading of a rotation (Quat::rotateVec({1,0,0}), normalised)"""
    vx = F(1.0) - F(2.0) * F(z * z)
    vy = F(2.0) * F(z * w)
    ln = np.sqrt(F(F(vx * vx) + F(vy * vy)))
    return F(vx / ln), F(vy / ln)


_HEAD = {}


def head_of(k):
    if k not in _HEAD:
        _HEAD[k] = heading(*rot_wz(k))
    return _HEAD[k]


def fl(ax, ay, hx, hy, cx, cy):
    """(f, l) of object c seen from camera a, float32, the oracle's order"""
    vx, vy = np.subtract(cx, ax, dtype=F), np.subtract(cy, ay, dtype=F)
    f = np.add(np.multiply(vx, hx, dtype=F), np.multiply(vy, hy, dtype=F), dtype=F)
    l = np.subtract(np.multiply(vx, hy, dtype=F), np.multiply(vy, hx, dtype=F), dtype=F)
    return f, l


def zq(z):
    """depth keys keep 14 mantissa bits (the low 9 carry the object order)"""
    b = np.asarray(z, F).view(np.uint32) & np.uint32(0xFFFFFE00)
    return b.view(F)


def q_absf(f, l):
    return np.abs(f)


def q_absl(f, l):
    return np.abs(l)


def q_f(f, l):
    return f


def q_disc_z(f, l):
    return zq(np.maximum(np.subtract(f, R_AGENT, dtype=F), F(0.0)))


def _rel(g, T, rel):
    return {"lt": g < T, "eq": g == T, "gt": g > T}[rel]


def solve(fixed, h, f_t, l_t, q=None, T=None, rel="any", move="obj", span=8, also=()):
    """The float32 point at (f_t, l_t) in the frame of the camera (move="obj":
    the camera is `fixed`, the object moves; move="cam": the object is `fixed`
    and the camera moves) whose quantity q(f, l) stands in relation rel ("lt",
    "eq", "gt") to T, nearest to T; None when no float32 neighbour within
    `span` ulps per coordinate inside the arena does.  also: further (q, T,
    rel) the point must satisfy; with rel="any" the point nearest (f_t, l_t)
    that satisfies them.  Every relation is asserted again on the point
    returned."""
    hx, hy = h
    sg = 1.0 if move == "obj" else -1.0
    px = float(fixed[0]) + sg * (f_t * float(hx) + l_t * float(hy))
    py = float(fixed[1]) + sg * (f_t * float(hy) - l_t * float(hx))
    if not (0.0 <= px <= LX and 0.0 <= py <= LY):
        return None
    p0 = np.array([px, py], np.float64).astype(F)
    i = np.arange(-span, span + 1, dtype=np.float64)
    X = (np.float64(p0[0]) + i * np.float64(np.spacing(max(p0[0], F(1e-3))))).astype(F)[:, None]
    Y = (np.float64(p0[1]) + i * np.float64(np.spacing(max(p0[1], F(1e-3))))).astype(F)[None, :]
    X, Y = np.broadcast_arrays(X, Y)
    fx, fy = F(fixed[0]), F(fixed[1])
    if move == "obj":
        f, l = fl(fx, fy, hx, hy, X, Y)
    else:
        f, l = fl(X, Y, hx, hy, fx, fy)
    ok = (X >= 0) & (X <= F(LX)) & (Y >= 0) & (Y <= F(LY))
    for q2, T2, rel2 in also:
        ok &= _rel(q2(f, l).astype(np.float64), float(T2), rel2)
    if rel == "any":
        cost = np.abs(f.astype(np.float64) - f_t) + np.abs(l.astype(np.float64) - l_t)
    else:
        g = q(f, l).astype(np.float64)
        T = float(T)
        ok &= _rel(g, T, rel)
        cost = np.abs(g - T) * 1e6 + np.abs(l.astype(np.float64) - l_t)
    if not ok.any():
        return None
    j = np.unravel_index(np.argmin(np.where(ok, cost, np.inf)), ok.shape)
    x, y = X[j], Y[j]
    # checked, not hoped for: recompute every relation on the returned point
    ff, ll = fl(fx, fy, hx, hy, x, y) if move == "obj" else fl(x, y, hx, hy, fx, fy)
    for q2, T2, rel2 in tuple(also) + (((q, T, rel),) if rel != "any" else ()):
        assert bool(_rel(float(q2(ff, ll)), float(T2), rel2)), (rel2, float(q2(ff, ll)), float(T2))
    return F(x), F(y)


def three_sides(fixed, h, f_t, l_t, q, T, move="obj", also=()):
    """the points just below, at (where representable) and just above T"""
    out = []
    for rel in ("lt", "eq", "gt"):
        p = solve(fixed, h, f_t, l_t, q, T, rel, move, also=also)
        if p is not None:
            out.append(p)
    if len(out) < 2 and solve(fixed, h, f_t, l_t) is not None:
        raise AssertionError(f"no float32 neighbours on both sides of {T} at {fixed}, {f_t}, {l_t}")
    return out


# the P1 wedge as the kernel writes it, |l| <= |f| + wk with
# wk = sqrt(2) (R' 1.001) + 0.05 in float32, for discs and for squares
WK_DISC = F(F(F(1.41421356) * F(R_AGENT * F(1.001))) + F(WEDGE_PAD))
WK_FOOD = F(F(F(1.41421356) * F(F(SQ_HALF_DIAG) * F(1.001))) + F(WEDGE_PAD))


def q_wedge(wk):
    """|l| - (|f| + wk): <= 0 where the wedge keeps the pair (the difference of
    the two float32 sides, exact in float64)"""
    return lambda f, l: np.abs(l).astype(np.float64) - np.add(np.abs(f), wk, dtype=F).astype(np.float64)


def q_lmf(f, l):
    """|l| - |f|, float32: the wedge family's distance from the line"""
    return np.subtract(np.abs(l), np.abs(f), dtype=F)


def q_tangent(u, s):
    """(l - u f) - s R sqrt(1 + u^2), float32: 0 where the disc's edge on side
    s touches the centre line of the ray with offset u"""
    u = F(u)
    rn = F(F(s) * F(R_AGENT * np.sqrt(F(F(1.0) + F(u * u)))))
    return lambda f, l: np.subtract(np.subtract(l, np.multiply(u, f, dtype=F), dtype=F), rn, dtype=F)


def wedge_reject_l(f_abs, wk):
    """just past the first |l| the P1 wedge rejects (solve asserts q_wedge > 0)"""
    return f_abs + float(wk) + 2e-6


# ---- assembling a world ------------------------------------------------------
def chunk_of(x, y):
    return (int(x) // 16) + (int(y) // 16) * 8


def num_cams(n):
    return min(KEY_AGENTS, max(1, n // 2))


def assemble(n, rng, cams, discs, food, discs_last=False):
    """cams: [(x, y, k)] into slots 0..; discs: [(x, y)] into the slots after
    them (discs_last: into the last slots, so their order ids pass 256 in the
    large classes), as many as fit (a random subset otherwise, kept in order);
    the rest of the world's n agents stand at random places with random
    headings.  food: [(x, y, rot)], kept while a chunk holds <= 5 and the
    world <= 30, and filled up to 12 with packages at random cells."""
    cams = cams[:n]
    room = n - len(cams)
    if len(discs) > room:
        keep = np.sort(rng.choice(len(discs), room, replace=False))
        discs = [discs[i] for i in keep]
    nfill = room - len(discs)
    pos = np.zeros((n, 2), F)
    rot = np.zeros((n, 2), F)
    fill = [(F(rng.uniform(0, LX)), F(rng.uniform(0, LY))) for _ in range(nfill)]
    body = fill + list(discs) if discs_last else list(discs) + fill
    for i, (x, y, k) in enumerate(cams):
        pos[i] = (x, y)
        rot[i] = rot_wz(k)
    for i, (x, y) in enumerate(body):
        pos[len(cams) + i] = (x, y)
        rot[len(cams) + i] = rot_wz(int(rng.integers(0, 126)))
    assert np.isfinite(pos).all() and (pos >= 0).all() and (pos[:, 0] <= LX).all() and (pos[:, 1] <= LY).all()
    # (a dozen packages at least: in a world of a thousand agents the scene's
    # own few can all be hidden behind somebody)
    food = list(food) + [(int(rng.integers(1, 127)), int(rng.integers(1, 95)), pick_rot(rng, j))
                         for j in range(max(0, 12 - len(food)))]
    per, out = {}, []
    for x, y, r in food:
        c = chunk_of(x, y)
        if not (0 <= x <= 127 and 0 <= y <= 95) or per.get(c, 0) >= 5 or len(out) >= 30:
            continue
        per[c] = per.get(c, 0) + 1
        out.append((c, int(x), int(y), int(r)))
    return pos, rot, np.array(out, np.int32).reshape(-1, 4)


def anchors(rng, nc, margin=14.0):
    """nc camera places on a 4 x 2 grid of the arena's interior, jittered"""
    pts = [(16.0 + 32.0 * (i % 4), 24.0 + 48.0 * (i // 4)) for i in range(8)]
    order = rng.permutation(8)[:nc]
    return [(pts[i][0] + rng.uniform(-2, 2), pts[i][1] + rng.uniform(-2, 2)) for i in order]


def lattice_near(x, y):
    return int(min(127, max(0, round(x)))), int(min(95, max(0, round(y))))


ROTS = (0, 1 << 21, (1 << 22) - 1)


def pick_rot(rng, i):
    return ROTS[i % 5] if i % 5 < 3 else int(rng.integers(0, 1 << 22))


# ---- family 1: regime thresholds ---------------------------------------------
def fam_thresholds(n, rng, k):
    """discs at |f| = 0.17, 1.1 - 0.92, 1.5, 5.0 and squares at |f| = 2.55, 5.0
    (below / at / above), at l = 0, |l| = R and the first l the wedge rejects"""
    h, nc = head_of(k), num_cams(n)
    off = int(rng.integers(0, 64))
    cams, discs, food = [], [], []
    for i, (ax, ay) in enumerate(anchors(rng, nc)):
        # the camera stands where its own package sits on a food threshold
        Tf = (FOOD_FAR, FAR_CULL)[(i + off) % 2]
        sgn = 1.0 if ((i + off) // 2) % 2 == 0 else -1.0
        lsel = ((i + off) // 4) % 3
        lt = (0.0, 1.0, wedge_reject_l(float(Tf), WK_FOOD))[lsel]
        also = [(), (), ((q_wedge(WK_FOOD), 0.0, "gt"),)][lsel]
        P = lattice_near(ax + sgn * float(Tf) * float(h[0]), ay + sgn * float(Tf) * float(h[1]))
        side = three_sides(P, h, sgn * float(Tf), lt, q_absf, Tf, move="cam", also=also)
        a = side[(i + off // 3) % len(side)]
        cams.append((a[0], a[1], k))
        food.append((P[0], P[1], pick_rot(rng, i + off)))
        # one side (below / at / above) and one l per camera, every disc
        # threshold, forward and backward by turns: discs of one camera then
        # differ in depth, so the float64 leg is not left with ties only.
        # |l| = R is placed just inside or just outside R (asserted), the
        # wedge's first rejected l where the kernel's expression rejects it
        lsel = ((i + off) // 3) % 4
        inout = "lt" if (i + off) % 2 else "gt"
        for j, Td in enumerate((INSIDE_NEAR, TOUCH, CIRCLE_FAR, FAR_CULL)):
            sd = 1.0 if (j + i + off) % 2 == 0 else -1.0
            lt = (0.0, float(R_AGENT), -float(R_AGENT), wedge_reject_l(float(Td), WK_DISC))[lsel]
            also = [(), ((q_absl, R_AGENT, inout),), ((q_absl, R_AGENT, inout),),
                    ((q_wedge(WK_DISC), 0.0, "gt"),)][lsel]
            side = three_sides(a, h, sd * float(Td), lt, q_absf, Td, also=also)
            discs.append(side[(i + off) % len(side)])
    return assemble(n, rng, cams, discs, food)


# ---- family 2: pixel tangency --------------------------------------------------
TANGENT_PIXELS = (0, 11, 12, 23, 24, 27, 28, 31, 32)
TANGENT_DU = (0.0, CULL_U, -CULL_U, 1.5 * U_EPS, -1.5 * U_EPS)   # 0, +-1e-4, +-3e-3: straddles both margins in u


def _far_corner(h, rng, spread):
    """a camera place in the corner the heading looks away from"""
    ax = 4.0 + rng.uniform(0, spread) if h[0] > 0 else 123.0 - rng.uniform(0, spread)
    ay = 4.0 + rng.uniform(0, spread) if h[1] > 0 else 91.0 - rng.uniform(0, spread)
    return ax, ay


def fam_tangency(n, rng, k):
    """disc edges, and food squares' corners, tangent to a pixel's centre ray
    (l = u f +- R sqrt(1 + u^2)) and 1e-4 |f|, 3e-3 |f| either side in u, at
    ranges 2, 6, 30 and 100+"""
    h, nc = head_of(k), num_cams(n)
    off = int(rng.integers(0, 1024))
    cams, discs, food = [], [], []
    for i in range(nc):
        pix = TANGENT_PIXELS[(i + off) % 9]
        u = float(ray_u(pix))
        back = 24 <= pix < 32
        dirx, diry = float(h[0]) + u * float(h[1]), float(h[1]) - u * float(h[0])
        if back:
            dirx, diry = -dirx, -diry
        hh = (dirx, diry)
        for rng_t in ((100.0, 30.0, 6.0, 2.0)[((i + off) // 9) % 4:] + (2.0,)):
            ax, ay = _far_corner(hh, rng, 24.0) if rng_t > 6 else anchors(rng, 1)[0]
            f = -rng_t if back else rng_t
            ex, ey = ax + f * (float(h[0]) + u * float(h[1])), ay + f * (float(h[1]) - u * float(h[0]))
            if 2.0 <= ex <= LX - 2.0 and 2.0 <= ey <= LY - 2.0:
                break
        a = (F(ax), F(ay))
        cams.append((a[0], a[1], k))
        for du in TANGENT_DU:
            for s in (1.0, -1.0):
                lt = (u + du) * f + s * float(R_AGENT) * np.sqrt(1.0 + u * u)
                qt = q_tangent(u, s)
                if du == 0.0:      # on the line: just either side of it, and on it where representable
                    discs += three_sides(a, h, f, lt, qt, 0.0) if solve(a, h, f, lt) is not None else []
                else:              # du f off the line, on the side it was meant for
                    p = solve(a, h, f, lt, also=((qt, 0.0, "gt" if du * f > 0 else "lt"),))
                    if p is not None:
                        discs.append(p)
    # squares: each camera also stands where one corner of a package lies on its
    # pixel's centre ray (+ du): the package is the fixed point, so this is a
    # second set of cameras in the slots after the discs' when there is room
    for i in range(nc):
        pix = TANGENT_PIXELS[(i + off + 3) % 9]
        u, back = float(ray_u(pix)), 24 <= pix < 32
        du = TANGENT_DU[(i + off) % 5]
        rot = pick_rot(rng, i + off)
        w = rot * (np.pi / 2) / 4194304.0
        cw, sw = np.cos(w), np.sin(w)
        sx, sy = ((1, 1), (1, -1), (-1, 1), (-1, -1))[(i + off) % 4]
        for t in (100.0, 30.0, 6.0, 2.0)[((i + off) // 5) % 4:]:
            d = np.array([float(h[0]) + (u + du) * float(h[1]), float(h[1]) - (u + du) * float(h[0])])
            d = -d if back else d
            ax, ay = _far_corner(d, rng, 24.0) if t > 6 else anchors(rng, 1)[0]
            P = lattice_near(ax + t * d[0], ay + t * d[1])
            corner = np.array([P[0] + sx * cw - sy * sw, P[1] + sx * sw + sy * cw])
            cam = corner - t * d
            if 0.0 <= cam[0] <= LX and 0.0 <= cam[1] <= LY and 0 < P[0] < 127 and 0 < P[1] < 95:
                food.append((P[0], P[1], rot))
                # (slots after the first cameras: a disc-less camera of its own)
                discs.insert(i, (F(cam[0]), F(cam[1])))
                break
    pos, rot_, fd = assemble(n, rng, cams, discs, food)
    # the food cameras took disc slots: give them the scene's heading
    for j in range(len(cams), min(n, len(cams) + nc)):
        rot_[j] = rot_wz(k)
    return pos, rot_, fd


# ---- family 3: the wedge line ----------------------------------------------------
WEDGE_D = (0.0, 0.05, -0.05, 0.06, -0.06)


def fam_wedge(n, rng, k):
    """pairs on |l| = |f| + sqrt(2) R' and 0.05, 0.06 either side of it, for
    the disc's R' = 0.92 and the square's 1.42 (pixels 0 and 23, |u| = 23/24,
    are the ones that can still see them)"""
    h, nc = head_of(k), num_cams(n)
    off = int(rng.integers(0, 64))
    cams, discs, food = [], [], []
    for i, (ax, ay) in enumerate(anchors(rng, nc)):
        fa = (0.2, 0.5, 1.0, 3.0, 8.0)[(i + off) % 5]
        sf = 1.0 if ((i + off) // 5) % 2 == 0 else -1.0
        sl = 1.0 if (i + off) % 2 else -1.0
        # lines in |l| - |f|: the geometric one sqrt(2) R' and 0.05, 0.06 either
        # side of it, and the kernel's own (wk: the 1.001 margin and the pad in)
        P = lattice_near(ax, ay)
        Ts = [F(1.41421356 * SQ_HALF_DIAG + d) for d in WEDGE_D]
        j = (i + off // 2) % (len(Ts) + 1)
        if j < len(Ts):
            side = three_sides(P, h, sf * fa, sl * (fa + float(Ts[j])), q_lmf, Ts[j], move="cam")
        else:
            side = three_sides(P, h, sf * fa, sl * (fa + float(WK_FOOD)), q_wedge(WK_FOOD), 0.0, move="cam")
        if side:
            a = side[(i + off // 7) % len(side)]
            food.append((P[0], P[1], pick_rot(rng, i + off)))
        else:
            a = (F(ax), F(ay))
        cams.append((a[0], a[1], k))
        for fd in (fa, (0.2, 0.5, 1.0, 3.0, 8.0)[(i + off + 2) % 5]):
            for sl in (1.0, -1.0):
                for d in WEDGE_D:
                    T = F(1.41421356 * float(R_AGENT) + d)
                    discs += three_sides(a, h, sf * fd, sl * (fd + float(T)), q_lmf, T) \
                        if solve(a, h, sf * fd, sl * (fd + float(T))) is not None else []
                discs += three_sides(a, h, sf * fd, sl * (fd + float(WK_DISC)), q_wedge(WK_DISC), 0.0) \
                    if solve(a, h, sf * fd, sl * (fd + float(WK_DISC))) is not None else []
    return assemble(n, rng, cams, discs, food)


# ---- family 4: depth ties and order ------------------------------------------------
def fam_ties(n, rng, k):
    """rows of overlapping discs at one f (identical quantised depth keys) in
    ascending and descending slot order, agents at bit-identical places, a
    square and a disc at one quantised depth, five packages on one lattice
    point -- the discs in the world's last slots"""
    h, nc = head_of(k), num_cams(n)
    off = int(rng.integers(0, 64))
    cams, discs, food = [], [], []
    for i, (ax, ay) in enumerate(anchors(rng, nc)):
        f0 = (3.0, 6.0, 9.0)[(i + off) % 3] * (1.0 if (i + off) % 2 else -1.0)
        P = lattice_near(ax + f0 * float(h[0]), ay + f0 * float(h[1]))
        a = (F(ax), F(ay))
        cams.append((a[0], a[1], k))
        rots = [pick_rot(rng, j) for j in range(5)] if i == 0 else [pick_rot(rng, i + off)]
        food += [(P[0], P[1], r) for r in rots]
        # the square's depth key for this camera, and a disc row with the same one
        fp, lp = fl(a[0], a[1], h[0], h[1], F(P[0]), F(P[1]))
        w = rots[0] * (np.pi / 2) / 4194304.0
        ext = abs(np.cos(w) * float(h[0]) + np.sin(w) * float(h[1])) + \
            abs(np.cos(w) * float(h[1]) - np.sin(w) * float(h[0]))
        zsq = float(zq(F(max(abs(float(fp)) - ext, 0.0))))
        fd = np.sign(f0) * (zsq + float(R_AGENT) + 1e-4)
        row = []
        for lt in np.arange(-2.0, 2.01, 0.5):
            q = q_disc_z if f0 > 0 else (lambda f, l: q_disc_z(-f, l))
            p = solve(a, h, fd, float(lp) + lt, q, zsq, "eq") or solve(a, h, fd, float(lp) + lt)
            if p is not None:
                row.append(p)
        row = row[::-1] if i % 2 else row
        discs += row + row[:1] * 2          # two more agents exactly on the row's first
    return assemble(n, rng, cams, discs, food, discs_last=True)


# ---- family 5: queue pressure ---------------------------------------------------------
def fam_queue(n, rng, k):
    """the eight cameras within radius 1; every other agent within 1.5 of them
    (all wide pairs), within 1.5 - 5 (all far pairs) or half and half; 30
    packages inside the wedge, five per chunk around a chunk corner"""
    h, nc = head_of(k), num_cams(n)
    mode = HEADINGS.index(k) % 3   # wide, far, half and half, wide: all three in every set of four headings
    cx, cy = 32.0 * int(rng.integers(1, 4)), 48.0 + rng.uniform(-0.4, 0.4)
    cx += rng.uniform(-0.4, 0.4)
    cams = []
    for i in range(nc):
        r, t = rng.uniform(0, 1.0), rng.uniform(0, 2 * np.pi)
        cams.append((F(cx + r * np.cos(t)), F(cy + r * np.sin(t)), k))
    discs = []
    for j in range(n - nc):
        near = mode == 0 or (mode == 2 and j % 2 == 0)
        r = rng.uniform(0, 1.5) if near else rng.uniform(2.6, 5.0)
        t = rng.uniform(0, 2 * np.pi)
        discs.append((F(cx + r * np.cos(t)), F(cy + r * np.sin(t))))
    cand = []
    for X in range(int(cx) - 30, int(cx) + 31):    # (30 packages need six chunks' worth of cells)
        for Y in range(int(cy) - 30, int(cy) + 31):
            f = (X - cx) * float(h[0]) + (Y - cy) * float(h[1])
            l = (X - cx) * float(h[1]) - (Y - cy) * float(h[0])
            if abs(l) <= abs(f) + 1.0 and abs(f) >= 2.0 and 0 <= X <= 127 and 0 <= Y <= 95:
                cand.append((abs(f) + abs(l) + rng.uniform(0, 3), X, Y))
    food = [(X, Y, pick_rot(rng, j)) for j, (_, X, Y) in enumerate(sorted(cand))]
    return assemble(n, rng, cams, discs, food)


# ---- family 6: long sight lines ----------------------------------------------------------
def fam_long(n, rng, k):
    """cameras in the corner the heading leaves, targets 60, 100 and 125 units
    out on pixel centres and between them, and targets whose z d on a ray's
    dominant axis is just below / at / above the inner wall's face (beats_wall)"""
    h, nc = head_of(k), num_cams(n)
    off = int(rng.integers(0, 64))
    cams, discs, food = [], [], []
    for i in range(nc):
        ax, ay = _far_corner((float(h[0]), float(h[1])), rng, 10.0)
        if abs(h[1]) < 0.5:
            ax, ay = (1.0 + rng.uniform(0, 0.5) if h[0] > 0 else 126.0 - rng.uniform(0, 0.5)), 8.0 + 10.0 * i
        a = (F(ax), F(ay))
        cams.append((a[0], a[1], k))
        for rng_t in (60.0, 100.0, 125.0):
            for pix in (2 + (i + off) % 20, 11, 12):
                for u in (float(ray_u(pix)), 0.5 * (float(ray_u(pix)) + float(ray_u(pix + 1)))):
                    p = solve(a, h, rng_t, u * rng_t)
                    if p is not None:
                        discs.append(p)
                        X, Y = lattice_near(float(p[0]) - 3 * float(h[0]), float(p[1]) - 3 * float(h[1]))
                        if i == 0:
                            food.append((X, Y, pick_rot(rng, len(food))))
        # beats_wall: ray `pix` leaves the inner rectangle through the face its
        # dominant axis points at; a disc whose z d equals that face's offset
        pix = (0, 23, 5, 18)[(i + off) % 4]
        u = ray_u(pix)
        dx = F(h[0] + F(u * h[1]))
        dy = F(h[1] + F(u * F(-h[0])))
        tx = (float(IN_HI_X) - float(a[0])) / float(dx) if dx > 0 else (float(IN_LO) - float(a[0])) / float(dx) if dx < 0 else np.inf
        ty = (float(IN_HI_Y) - float(a[1])) / float(dy) if dy > 0 else (float(IN_LO) - float(a[1])) / float(dy) if dy < 0 else np.inf
        if tx <= ty:
            d, T = dx, (F(IN_HI_X - a[0]) if dx > 0 else F(IN_LO - a[0]))
        else:
            d, T = dy, (F(IN_HI_Y - a[1]) if dy > 0 else F(IN_LO - a[1]))
        zt = min(tx, ty)
        # (z d < T for d > 0, z d > T for d < 0: both are |z d| < |T|)
        q = lambda f, l, d=d: np.abs(np.multiply(q_disc_z(f, l), d, dtype=F))
        ft = zt + float(R_AGENT)
        for p in three_sides(a, h, ft, float(u) * ft, q, abs(float(T))) \
                if solve(a, h, ft, float(u) * ft) is not None else []:
            discs.append(p)
    return assemble(n, rng, cams, discs, food)


# ---- family 7: corners and walls with company ---------------------------------------------
def fam_walls(n, rng, k):
    """cameras at the four corners and mid-edges, 0 / 1 / 2 units off the wall
    (near points beyond the wall, inside its box, in the inner rectangle),
    looking into and along it, each with a disc and a package on the finder
    ray at f = 0.18, 1.1 or 2"""
    nc = num_cams(n)
    off = int(rng.integers(0, 64))
    spots = [(0, 0), (64, 0), (127, 0), (127, 48), (127, 95), (64, 95), (0, 95), (0, 48)]
    cams, discs, food = [], [], []
    for i in range(nc):
        sx, sy = spots[(i + off) % 8]
        d = (0.0, 1.0, 2.0)[(i + off // 8) % 3] + rng.uniform(0, 0.05)
        ax = sx + d if sx == 0 else sx - d if sx == 127 else sx + rng.uniform(-1, 1)
        ay = sy + d if sy == 0 else sy - d if sy == 95 else sy + rng.uniform(-1, 1)
        kk = (k + 31 * (i + off)) % 126            # 3.1 rad apart: into, along, away
        h = head_of(kk)
        a = (F(ax), F(ay))
        cams.append((a[0], a[1], kk))
        fo = (0.18, 1.1, 2.0)[(i + off) % 3]
        p = solve(a, h, fo, 0.0)
        if p is not None:
            discs.append(p)
        fq = (0.18, 1.1, 2.0)[(i + off + 1) % 3]
        X, Y = lattice_near(ax + fq * float(h[0]), ay + fq * float(h[1]))
        food.append((X, Y, pick_rot(rng, i + off)))
    return assemble(n, rng, cams, discs, food)


# ---- family 8: the K1 finder pass's own cull -------------------------------------------------
def fam_finder(n, rng, k):
    """discs at |l| around 0.92 and 1.45 with f around 0.18 and -0.35, squares
    at |l| around sqrt 2 and f + ext around 1.1: what the finder ray just
    reaches and what K1's cull (|l| <= 1.45, f >= -0.35) just drops"""
    h, nc = head_of(k), num_cams(n)
    off = int(rng.integers(0, 64))
    cams, discs, food = [], [], []
    for i, (ax, ay) in enumerate(anchors(rng, nc)):
        # the camera stands where its package has |l| at sqrt 2 (a 45-degree
        # square's corner on the finder ray) or f + ext at 1.1
        rot = (1 << 21, 0, pick_rot(rng, 3))[(i + off) % 3]
        P = lattice_near(ax, ay)
        if (i + off) % 2:
            side = three_sides(P, h, 2.0, 1.41421356, q_absl, F(1.41421356), move="cam")
        else:
            w = rot * (np.pi / 2) / 4194304.0
            ext = abs(np.cos(w) * float(h[0]) + np.sin(w) * float(h[1])) + \
                abs(np.cos(w) * float(h[1]) - np.sin(w) * float(h[0]))
            side = three_sides(P, h, 1.1 - ext, 0.3, q_f, F(1.1 - ext), move="cam")
        a = side[(i + off // 2) % len(side)]
        cams.append((a[0], a[1], k))
        food.append((P[0], P[1], rot))
        for T in (R_AGENT, FINDER_L):
            for ft in (0.18, 2.0, -0.3):
                for s in (1.0, -1.0):
                    discs += three_sides(a, h, ft, s * float(T), q_absl, T)[:3 if (i + off) % 2 else 2]
        for lt in (0.0, 0.9, -1.44):
            discs += three_sides(a, h, float(FINDER_F), lt, q_f, FINDER_F)
        discs += three_sides(a, h, float(TOUCH), 0.0, q_f, TOUCH)
    return assemble(n, rng, cams, discs, food)


FAMILIES = [
    ("thresholds", fam_thresholds), ("tangency", fam_tangency), ("wedge", fam_wedge),
    ("ties", fam_ties), ("queue", fam_queue), ("long", fam_long), ("walls", fam_walls),
    ("finder", fam_finder),
]
# families whose objects sit on decision boundaries by construction: compared
# bitwise only, never with the float64 renderer
BOUNDARY_FAMILIES = ("tangency", "ties")

# the catalogue: every family at every heading; scene(n, rng) -> (pos, rot, food)
SCENES = [(f"{name}-k{k}", name, (lambda n, rng, fn=fn, k=k: fn(n, rng, k)))
          for name, fn in FAMILIES for k in HEADINGS]


def check_scene(n, pos, rot, food):
    """what both setters demand of a scene"""
    assert pos.shape == (n, 2) and rot.shape == (n, 2) and pos.dtype == F and rot.dtype == F
    assert np.isfinite(pos).all() and np.isfinite(rot).all()
    assert (pos >= 0).all() and (pos[:, 0] <= LX).all() and (pos[:, 1] <= LY).all()
    nn = rot.astype(np.float64)
    assert (np.abs(nn[:, 0] ** 2 + nn[:, 1] ** 2 - 1.0) <= 1e-3).all()
    assert len(food) <= 30
    if len(food):
        assert (np.bincount(food[:, 0], minlength=48) <= 5).all()
        assert ((food[:, 1] // 16) + (food[:, 2] // 16) * 8 == food[:, 0]).all()
        assert (food[:, 3] >= 0).all() and (food[:, 3] < (1 << 22)).all()
