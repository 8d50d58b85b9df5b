"""A numpy float32 restatement of the rasteriser's image (include/mbots.h
"Rasteriser", DESIGN.md "Rasteriser"), written from that text: it takes what
SimManager.world_state() reports and a scale and returns the class map, the
slot map and the RGB image that render_worlds must give, bit for bit.

Every product and sum is one float32 rounding in the order the spec writes it
(numpy float32 arrays round each operation once).  Objects are evaluated over a
window of pixels around them that is far wider than they can reach (2 cells
for a disc of radius 0.92 and for a square of half diagonal 1.42); outside it
the predicates cannot hold."""
import numpy as np

F = np.float32
AGENT_R2 = F(0.8464)
MARK_FWD, MARK_HALF = F(0.3), F(0.25)
QUARTER_TURN_UNIT = F(1.57079632679489662 / 4194304.0)
WALL = F(0.2)
LX, LY = F(128.0), F(96.0)
REACH = 2.0          # cells: the window evaluated around an object
FLOOR, WALL_CLS, FOOD, BODY, MARK = 0, 1, 2, 4, 8


def palette():
    import madrona_bots as mb
    return np.asarray(mb.RENDER_PALETTE)


def heading(w, z):
    """rot.rotateVec({1, 0, 0}).normalize() of the z-only quaternion (w, z)."""
    w, z = F(w), F(z)
    vx = F(1.0) - F(2.0) * (z * z)
    vy = F(2.0) * (z * w)
    ln = np.sqrt(vx * vx + vy * vy)
    return vx / ln, vy / ln


def food_cs(q22):
    """cos / sin of a 22-bit quarter-turn fraction: the fixed Taylor
    polynomials of the sensor's food boxes."""
    one = F(1.0)
    w = F(int(q22)) * QUARTER_TURN_UNIT
    w2 = w * w
    s = one - w2 * (one / F(110.0))
    for d in (72.0, 42.0, 20.0, 6.0):
        s = one - w2 * (one / F(d)) * s
    s = w * s
    c = one - w2 * (one / F(132.0))
    for d in (90.0, 56.0, 30.0, 12.0):
        c = one - w2 * (one / F(d)) * c
    c = one - w2 * F(0.5) * c
    return c, s


def samples(n, scale):
    return (np.arange(n, dtype=F) + F(0.5)) * (F(1.0) / F(scale))


def _window(centre, n, scale):
    lo = max(0, int(np.floor((float(centre) - REACH) * scale)))
    hi = min(n, int(np.ceil((float(centre) + REACH) * scale)) + 1)
    return lo, max(lo, hi)


def in_wall_box(x, y):
    xs = (x >= F(0.0)) & (x <= LX)
    ys = (y >= F(0.0)) & (y <= LY)
    bx = ((x >= F(0.0) - WALL) & (x <= F(0.0) + WALL)) | ((x >= LX - WALL) & (x <= LX + WALL))
    by = ((y >= F(0.0) - WALL) & (y <= F(0.0) + WALL)) | ((y >= LY - WALL) & (y <= LY + WALL))
    return (bx & ys) | (by & xs)


def shade(health):
    return 64 + (191 * min(max(int(health), 0), 100)) // 100


def render_ref(state, scale, pal=None):
    """(cls uint8 [H, W], slot int16 [H, W], rgb uint8 [H, W, 3]) of one world."""
    assert scale in (1, 2, 4, 8)
    pal = palette() if pal is None else pal
    H, W = 96 * scale, 128 * scale
    px, py = samples(W, scale), samples(H, scale)
    # rules 4 and 3: floor, wall
    cls = np.where(in_wall_box(px[None, :], py[:, None]), WALL_CLS, FLOOR).astype(np.uint8)
    # rule 2: food, any package
    for _, X, Y, rot in np.asarray(state["food"]).reshape(-1, 4):
        c, s = food_cs(rot)
        i0, i1 = _window(X, W, scale)
        j0, j1 = _window(Y, H, scale)
        dx = (px[i0:i1] - F(X))[None, :]
        dy = (py[j0:j1] - F(Y))[:, None]
        hit = (np.abs(dx * c + dy * s) <= F(1.0)) & (np.abs(dy * c - dx * s) <= F(1.0))
        cls[j0:j1, i0:i1][hit] = FOOD
    # rule 1: agents, the lowest slot wins -- painted from the highest slot down
    slot = np.full((H, W), -1, np.int16)
    k_of = np.zeros((H, W), np.int32)
    pos, rot = np.asarray(state["position"], F), np.asarray(state["rotation_wz"], F)
    for a in range(len(pos) - 1, -1, -1):
        x, y = pos[a]
        hx, hy = heading(rot[a, 0], rot[a, 1])
        i0, i1 = _window(x, W, scale)
        j0, j1 = _window(y, H, scale)
        dx = (px[i0:i1] - x)[None, :]
        dy = (py[j0:j1] - y)[:, None]
        disc = dx * dx + dy * dy <= AGENT_R2
        fa = dx * hx + dy * hy
        la = dy * hx - dx * hy
        mark = (fa >= MARK_FWD) & (np.abs(la) <= MARK_HALF)
        sp1 = int(state["species"][a]) - 1
        code = np.where(mark, MARK + sp1, BODY + sp1).astype(np.uint8)
        cls[j0:j1, i0:i1][disc] = code[disc]
        slot[j0:j1, i0:i1][disc] = a
        k_of[j0:j1, i0:i1][disc] = shade(state["health"][a])
    rgb = pal[cls].astype(np.int32)
    body = (cls >= BODY) & (cls < MARK)
    rgb[body] = (rgb[body] * k_of[body][:, None]) // 255
    return cls, slot, rgb.astype(np.uint8)


def render_all(mgr, worlds, scale):
    """render_ref of each of `worlds`, stacked like render_worlds' outputs."""
    outs = [render_ref(mgr.world_state(w), scale) for w in worlds]
    return {"cls": np.stack([o[0] for o in outs]), "slot": np.stack([o[1] for o in outs]),
            "rgb": np.stack([o[2] for o in outs])}
