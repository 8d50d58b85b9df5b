"""Scenes and helpers shared by tests/test_render_cpu.py and
tests/test_render_gpu.py: the directed seam scenes (every integer row and
column boundary of the arena straddled by a disc and by a food square, so no
band or tile seam of the rasteriser lies on empty floor), one world of special
cases, and the comparisons against tests/render_ref.py."""
import math

import numpy as np

import madrona_bots as mb
import render_ref as rr

SCALES = (1, 2, 4, 8)
KEYS = ("cls", "slot", "rgb")
# render_kernel examines this many agent slots per pass (kRenderStage,
# csrc/mbots_kernels.hip): a world of more agents takes further passes
STAGE = 256
BIG_POP = 300
assert BIG_POP > STAGE


def make(mode, worlds, seed, agents, **kw):
    return mb.SimManager(0, worlds, seed, agents, exec_mode=mode, **kw)


def rendered(mgr, worlds, scale):
    """All three outputs of render_worlds as numpy arrays."""
    out = mgr.render_worlds(worlds, scale, rgb=True, cls=True, slot=True)
    return {k: out[k].cpu().numpy() for k in KEYS}


def assert_same(a, b, where):
    for k in KEYS:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (where, k, a[k].shape, b[k].shape)
        bad = np.argwhere(a[k] != b[k])
        assert len(bad) == 0, f"{where}: {k} differs at {len(bad)} entries, first {bad[0].tolist()}"


def assert_equals_ref(mgr, worlds, scale, where):
    got = rendered(mgr, worlds, scale)
    assert_same(got, rr.render_all(mgr, worlds, scale), f"{where} scale {scale}")
    return got


def rot_of(theta):
    """(w, z) of a rotation by theta about z."""
    return (math.cos(theta / 2), math.sin(theta / 2))


def chunk_of(x, y):
    return (x // 16) + (y // 16) * 8


# ---------------------------------------------------------------------------
# Seam scenes: a 4-world manager of 96 agents per world.  Worlds 0 and 1 carry
# the discs (a diagonal and an anti-diagonal), worlds 2 and 3 the 45-degree food
# squares (half diagonal 1.41: a square at X strictly contains X - 1, X, X + 1).
# ---------------------------------------------------------------------------
SEAM_AGENTS = 96
DISC_R = 0.92


def seam_discs():
    k = np.arange(SEAM_AGENTS)
    w0 = np.stack([1.3 * k + 2.0, k.astype(float)], axis=1)
    w1 = np.stack([1.32 * k + 1.0, 95.0 - k], axis=1)
    return w0.astype(np.float32), w1.astype(np.float32)


def seam_food():
    """Two lists of (chunk, x, y, rotation): squares at X = 3 m + 1 along an
    anti-diagonal in y, alternating between the two worlds (at most 3 per
    chunk, 22 per world)."""
    out = ([], [])
    for m in range(43):
        x = 3 * m + 1
        y = 94 - 3 * (m % 32)
        out[m % 2].append((chunk_of(x, y), x, y, 1 << 21))
    return out


def straddled(centres, reach, n):
    """The integer boundaries 1 .. n-1 lying strictly inside [c - reach, c + reach] of some centre."""
    b = np.arange(1, n)[:, None]
    return set((np.arange(1, n)[(np.abs(np.asarray(centres, float)[None, :] - b) < reach).any(axis=1)]).tolist())


def seam_manager(mode):
    mgr = make(mode, 4, 11, SEAM_AGENTS)
    w0, w1 = seam_discs()
    f2, f3 = seam_food()
    # the test's own coverage: every row boundary 1..95 and column boundary
    # 1..127 inside a disc of worlds 0 / 1 and inside a square of worlds 2 / 3
    xs, ys = np.concatenate([w0[:, 0], w1[:, 0]]), np.concatenate([w0[:, 1], w1[:, 1]])
    assert straddled(xs, DISC_R, 128) == set(range(1, 128)) and straddled(ys, DISC_R, 96) == set(range(1, 96))
    fx, fy = [f[1] for f in f2 + f3], [f[2] for f in f2 + f3]
    assert straddled(fx, 1.41, 128) == set(range(1, 128)) and straddled(fy, 1.41, 96) == set(range(1, 96))
    rots = np.array([rot_of(0.37 * i) for i in range(SEAM_AGENTS)], np.float32)
    mgr.set_world_state(0, w0, rots, np.zeros((0, 4), np.int32))
    mgr.set_world_state(1, w1, rots, np.zeros((0, 4), np.int32))
    for w, food in ((2, f2), (3, f3)):
        st = mgr.world_state(w)
        # (the initial positions, clamped as the first step would clamp them)
        pos = np.clip(st["position"], [0.0, 0.0], [127.0, 95.0]).astype(np.float32)
        mgr.set_world_state(w, pos, st["rotation_wz"], np.array(food, np.int32))
    return mgr


# ---------------------------------------------------------------------------
# Special cases, one world of 8 agents: two agents of different species on one
# spot, agents at the arena's corners (bounding boxes leave the image), an agent
# over a food square, a food square over the wall band, food at rotation 0, at
# 2^21 (45 degrees) and at an odd value, headings along +-x, +-y and a diagonal.
# ---------------------------------------------------------------------------
SPOT = (10.3, 10.6)
ODD_ROT = 1234567


def special_manager(mode):
    mgr = make(mode, 2, 23, 8)
    sp = mgr.world_state(0)["species"]
    lo = 0
    hi = next(i for i in range(1, 8) if sp[i] != sp[lo])      # another species than slot 0's
    rest = [i for i in range(1, 8) if i != hi]
    pos = np.zeros((8, 2), np.float32)
    rot = np.zeros((8, 2), np.float32)
    pos[lo], rot[lo] = SPOT, rot_of(0.0)
    pos[hi], rot[hi] = SPOT, rot_of(math.pi / 2)
    places = [((0.0, 0.0), 0.0), ((127.0, 95.0), math.pi), ((40.0, 40.0), math.pi / 2),
              ((70.5, 20.25), -math.pi / 2), ((90.0, 70.0), math.pi / 4), ((20.0, 80.0), 2.5)]
    for i, (p, th) in zip(rest, places):
        pos[i], rot[i] = p, rot_of(th)
    food = [(chunk_of(40, 40), 40, 40, 0),            # under an agent
            (chunk_of(0, 50), 0, 50, 1 << 21),        # over the left wall band
            (chunk_of(60, 0), 60, 0, ODD_ROT),        # over the bottom wall band
            (chunk_of(100, 60), 100, 60, ODD_ROT),
            (chunk_of(101, 61), 101, 61, 0)]          # overlapping squares
    mgr.set_world_state(0, pos, rot, np.array(food, np.int32))
    return mgr, lo, hi


def stepped_manager(mode, worlds=8, seed=69, agents=32, steps=30, **kw):
    mgr = make(mode, worlds, seed, agents, **kw)
    for t in range(steps):
        mgr.write_synthetic_actions(1234, t, True)
        mgr.step()
    return mgr


def big_manager(mode):
    """Two worlds of BIG_POP agents in 512 slots: more than one pass of STAGE slots."""
    return make(mode, 2, 5, BIG_POP, agent_capacity=512)
