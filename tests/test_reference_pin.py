"""CPU, live: the oracle in lock-step with the reference's own simulation code.

oracle/_ref/libmbots_ref.so is the reference's sim.cpp compiled against the
stand-in engine of oracle/refbuild/ (`make -C oracle ref`; build() makes it
where the reference's source lies on the machine).  Where it is absent these
tests are skipped; tests/test_golden.py then holds the oracle, the CPU mode and
the device to what that library recorded (tests/golden/reference_*.npz).

What this pins to the reference's compiled code, and what stays the build's own
spec, is tabled in DESIGN.md section 7.  tests/ref_lockstep.py says what is
compared after every step and shift.
"""
import numpy as np
import pytest

import pyoracle as po
import pyref
from ref_lockstep import LockStep, breed_heavy, shoot_heavy

pytestmark = pytest.mark.skipif(
    not pyref.available(),
    reason="oracle/_ref/libmbots_ref.so is not built: the reference's source is not on this machine "
           "(tests/test_golden.py checks its recorded output instead)")

F = np.float32


@pytest.mark.parametrize("W,A,steps", [(8, 32, 24), (5, 4, 40), (5, 6, 40), (5, 9, 40)])
def test_seeded_stream(W, A, steps):
    """Identity-keyed one-hot actions and hidden values.  A = 6 and 9: the
    initNumAgentsPerWorld / kNumSpecies integer division of the respawn loop
    (1 and 2 per species) and i % 4 species of initWorld."""
    ls = LockStep(W, 69, A)
    for _ in range(steps):
        ls.synthetic(1234, True)
        ls.step()
        ls.shift()
    if A == 32:
        assert ls.births and ls.deaths and ls.respawns and ls.enemy


def test_breed_heavy_past_128():
    """Births (parent -40, child 50, `health > 10` after the food bonus) until a
    world holds more than 128 agents."""
    ls = LockStep(4, 69, 32, cap=1024)
    while ls.peak_world <= 128:
        assert ls.t < 80, "the stream should have passed 128 agents by now"
        ls.write_actions(breed_heavy(ls.orc.num_agents(), ls.t))
        ls.step()
        ls.shift()
    assert ls.births >= 97      # 32 -> more than 128 in one world


def test_shoot_heavy():
    """-50 accumulation, friendly and enemy stats, deaths, respawns up to A / 4
    per species in species order."""
    ls = LockStep(4, 69, 32)
    for _ in range(60):
        ls.write_actions(shoot_heavy(ls.orc.num_agents(), ls.t))
        ls.step()
        ls.shift()
    assert ls.deaths >= 1 and ls.respawns >= 1 and ls.friendly >= 1 and ls.enemy >= 1


def test_food_to_its_cap():
    """All-zero actions: only addFoodSystem acts -- its two discarded draws, the
    rotation draw, min(rand_sample, diff_allowed) at the cap of 30 and one unit
    per package."""
    ls = LockStep(2, 69, 32)
    at_cap = 0
    for _ in range(400):
        ls.write_actions(np.zeros((ls.orc.num_agents(), 6), np.int32))
        ls.step()
        ls.shift()
        at_cap += all(len(ls.orc.world_state(w)["food"]) == 30 for w in range(2))
    assert ls.peak_food == 30 and at_cap > 20, (ls.peak_food, at_cap)


# (action, steps): backward, forward to +x, then left turns of 1.5, 1.6, 1.6 and
# 1.5 rad, each followed by a walk along a wall into the next corner
WALL_PHASES = [(1, 10), (0, 130), (2, 15), (0, 100), (2, 16), (0, 130), (2, 16), (0, 100), (2, 15), (0, 130)]
# test_agents_driven_into_the_walls' stream (tests/test_parity_gpu.py): forward
# to the +x wall, turn about (31 x 0.1 rad), forward to the -x wall
DRIVEN_PHASES = [(0, 100), (2, 31), (0, 129)]


@pytest.mark.parametrize("phases,want", [
    (WALL_PHASES, {"x0", "x1", "y0", "y1", "x1y1", "x0y1", "x0y0", "x1y0"}),
    (DRIVEN_PHASES, {"x0", "x1"})], ids=["four-corners", "driven"])
def test_walls_and_corners(phases, want):
    """Backward into the -x wall, forward into +x, then along the walls through
    all four corners; and the stream of test_agents_driven_into_the_walls:
    min(limit - 1, max(0, x)) in x and y and (uint32_t)(len * 2.f) of clipped
    moves."""
    ls = LockStep(2, 69, 32)
    seen = set()
    for k, steps in phases:
        for _ in range(steps):
            a = np.zeros((ls.orc.num_agents(), 6), np.int32)
            a[:, k] = 1
            ls.write_actions(a)
            ls.step()
            ls.shift()
            p = ls.orc.column(po.COL_POS)
            x0, x1, y0, y1 = p[:, 0] == 0, p[:, 0] == 127, p[:, 1] == 0, p[:, 1] == 95
            for nm, m in (("x0", x0), ("x1", x1), ("y0", y0), ("y1", y1), ("x1y1", x1 & y1),
                          ("x0y1", x0 & y1), ("x0y0", x0 & y0), ("x1y0", x1 & y0)):
                if m.any():
                    seen.add(nm)
    assert seen >= want, (seen, want)


# -- placed scenes -------------------------------------------------------------
def _around(v):
    v = F(v)
    return [np.nextafter(v, F(-1e9)), v, np.nextafter(v, F(1e9))]


def _rot(k):
    return [F(np.cos(0.05 * k)), F(np.sin(0.05 * k))]


def border_values():
    """On and one ulp either side of every chunk border and chunk centroid, and
    the ends 0, 127 / 95: (xs, ys)."""
    xs = [F(0), F(127)] + [v for b in range(8, 128, 8) for v in _around(b)]
    ys = [F(0), F(95)] + [v for b in range(8, 96, 8) for v in _around(b)]
    return xs, ys


def border_scenes(n=32):
    """Scenes that between them place every value of border_values() in x and
    in y (consecutive runs of each list, so 4 x 32 agents go round the 47 x
    values and the 35 y values more than twice, in changing pairs)."""
    xs, ys = border_values()
    out = []
    for j in range(4):
        pos = np.array([[xs[(i + n * j) % len(xs)], ys[(i + n * j) % len(ys)]] for i in range(n)], F)
        rot = np.array([_rot(7 * i + 3 * j) for i in range(n)], F)
        out.append((pos, rot, np.zeros((0, 4), np.int32)))
    return out


def stacked_scene(n=32):
    """2, 3 and 6 agents on a food cell holding 1 and 2 packages (the order
    FoodPackage::consume is reached in), and agents on the cell of another chunk
    with the same in-chunk (x, y) as a package."""
    food = [(9, 20, 20, 5), (10, 40, 20, 1 << 21), (10, 40, 20, 77), (19, 60, 40, 0), (19, 60, 40, 9),
            (29, 84, 52, (1 << 22) - 1), (29, 86, 52, 3)]
    pos = []
    pos += [(20.25, 20.5), (20.75, 20.125)]                          # 2 agents, 1 package
    pos += [(40.5, 20.5), (40.0, 20.0), (40.99, 20.99)]              # 3 agents, 2 packages
    pos += [(60.0 + 0.15 * i, 40.5) for i in range(6)]               # 6 agents, 2 packages
    pos += [(84.5, 52.0 + 0.15 * i) for i in range(6)]               # 6 agents, 1 package
    pos += [(36.5, 20.5), (36.25, 20.75), (20.5, 36.5), (100.5, 52.5)]   # chunk 10 / 17 / 30: no package there
    while len(pos) < n:
        pos.append((60.0 + len(pos), 90.0))
    rot = np.array([_rot(3 * i) for i in range(n)], F)
    return np.array(pos, F), rot, np.array(food, np.int32)


@pytest.mark.parametrize("which", ["borders", "stacked"])
def test_placed_scenes(which):
    ls = LockStep(2, 69, 32)
    scenes = border_scenes() if which == "borders" else [stacked_scene()]
    if which == "borders":     # every listed x and y value is placed
        xs, ys = border_values()
        assert len(xs) == 47 and len(ys) == 35
        assert {float(v) for v in xs} == {float(v) for p, _, _ in scenes for v in p[:, 0]}
        assert {float(v) for v in ys} == {float(v) for p, _, _ in scenes for v in p[:, 1]}
        for v in (64.0, 24.0, 16.0, 8.0):
            assert any((p[:, 1] == F(v)).any() for p, _, _ in scenes)
    for pos, rot, food in scenes:
        for w in range(2):
            ls.set_world_state(w, pos, rot, food)
        ate0 = ls.ate
        for k in (None, 0, 1):     # nothing, forward, backward
            a = np.zeros((ls.orc.num_agents(), 6), np.int32)
            if k is not None:
                a[:, k] = 1
            ls.write_actions(a)
            ls.step()
            ls.shift()
        if which == "stacked":
            # per world: 1 + 2 + 2 + 1 packages under stacks of agents
            assert ls.ate - ate0 >= 2 * 6, ls.ate - ate0


def test_breed_at_health_10_on_food():
    """healthSync tests `health > 10` after the food bonus (sim.cpp:536, :547):
    an agent shot and bred down to exactly 10 that stands on food and breeds
    again eats first (30), so it does breed -- and dies of it at -10, its child
    born.  Slots 0, 4 and 8 are of one species; 8 looks at 0, 0 at 4."""
    ls = LockStep(1, 69, 32)
    pos = np.array([(8.5 + 3 * i, 90.5) for i in range(32)], F)
    pos[0], pos[4], pos[8] = (20.5, 20.5), (24.5, 20.5), (16.5, 20.5)
    rot = np.tile(np.array([1, 0], F), (32, 1))
    none = np.zeros((0, 4), np.int32)

    def act(**slots):
        a = np.zeros((ls.orc.num_agents(), 6), np.int32)
        rows = ls.orc.sensor_index()
        for slot, k in slots.items():
            a[rows[int(slot[1:])], k] = 1
        ls.write_actions(a)
        ls.step()
        ls.shift()

    ls.set_world_state(0, pos, rot, none)
    act()                                   # the sensor finds who looks at whom
    st = ls.orc.world_state(0)
    assert st["finder"][0] == 4 and st["finder"][8] == 0
    act(s0=5, s8=4)                         # 100 - 50 (shot) - 40 (breed) = 10
    st = ls.orc.world_state(0)
    assert st["health"][0] == 10 and len(st["health"]) == 33 and st["finder"][0] == 4
    ls.set_world_state(0, st["xy"], st["rot"], np.array([(9, 20, 20, 0)], np.int32))
    act(s0=5)                               # 10 + 20 > 10: breeds, -10, dies
    st = ls.orc.world_state(0)
    # the parent's slot is gone (slot 1 moved up), its second child is there, the food is eaten
    assert len(st["health"]) == 33 and st["xy"][0].tolist() == [11.5, 90.5] and len(st["food"]) == 0
    assert st["species"][-2:].tolist() == [1, 1] and st["health"][-2:].tolist() == [50, 50]
    assert st["xy"][-2:].tolist() == [[20.5, 20.5], [20.5, 20.5]]


# -- random call sequences ------------------------------------------------------
def random_scene(rng, n):
    pos = np.stack([rng.uniform(0, 127, n), rng.uniform(0, 95, n)], 1).astype(F)
    if rng.random() < 0.5:    # on cells, so that food is eaten
        pos = np.floor(pos) + F(0.5)
    rot = np.array([_rot(int(k)) for k in rng.integers(0, 126, n)], F)
    nf = int(rng.integers(0, 31))
    food, used = [], {}
    for _ in range(nf):
        if rng.random() < 0.5:
            i = int(rng.integers(0, n))
            x, y = int(pos[i, 0]), int(pos[i, 1])
        else:
            x, y = int(rng.integers(0, 128)), int(rng.integers(0, 96))
        c = x // 16 + 8 * (y // 16)
        if used.get(c, 0) < 5:
            used[c] = used.get(c, 0) + 1
            food.append((c, x, y, int(rng.integers(0, 1 << 22))))
    return pos, rot, np.array(food, np.int32).reshape(-1, 4)


@pytest.mark.parametrize("seed", range(8))
def test_random_call_sequences(seed):
    """48 operations a seed: steps, shifts or none, action and hidden writes
    between step and shift, placed scenes (no resets: the reference's
    resetSystem is empty)."""
    rng = np.random.default_rng(9000 + seed)
    W, A = int(rng.integers(1, 5)), int(rng.choice([4, 7, 12, 32]))
    ls = LockStep(W, 100 + seed, A)

    def write():
        n = ls.orc.num_agents()
        mode = rng.integers(0, 4)
        if mode == 0:
            a = (rng.random((n, 6)) < 0.4).astype(np.int32)        # several at once
        elif mode == 1:
            a = shoot_heavy(n, int(rng.integers(0, 1000)))
        elif mode == 2:
            a = breed_heavy(n, int(rng.integers(0, 1000)))
        else:
            a = np.eye(6, dtype=np.int32)[rng.integers(0, 6, n)]
        ls.write_actions(a, rng.standard_normal((n, po.HIDDEN)).astype(F) if rng.random() < 0.5 else None)

    for _ in range(48):
        op = rng.random()
        if op < 0.45:
            write()
            ls.step()
            if rng.random() < 0.3:
                write()          # a learner writing between step and shift
                ls.compare("write after step")
            if rng.random() < 0.7:
                ls.shift()
        elif op < 0.6:
            ls.shift()
        elif op < 0.75:
            write()
            ls.compare("write")
        else:
            w = int(rng.integers(0, W))
            ls.set_world_state(w, *random_scene(rng, int(ls.orc.world_counts()[0][w])))
            ls.compare("scene")
    assert ls.t > 10
