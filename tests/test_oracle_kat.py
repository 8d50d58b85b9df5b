"""CPU: known-answer tests of the oracle (oracle/mbots_oracle.c), hand-derived
from the cited reference formulas, plus independent numpy restatements of the
small systems.  No GPU needed."""
import numpy as np
import pytest

import pyoracle as po


def f32(x):
    return np.float32(x)


# ---------------------------------------------------------------------------
# RNG: Threefry-2x32-20 known-answer vectors published with Random123
# (kat_vectors: "threefry2x32 20 <ctr0> <ctr1> <key0> <key1> <out0> <out1>")
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,out", [
    ((0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6b200159, 0x99ba4efe)),
    ((0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x1cb996fc, 0xbb002be7)),
    ((0x243f6a88, 0x85a308d3), (0x13198a2e, 0x03707344), (0xc4923a9c, 0x483df7a0)),
])
def test_threefry_kat(ctr, key, out):
    assert po.threefry2x32(key, ctr) == out


def test_samplers():
    L = po.lib()
    assert L.orc_sample_uniform(0) == 0.0
    assert L.orc_sample_uniform(0xFFFFFFFF) == f32(16777215 / 16777216)
    for bits in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 12345678):
        v = L.orc_sample_i32(bits, 0, 10)
        assert 0 <= v < 10 and v == (bits * 10) >> 32
        assert 1 <= L.orc_sample_i32(bits, 1, 3) < 3


def _rows_by_species(sim):
    """A=4, one agent per species, no deaths: row r holds species r+1."""
    sp = sim.column(po.COL_SPECIES).ravel()
    assert list(sp) == [1, 2, 3, 4]


# ---------------------------------------------------------------------------
# actionSystem (sim.cpp:419-502)
# ---------------------------------------------------------------------------
def test_forward_step_moves_plus_one_x():
    sim = po.OracleSim(1, 69, 4, cap=16)
    _rows_by_species(sim)
    p0 = sim.column(po.COL_POS).copy()
    act = sim.column(po.COL_ACTION)
    act[:] = 0
    act[:, 0] = 1                       # forward
    sim.step()
    _rows_by_species(sim)
    p1 = sim.column(po.COL_POS)
    # identity rotation: view_dir = (1 - 2*0, 2*0*1) = (1, 0) exactly
    exp_x = np.minimum(f32(127.0), np.maximum(f32(0.0), p0[:, 0] + f32(1.0)))
    assert np.array_equal(p1[:, 0], exp_x)
    assert np.array_equal(p1[:, 1], p0[:, 1])


def test_rotate_left_ten_times_then_forward():
    sim = po.OracleSim(1, 3, 4, cap=16)
    act = sim.column(po.COL_ACTION)
    for _ in range(10):
        act = sim.column(po.COL_ACTION)
        act[:] = 0
        act[:, 2] = 1                   # rotateLeft: rot *= angleAxis(0.1, z)
        sim.step()
    p0 = sim.column(po.COL_POS).copy()
    act = sim.column(po.COL_ACTION)
    act[:] = 0
    act[:, 0] = 1
    sim.step()
    d = sim.column(po.COL_POS) - p0
    want = np.array([np.cos(1.0), np.sin(1.0)])
    for k in range(4):
        x, y = p0[k]
        if 2 < x < 125 and 2 < y < 93:          # not clamped by the walls
            assert np.allclose(d[k], want, atol=1e-5), (d[k], want)


# ---------------------------------------------------------------------------
# speciesInfoSync (sim.cpp:791-838) + rewardSystem setting 8 (sim.cpp:942-956)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
def test_reward_no_events(fixed):
    sim = po.OracleSim(1, 69, 4, cap=16, reward_fixed=fixed)
    act = sim.column(po.COL_ACTION)
    act[:] = 0
    sim.step()
    _rows_by_species(sim)
    assert not sim.column(po.COL_STATS).any()
    assert list(sim.column(po.COL_HEALTH).ravel()) == [100] * 4
    # rewards[i] = count/A + avg/100 - 2 = 1/4 + 1 - 2 = -0.75
    sr = f32(f32(f32(1.0) / f32(4.0)) + f32(f32(100.0) / f32(100.0))) - f32(2.0)
    r_own = f32(f32(sr + f32(f32(100.0) / f32(100.0))) - f32(0.5))
    rew = sim.column(po.COL_REWARD).ravel()
    if fixed:
        assert list(rew) == [r_own] * 4
    else:
        # faithful rewards[speciesID]: species 1..3 read rewards[1..3] (= -0.75),
        # species 4 reads past the array -> 0 for the table's last world (B.3)
        r4 = f32(f32(f32(0.0) + f32(1.0)) - f32(0.5))
        assert list(rew) == [r_own, r_own, r_own, r4]


def test_respawn_refills_species():
    # A = 4: any species that drops below A/4 = 1 is respawned in the same step
    sim = po.OracleSim(16, 5, 4, cap=16)
    for t in range(40):
        sim.write_synthetic_actions(99, t)
        sim.step()
        assert (sim.species_count() >= 1).all()


# ---------------------------------------------------------------------------
# updateSurroundingObservation (sim.cpp:583-654): numpy float32 restatement
# ---------------------------------------------------------------------------
def _chunk_index(cx, cy):
    x, y = int(cx), int(cy)
    if x < 0 or y < 0 or x >= 8 or y >= 6:
        return -1
    return x + y * 8


def test_surrounding_matches_numpy_restatement():
    W = 4
    sim = po.OracleSim(W, 69, 32, cap=128)
    p0 = sim.column(po.COL_POS).copy()
    act = sim.column(po.COL_ACTION)
    act[:] = 0          # no actions: the only motion is the clamp to [0, Lx-1] x [0, Ly-1]
    sim.step()
    assert sim.num_agents() == W * 32        # nobody born or died: rows are stable
    pos = sim.column(po.COL_POS)
    sur = sim.column(po.COL_SURROUND)
    # clamp (sim.cpp:485-486) and the speed heuristic (u32)(2 |dpos|) (sim.cpp:488-501)
    assert np.array_equal(pos[:, 0], np.minimum(f32(127), np.maximum(f32(0), p0[:, 0])))
    assert np.array_equal(pos[:, 1], np.minimum(f32(95), np.maximum(f32(0), p0[:, 1])))
    d = pos - p0
    speed = (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) * f32(2)).astype(np.uint32)
    # export rows are ordered (species, world, slot): rebuild per-world row lists
    sc = sim.species_count()
    row = 0
    rows_of = {w: [] for w in range(W)}
    for s in range(4):
        for w in range(W):
            rows_of[w] += list(range(row, row + sc[w, s]))
            row += sc[w, s]
    for w in range(W):
        rr = rows_of[w]
        n_ag = np.zeros(48, np.uint32)
        t_sp = np.zeros(48, np.uint32)
        for r in rr:
            c = _chunk_index(np.floor(pos[r, 0] / f32(16)), np.floor(pos[r, 1] / f32(16)))
            n_ag[c] += 1
            t_sp[c] += speed[r]
        for r in rr:
            cpx = pos[r, 0] - f32(8.0)
            cpy = pos[r, 1] - f32(8.0)
            chx, chy = cpx / f32(16), cpy / f32(16)
            x0, y0, x1, y1 = np.floor(chx), np.floor(chy), np.ceil(chx), np.ceil(chy)
            idx = [_chunk_index(x0, y0), _chunk_index(x1, y0), _chunk_index(x0, y1),
                   _chunk_index(x1, y1)]
            xi, yi = chx - x0, chy - y0
            for col, cnt in ((0, n_ag), (1, t_sp)):
                n = [f32(cnt[i]) if i >= 0 else f32(0) for i in idx]
                nx0 = xi * n[1] + (f32(1) - xi) * n[0]
                nx1 = xi * n[3] + (f32(1) - xi) * n[2]
                want = yi * nx1 + (f32(1) - yi) * nx0
                assert sur[r, col] == want, (w, r, col, sur[r, col], want)


def test_surround_at_chunk_centroid_is_that_count():
    # at a chunk centroid (8 + 16 i, 8 + 16 j) the interpolants are 0 and the
    # presence heuristic is exactly that chunk's agent count
    chx = (f32(8 + 16 * 3) - f32(8)) / f32(16)
    assert chx - np.floor(chx) == 0.0


# ---------------------------------------------------------------------------
# Export invariants and shift_observations (sim.cpp:1002-1048)
# ---------------------------------------------------------------------------
def test_export_invariants_and_shift():
    sim = po.OracleSim(32, 11, 32, cap=128)
    for t in range(30):
        sim.write_synthetic_actions(1234, t, True)
        sim.step()
        N = sim.num_agents()
        sc = sim.species_count()
        assert sc.sum() == N
        sp = sim.column(po.COL_SPECIES).ravel()
        assert (np.diff(sp) >= 0).all()             # species-major rows
        assert list(np.bincount(sp, minlength=5)[1:]) == list(sc.sum(0))
        assert (sim.column(po.COL_HEALTH) > 0).all()
        sem = sim.column(po.COL_SEMANTIC)
        assert set(np.unique(sem).tolist()) <= {-1, 1, 2, 3, 4, 5, 6}   # -1: a miss
        sim.shift_observations()
        for c in (po.COL_SPECIES, po.COL_POS, po.COL_HEALTH, po.COL_SURROUND, po.COL_REWARD,
                  po.COL_ACTION, po.COL_HIDDEN):
            assert np.array_equal(sim.column(c), sim.column(c, True))
        st, pst = sim.column(po.COL_STATS), sim.column(po.COL_STATS, True)
        assert np.array_equal(pst[:, [0, 2, 3]], st[:, [0, 2, 3]])
        assert np.array_equal(pst[:, 1], st[:, 0])  # hitEnemy <- hitFriendly (sim.cpp:1034)
    assert sim.overflow() == 0


def test_prev_sensor_is_last_steps_sensor():
    sim = po.OracleSim(1, 69, 4, cap=16)
    act = sim.column(po.COL_ACTION)
    act[:] = 0
    sim.step()
    sem0 = sim.column(po.COL_SEMANTIC).copy()
    act = sim.column(po.COL_ACTION)
    act[:] = 0
    act[:, 2] = 1
    sim.step()
    _rows_by_species(sim)
    assert np.array_equal(sim.column(po.COL_SEMANTIC, True), sem0)


def test_health_export_is_int_bits():
    # health_tensor views int32 health as float32 (types.hpp:119-124, mgr.cpp:329-346)
    h = np.array([100], np.int32).view(np.float32)[0]
    assert h == np.float32(1.4e-43)


# ---- food boxes (the +-1 cube of sim.cpp:332-341, rotated) ----
FWD = list(range(24))


def _hit_pixels(hit):
    return [k for k in range(33) if hit[k]]


def test_food_box_axis_aligned_ahead():
    # box centre 10 ahead, rotation 0: spans Y in [-1, 1] from X = 9, so the
    # line Y = u X meets it iff |u| <= 1/9: pixels 11, 12 (u = -+1/24) + finder
    hit, z = po.probe_box((20.0, 20.0), (1.0, 0.0), (30.0, 20.0), 0)
    assert _hit_pixels(hit) == [11, 12, 32]
    assert z[11] == z[12] == z[32] == 9.0          # nearest face at view depth 9


def test_food_box_diagonal_is_wider_and_nearer():
    # a quarter-turn fraction 1/2 (45 degrees): corners at sqrt 2 on the
    # diagonals, |u| <= sqrt(2)/10 = 0.141 covers pixels 10..13 (u = -+0.125)
    hit, z = po.probe_box((20.0, 20.0), (1.0, 0.0), (30.0, 20.0), 1 << 21)
    assert _hit_pixels(hit) == [10, 11, 12, 13, 32]
    assert abs(float(z[10]) - (10.0 - 2.0 ** 0.5)) < 1e-3
    # rotation by a full quarter turn is the same square as rotation 0
    hit_q, z_q = po.probe_box((20.0, 20.0), (1.0, 0.0), (30.0, 20.0), (1 << 22) - 1)
    assert _hit_pixels(hit_q) == [11, 12, 32]


def test_food_box_behind_uses_backward_camera():
    # backward pixels 24..31 at u = (2k+1)/8 - 1: only the 45-degree box reaches
    # |u| = 0.125 (pixels 27, 28); no forward pixel, no finder
    hit, _ = po.probe_box((50.0, 20.0), (1.0, 0.0), (40.0, 20.0), 0)
    assert _hit_pixels(hit) == []
    hit, z = po.probe_box((50.0, 20.0), (1.0, 0.0), (40.0, 20.0), 1 << 21)
    assert _hit_pixels(hit) == [27, 28]
    assert abs(float(z[27]) - (10.0 - 2.0 ** 0.5)) < 1e-3


def test_food_box_containing_the_agent_near_sphere():
    # the agent at the centre of an axis-aligned box, heading +x: ray (1, u)
    # leaves the box at X = 1, t = sqrt(1 + u^2), seen iff t >= 1.1 (nearSphere,
    # mgr.cpp:133): |u| >= 0.458 -> forward pixels 0..6, 17..23, backward
    # u = +-7/8, +-5/8 (24, 25, 30, 31); the finder (t = 1) sees nothing of it
    hit, z = po.probe_box((20.0, 20.0), (1.0, 0.0), (20.0, 20.0), 0)
    assert _hit_pixels(hit) == list(range(7)) + list(range(17, 26)) + [30, 31]
    assert (z[hit] == 0.0).all()


# ---- the near sphere and the agent disc -------------------
# (the float64 geometry lives in scene_ref.py, shared with the scene renderer)
from scene_ref import NEAR, R_AGENT, dirs as _dirs, ref_box as _ref_box, ref_disc as _ref_disc  # noqa: E402,F401


def test_disc_at_1_5_ahead():
    # centre 1.5 ahead: the line reaches the 0.92 disc for |u| <= 0.777 (pixels
    # 3..20) and every such ray leaves it beyond 1.1; depth f - R = 0.58
    hit, z = po.probe_agent((30.0, 30.0), (1.0, 0.0), (31.5, 30.0))
    assert _hit_pixels(hit) == list(range(3, 21)) + [32]
    assert (np.abs(z[hit] - 0.58) < 1e-3).all()
    ref, _ = _ref_disc((30.0, 30.0), (1.0, 0.0), (31.5, 30.0))
    assert np.array_equal(hit, ref)


def test_disc_at_0_9_ahead_overlapping_bodies():
    # centre 0.9 ahead: the camera lies inside the other agent's disc; rays see
    # its far side where it reaches past the near sphere (the finder does:
    # its near point (1.1, 0) is 0.2 from the centre); depth clamps at 0
    hit, z = po.probe_agent((30.0, 30.0), (1.0, 0.0), (30.9, 30.0))
    ref, margin = _ref_disc((30.0, 30.0), (1.0, 0.0), (30.9, 30.0))
    assert margin.min() > 1e-4
    assert np.array_equal(hit, ref)
    assert hit[32] and hit[:24].any() and not hit[24:32].any()
    assert (z[hit] == 0.0).all()


def test_disc_inside_the_near_sphere_is_invisible():
    # 0.1 + 0.92 < 1.1: the whole disc lies inside the near sphere
    for c in ((30.1, 30.0), (30.0, 30.05), (29.9, 30.0)):
        hit, _ = po.probe_agent((30.0, 30.0), (1.0, 0.0), c)
        assert not hit.any(), c


def test_disc_behind_is_seen_by_backward_pixels():
    hit, z = po.probe_agent((30.0, 30.0), (0.0, 1.0), (30.0, 28.5))
    ref, _ = _ref_disc((30.0, 30.0), (0.0, 1.0), (30.0, 28.5))
    assert np.array_equal(hit, ref)
    assert _hit_pixels(hit) == list(range(25, 31))      # |u| <= 0.777: not +-7/8
    assert (np.abs(z[hit] - 0.58) < 1e-3).all()


def test_disc_and_box_predicates_match_float64_restatement():
    """2000 random (agent, heading, object) configurations within 4 units:
    every ray not within 1e-4 of a decision boundary agrees with the float64
    geometry (discs of radius 0.92, rotated unit squares, near sphere 1.1)."""
    rng = np.random.default_rng(7)
    checked = 0
    for t in range(2000):
        a = rng.uniform(10, 60, 2).astype(np.float32)
        th = rng.uniform(0, 2 * np.pi)
        h = (np.float32(np.cos(th)), np.float32(np.sin(th)))
        c = (a + rng.uniform(-4, 4, 2)).astype(np.float32)
        if t % 2:
            hit, _ = po.probe_agent(a, h, c)
            ref, margin = _ref_disc(a.astype(np.float64), np.array(h, np.float64), c.astype(np.float64))
        else:
            rot = int(rng.integers(0, 1 << 22))
            hit, _ = po.probe_box(a, h, c, rot)
            ref, margin = _ref_box(a.astype(np.float64), np.array(h, np.float64), c.astype(np.float64), rot)
        ok = margin > 1e-4
        assert np.array_equal(hit[ok], ref[ok]), (t, a, h, c)
        checked += int(ok.sum())
    assert checked > 60000


def test_walls_near_sphere_classes():
    # agent 0.5 from the left wall looking at it: every forward near point lies
    # beyond the wall box (x < -0.2): a miss (semantic -1, depth 255); the
    # backward pixels see the right wall's inner face 127.3 away
    sem, dep = po.probe_walls((0.5, 50.0), (-1.0, 0.0))
    assert (sem[:24] == -1).all() and sem[32] == -1 and (dep[:24] == 255).all()
    assert (sem[24:32] == 5).all() and dep[27] == dep[28] == 127
    # 1.0 from it: the central near points fall inside the wall box (the wall,
    # depth s0 = 1.1 / |(1, u)| -> byte 1), the outer ones still in the arena
    # (the wall's face 0.8 ahead along the heading -> byte 0)
    sem, dep = po.probe_walls((1.0, 50.0), (-1.0, 0.0))
    assert (sem[:24] == 5).all() and sem[32] == 5
    assert dep[11] == dep[12] == dep[32] == 1 and dep[0] == dep[23] == 0
    # the arena's middle: every ray ends on a wall
    sem, dep = po.probe_walls((64.0, 48.0), (1.0, 0.0))
    assert (sem == 5).all() and dep[11] == 63 and dep[27] == 63


def test_food_box_rotation_follows_heading_frame():
    # heading +y: a box 10 ahead along +y behaves like the +x case
    hit, z = po.probe_box((20.0, 20.0), (0.0, 1.0), (20.0, 30.0), 0)
    assert _hit_pixels(hit) == [11, 12, 32] and z[11] == 9.0


# ---------------------------------------------------------------------------
# Resets and episodes (INTEGRATION.md "Episodes and resets"; the key schedule
# split_i(initKey, episode, world) of sim.cpp:64-75, :1236-1240).  These pin the
# oracle's own restatement: no manager is involved.
# ---------------------------------------------------------------------------
from reset_util import initial_positions  # noqa: E402

_NAMES = ["species", "pos", "health", "surround", "reward", "action", "stats", "hidden", "semantic",
          "depth"]


def _drive_o(sims, t):
    for s in sims:
        s.step()
        s.shift_observations()
        s.write_synthetic_actions(1234, t, True)


def _bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _tables_equal(a, b, where):
    """Two oracles: every column, current and Prev, bitwise."""
    sa, sb = a.snapshot(), b.snapshot()
    for k in sa:
        assert _bytes_equal(sa[k], sb[k]), (where, k)


def _world_slots(sim, w, prev=False):
    """World w's rows of every column in slot order."""
    cnt, off = sim.world_counts()
    rows = sim.sensor_index()[off[w]:off[w] + cnt[w]]
    return {nm: sim.column(i, prev)[rows] for i, nm in enumerate(_NAMES)}


def _worlds_equal(a, wa, b, wb, where, prev=False):
    """World wa of oracle a against world wb of oracle b: the slot state and
    every column in slot order."""
    sa, sb = a.world_state(wa), b.world_state(wb)
    for k in sa:
        assert _bytes_equal(sa[k], sb[k]), (where, "state", k)
    ca, cb = _world_slots(a, wa, prev), _world_slots(b, wb, prev)
    for k in ca:
        assert _bytes_equal(ca[k], cb[k]), (where, k, prev)


@pytest.mark.parametrize("A", [4, 32])
@pytest.mark.parametrize("e", [0, 1, 7])
@pytest.mark.parametrize("off", [0, 7])
def test_reset_positions_from_threefry(A, e, off):
    W, w = 3, 2
    sim = po.OracleSim(W, 69, A, cap=128, world_offset=off)
    for t in range(3):
        _drive_o((sim,), t)
    sim.column(po.COL_ACTION)[:] = 0
    sim.reset_worlds([off + w], [e])
    assert list(sim.reset_flags()) == [0, 0, e + 2]
    sim.step()
    assert list(sim.episode()) == [0, 0, e] and list(sim.episode_step()) == [4, 4, 1]
    assert list(sim.reset_flags()) == [0, 0, 0]
    st = sim.world_state(w)
    assert list(st["species"]) == [i % 4 + 1 for i in range(A)]
    assert (st["health"][:A] >= 100).all()
    want = initial_positions(69, A, e, off + w)
    # the step's only motion on all-zero actions: the clamp of sim.cpp:485-486
    want[:, 0] = np.minimum(f32(127), np.maximum(f32(0), want[:, 0]))
    want[:, 1] = np.minimum(f32(95), np.maximum(f32(0), want[:, 1]))
    assert _bytes_equal(st["xy"], want)
    assert _bytes_equal(st["rot"], np.tile(np.array([1, 0], np.float32), (A, 1)))
    # a reset world's rows are new: Action, HiddenState and every Prev column zero
    for prev in (False, True):
        c = _world_slots(sim, w, prev)
        for nm in (("action", "hidden") if not prev else _NAMES):
            assert not c[nm].view(np.uint8).any(), (nm, prev)
    # an index outside the oracle's worlds is another rank's
    sim.reset_worlds([off + W, (off - 1) & 0xFFFFFFFF])
    assert list(sim.reset_flags()) == [0, 0, 0]


def test_reset_everything_equals_fresh_oracle():
    W = 5
    sim = po.OracleSim(W, 69, 32)
    for t in range(6):
        _drive_o((sim,), t)
    sim.reset_worlds(range(W), [0] * W)
    fresh = po.OracleSim(W, 69, 32)
    for t in range(6, 12):
        for s in (sim, fresh):
            s.step()
        _tables_equal(sim, fresh, f"step {t}")
        for s in (sim, fresh):
            s.shift_observations()
        _tables_equal(sim, fresh, f"shift {t}")
        for s in (sim, fresh):
            s.write_synthetic_actions(1234, t, True)
    assert list(sim.episode()) == [0] * W and list(sim.episode_step()) == [6] * W
    assert list(fresh.episode_step()) == [6] * W


def test_partial_reset_equals_one_world_oracles():
    W = 5
    sim, never = po.OracleSim(W, 69, 32, reward_fixed=True), po.OracleSim(W, 69, 32, reward_fixed=True)
    for t in range(6):
        _drive_o((sim, never), t)
    sim.reset_worlds([1, 3], [0, 0])
    ones = {w: po.OracleSim(1, 69, 32, world_offset=w, reward_fixed=True) for w in (1, 3)}
    for t in range(6, 14):
        for s in [sim, never] + list(ones.values()):
            s.step()
        for prev in (False, True):
            for w in (1, 3):
                _worlds_equal(sim, w, ones[w], 0, f"step {t} world {w}", prev)
            for w in (0, 2, 4):
                _worlds_equal(sim, w, never, w, f"step {t} world {w}", prev)
        for s in [sim, never] + list(ones.values()):
            s.shift_observations()
            s.write_synthetic_actions(1234, t, True)
    assert list(sim.episode_step()) == [14, 8, 14, 8, 14]
    assert list(sim.episode()) == [0] * W


def test_episode_length_and_flag_forms():
    W = 3
    sim, twin = po.OracleSim(W, 69, 32), po.OracleSim(W, 69, 32)
    sim.set_episode_length(4)
    for t in range(11):
        if t and t % 4 == 0:
            twin.reset_worlds(range(W))
        _drive_o((sim, twin), t)
        assert list(sim.episode_step()) == [t % 4 + 1] * W, t
        assert list(sim.episode()) == [t // 4] * W, t
        assert list(twin.episode()) == [t // 4] * W, t
        _tables_equal(sim, twin, f"step {t}")
    # a flag written as 1 is reset_worlds([w]); as e + 2, reset_worlds([w], [e])
    a, b = po.OracleSim(W, 69, 32, world_offset=5), po.OracleSim(W, 69, 32, world_offset=5)
    flags = a.reset_flags()        # (taken early: the array is live)
    for t in range(4):
        _drive_o((a, b), t)
    flags[2] = 1
    b.reset_worlds([5 + 2])
    assert list(b.reset_flags()) == [0, 0, 1]
    for t in range(4, 7):
        _drive_o((a, b), t)
        _tables_equal(a, b, f"flag 1, step {t}")
    assert list(a.episode()) == list(b.episode()) == [0, 0, 1]
    flags[0] = 5 + 2
    b.reset_worlds([5], [5])
    assert list(b.reset_flags()) == [7, 0, 0]
    for t in range(7, 10):
        _drive_o((a, b), t)
        _tables_equal(a, b, f"flag e + 2, step {t}")
    assert list(a.episode()) == list(b.episode()) == [5, 0, 1]
    assert list(a.episode_step()) == list(b.episode_step()) == [3, 10, 6]
    assert list(a.reset_flags()) == [0] * W


def test_faithful_reward_reads_the_reset_neighbour():
    """B.3: species 4 of world w reads species_reward[0] of world w + 1, which
    is final after phase A of every world -- so in the step that resets world
    1, world 0's species-4 rows read the reward of world 1's fresh population."""
    W, A = 3, 32
    sim, never = po.OracleSim(W, 69, A), po.OracleSim(W, 69, A)
    # (action stream 1246: under it world 1's species 1 has bred and been shot
    # by step 5 -- 9 agents, healths 60 and 50 among them -- so its old
    # population's reward differs from a fresh one's; under 1234 it does not)
    for t in range(5):
        for s in (sim, never):
            s.step()
            s.shift_observations()
            s.write_synthetic_actions(1246, t, True)
    sim.reset_worlds([1])
    sim.step()
    never.step()
    assert list(sim.episode()) == [0, 1, 0] and list(sim.episode_step()) == [6, 1, 6]

    def sr0_of_world_1(s):
        # speciesInfoSync (sim.cpp:791-838) over world 1's species-1 agents;
        # nobody of a fresh population dies or is born in its first step
        c = _world_slots(s, 1)
        h = c["health"][c["species"].ravel() == 1].ravel()
        count = len(h)
        avg = f32(np.uint32(h.sum())) / f32(count)
        return f32(f32(f32(count) / f32(A)) + f32(avg / f32(100.0))) - f32(2.0)

    c1 = _world_slots(sim, 1)
    assert len(c1["species"]) == A and (c1["species"].ravel() == 1).sum() == A // 4
    sr = sr0_of_world_1(sim)
    c0 = _world_slots(sim, 0)
    sp4 = c0["species"].ravel() == 4
    assert sp4.any()
    want = []
    for hp, st in zip(c0["health"][sp4].ravel(), c0["stats"][sp4]):
        rew = f32(f32(sr + f32(f32(hp) / f32(100.0))) - f32(0.5))    # rewardSystem :942-956
        if st[2]:
            rew = f32(rew + f32(10.0))
        if st[3]:
            rew = f32(rew + f32(10.0))
        if st[1]:
            rew = f32(rew + f32(15.0))
        want.append(rew)
    assert _bytes_equal(c0["reward"][sp4].ravel(), np.array(want, np.float32))
    # (the check bites: world 1's old population would have given another reward)
    n0 = _world_slots(never, 0)
    assert _bytes_equal(n0["health"], c0["health"]) and _bytes_equal(n0["stats"], c0["stats"])
    assert not _bytes_equal(n0["reward"][sp4], c0["reward"][sp4])
    # species 1..3 of world 0 and all of world 2 (the table's last: 0) are untouched
    assert _bytes_equal(n0["reward"][~sp4], c0["reward"][~sp4])
    assert _bytes_equal(_world_slots(never, 2)["reward"], _world_slots(sim, 2)["reward"])
