"""Per-world resets and episodes against the oracle, in both execution modes.

The oracle restates resets from INTEGRATION.md "Episodes and resets" and the
reference's key schedule on its own (oracle/mbots_oracle.h; its known answers
are in tests/test_oracle_kat.py), so a reading of the semantics that the HIP
kernels and the CPU mode share -- which the twin comparisons of
tests/test_reset_gpu.py cannot see -- shows here.  Every comparison is
simpair.compare with the Prev columns plus the three episode arrays.

The driver: step(); shift_observations(); write_synthetic_actions(1234, t, True)."""
import numpy as np
import pytest

import pyoracle
from reset_util import episode_errors
from simpair import COLUMNS, compare
from test_grow_capacity import _breed_heavy

SEED = 69

MODES = [pytest.param("cpu"), pytest.param("hip", marks=pytest.mark.gpu)]


def _mgr(mode, W, A=32, **kw):
    import madrona_bots as mb
    return mb.SimManager(0, W, SEED, A, exec_mode=mode, **kw)


def _check(mgr, orc, where):
    errs = compare(mgr, orc, where, prev_too=True) + episode_errors(mgr, orc, where)
    assert not errs, errs[:5]


def _drive_checked(mgr, orc, t, where=""):
    """One driver round, compared after the step and after the shift."""
    for s in (mgr, orc):
        s.step()
    _check(mgr, orc, f"{where}step {t}")
    for s in (mgr, orc):
        s.shift_observations()
    _check(mgr, orc, f"{where}shift {t}")
    for s in (mgr, orc):
        s.write_synthetic_actions(1234, t, True)


# A, capacity.  The reset body spreads its 2 A draws over the lanes 64 per
# round, the even lanes taking y from the neighbour lane: A = 4 is a fraction
# of one round, 31 and 33 are odd counts whose last round holds 62 and 2 draws,
# 64 fills two rounds, 100 ends in a round of 8, 128 fills four rounds and
# every slot of the world, 96 is three rounds in the 256-slot class.
@pytest.mark.parametrize("A,cap", [(4, 16), (31, 128), (33, 128), (64, 128), (100, 128), (128, 128),
                                   (96, 256)])
@pytest.mark.parametrize("mode", MODES)
def test_draw_rounds_of_the_reset_body(mode, A, cap):
    W = 6
    mgr = _mgr(mode, W, A, agent_capacity=cap)
    orc = pyoracle.OracleSim(W, SEED, A, cap=cap, num_threads=4)
    t = 0
    for rnd, episodes in enumerate(([5, None, None], [None, 3, None])):
        for _ in range(4):
            _drive_checked(mgr, orc, t, f"round {rnd} ")
            t += 1
        # {0, 2, 5}: one with an explicit episode, the others their next one
        plain = [w for w, e in zip((0, 2, 5), episodes) if e is None]
        expl = [(w, e) for w, e in zip((0, 2, 5), episodes) if e is not None]
        for s in (mgr, orc):
            s.reset_worlds(plain)
            s.reset_worlds([w for w, _ in expl], [e for _, e in expl])
        _check(mgr, orc, f"round {rnd} flagged")
        for _ in range(6):
            _drive_checked(mgr, orc, t, f"round {rnd} reset ")
            t += 1
    assert orc.episode().tolist() == [6, 0, 3, 0, 0, 2]
    assert orc.episode_step().tolist() == [6, 20, 6, 20, 20, 6]
    assert mgr.overflow() == orc.overflow()


def _world_rows(n_of, off_of, sidx, w):
    return sidx[off_of[w]:off_of[w] + n_of[w]]


def _check_per_world(mgr, orc, W, where):
    """Worlds 0..W-1 of the manager against the same worlds of an oracle that
    holds one world more (the manager's ghost): the state and, in slot order
    through sensor_index, every column, current and Prev.  (The oracle's
    species-major rows differ from the manager's by the extra world's.)"""
    cnt, off = orc.world_counts()
    osidx = orc.sensor_index()
    msidx = mgr.sensor_index_tensor().to_torch().cpu().numpy().reshape(-1)
    moff = [mgr.agent_offset_for_world(w) for w in range(W)]
    assert mgr.num_agents() == int(cnt[:W].sum()), where
    assert np.array_equal(mgr.species_count_tensor().to_torch().cpu().numpy(), orc.species_count()[:W]), where
    cols = {}
    for name, cid in COLUMNS:
        for prev in (False, True):
            cols[name, prev] = (getattr(mgr, name)(prev).to_torch().cpu().numpy(), orc.column(cid, prev))
    for w in range(W):
        ms, os_ = mgr.world_state(w), orc.world_state(w)
        for km, ko in (("position", "xy"), ("rotation_wz", "rot"), ("species", "species"),
                       ("health", "health"), ("food", "food")):
            a, b = np.ascontiguousarray(ms[km]), np.ascontiguousarray(os_[ko])
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (where, w, km)
        ra, rb = msidx[moff[w]:moff[w] + cnt[w]], _world_rows(cnt, off, osidx, w)
        for (name, prev), (g, o) in cols.items():
            x, y = np.ascontiguousarray(g[ra]), np.ascontiguousarray(o[rb])
            assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), \
                (where, w, name, prev)
    errs = episode_errors(mgr, orc, where)
    assert not errs, errs


@pytest.mark.parametrize("mode", MODES)
def test_faithful_reward_over_a_reset_neighbour_and_the_ghost(mode):
    """W = 37 with the shard ghost against an oracle of 38 worlds, default
    (faithful, B.3) rewards: species 4 of world w reads species_reward[0] of
    world w + 1.  World 35 never resets and world 36 does; world 36 reads the
    ghost, which resets with it.  In the resetting steps those rewards come from
    the neighbour's fresh population."""
    W = 37
    mgr = _mgr(mode, W, shard_ghost=True)
    orc = pyoracle.OracleSim(W + 1, SEED, 32, num_threads=4)

    def drive(t):
        for s in (mgr, orc):
            s.step()
        _check_per_world(mgr, orc, W, f"step {t}")
        for s in (mgr, orc):
            s.shift_observations()
        _check_per_world(mgr, orc, W, f"shift {t}")
        for s in (mgr, orc):
            s.write_synthetic_actions(1234, t, True)

    for t in range(4):
        drive(t)
    for s in (mgr, orc):
        s.reset_worlds([36, 37], [3, 3])
    for t in range(4, 7):
        drive(t)
    for s in (mgr, orc):
        s.set_episode_length(7)
    # (every world but 36 and the ghost is 7 steps old: they all expire at
    # step 7; 36 and the ghost at step 11, where {0, 36} are flagged too)
    for t in range(7, 11):
        drive(t)
    for s in (mgr, orc):
        s.reset_worlds([0, 36])
    for t in range(11, 14):
        drive(t)
    assert orc.episode().tolist() == [2] + [1] * 35 + [4, 4]
    assert orc.episode_step().tolist() == [3] + [7] * 35 + [3, 3]


@pytest.mark.parametrize("mode", MODES)
def test_reset_into_a_smaller_population_mixed_classes(mode):
    """Capacity 512, 8 worlds, 29 breed-heavy steps (populations 88..161), then
    worlds 4 and 5 start over with 32 agents and breed on for 12 steps: their
    births land in slots the old populations used, whose sur / stats the reset
    left alone above slot 32.  A world is in the class range while 2 n + 32 >
    128 (DESIGN.md "Mixed classes"); world 4 is reset again one step after it
    is back in it."""
    W = 8
    mgr = _mgr(mode, W, agent_capacity=512)
    orc = pyoracle.OracleSim(W, SEED, 32, cap=512, num_threads=4)

    def drive(t):
        for s in (mgr, orc):
            s.step()
        _check(mgr, orc, f"step {t}")
        for s in (mgr, orc):
            s.shift_observations()
        _check(mgr, orc, f"shift {t}")
        a = _breed_heavy(mgr.num_agents(), t)
        mgr.action_tensor().to_torch().copy_(a.to(mgr.device))
        orc.column(pyoracle.COL_ACTION)[:] = a.numpy()

    for t in range(1, 30):
        drive(t)
    assert orc.world_counts()[0].tolist() == [146, 111, 132, 146, 161, 88, 156, 116]
    for s in (mgr, orc):
        s.reset_worlds([4, 5])
    back_in_range = again = None
    for t in range(30, 44):   # (12 steps, and 2 more past the second reset)
        if back_in_range is not None and t == back_in_range + 1:
            for s in (mgr, orc):
                s.reset_worlds([4])
            again = t
        drive(t)
        n4 = int(orc.world_counts()[0][4])
        if t == 30:
            assert orc.world_counts()[0][[4, 5]].tolist() == [32, 32]
        if back_in_range is None and 2 * n4 + 32 > 128:
            back_in_range = t
    # what happened: world 4 (32 agents at step 30) holds 49 or more after
    # step 40, so 2 n + 32 > 128 again, and step 41 resets it a second time
    assert (back_in_range, again) == (40, 41)
    assert orc.episode().tolist() == [0, 0, 0, 0, 2, 1, 0, 0]
    assert mgr.overflow() == orc.overflow() == 0

