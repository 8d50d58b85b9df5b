"""Per-world resets and episodes, CPU mode (mbots_reset_worlds,
mbots_set_episode_length, MBOTS_EXPORT_RESET / EPISODE / EPISODE_STEP;
SimManager.reset_worlds, reset_tensor, episode_tensor, episode_step_tensor,
set_episode_length).

Reset, then step: a flagged world is re-initialised at the start of the next
step() from its episode's key -- threefry2x32(seed, 0, episode, global world),
the reference's split_i(initKey, episode, world) -- and then stepped.  So a
manager whose worlds are all reset to episode 0 equals, bitwise on every column,
a fresh oracle driven by the same calls from its creation, and a single reset
world a one-world oracle created at that world's global index.

The driver throughout: step(); shift_observations();
write_synthetic_actions(1234, t, True)."""
import numpy as np
import pytest
import torch

import pyoracle
from reset_util import initial_positions
from simpair import COLUMNS, compare

SEED, A = 69, 32


def _cpu(W, **kw):
    import madrona_bots as mb
    return mb.SimManager(0, W, SEED, A, exec_mode="cpu", **kw)


def _drive(sims, t):
    for s in sims:
        s.step()
        s.shift_observations()
        s.write_synthetic_actions(1234, t, True)


def _same(a, b, where):
    """Two managers: every exported column, current and Prev, bitwise."""
    assert a.num_agents() == b.num_agents(), where
    assert torch.equal(a.species_count_tensor().to_torch().cpu(), b.species_count_tensor().to_torch().cpu()), where
    for name in [c[0] for c in COLUMNS] + ["depth_tensor"]:
        for prev in (False, True):
            x = getattr(a, name)(prev).to_torch().cpu()
            y = getattr(b, name)(prev).to_torch().cpu()
            assert x.shape == y.shape, (where, name, prev)
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (where, name, prev)


def _ints(t):
    return t.to_torch().cpu().numpy().reshape(-1).tolist()


def _world_rows(m, w):
    """Export rows of world w's agents in slot order."""
    off = m.agent_offset_for_world(w)
    n = len(m.world_state(w)["species"])
    return m.sensor_index_tensor().to_torch().cpu().numpy().reshape(-1)[off:off + n]


def _state_equal(sa, sb, where):
    """world_state dicts of a manager (sa) and a manager or an oracle (sb)."""
    pos_b = sb["position"] if "position" in sb else sb["xy"]
    rot_b = sb["rotation_wz"] if "rotation_wz" in sb else sb["rot"]
    assert sa["position"].shape == pos_b.shape, where
    assert np.array_equal(sa["position"].view(np.uint32), np.ascontiguousarray(pos_b).view(np.uint32)), where
    assert np.array_equal(sa["rotation_wz"].view(np.uint32), np.ascontiguousarray(rot_b).view(np.uint32)), where
    for k in ("species", "health", "finder"):
        assert np.array_equal(sa[k], sb[k]), (where, k)
    assert np.array_equal(sa["food"], sb["food"]), (where, "food")


def _world_equals_oracle(m, w, orc, where):
    """World w of manager m against the one-world oracle orc: the state and,
    in slot order, every current column."""
    _state_equal(m.world_state(w), orc.world_state(0), where)
    rows, orows = _world_rows(m, w), orc.sensor_index()
    for name, cid in COLUMNS:
        g = getattr(m, name)(False).to_torch().cpu().numpy()[rows]
        o = orc.column(cid)[orows]
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(o).view(np.uint8)), \
            (where, name)


def _world_equals_world(m, b, w, where):
    _state_equal(m.world_state(w), b.world_state(w), where)
    ra, rb = _world_rows(m, w), _world_rows(b, w)
    for name, _ in COLUMNS:
        x = getattr(m, name)(False).to_torch().cpu().numpy()[ra]
        y = getattr(b, name)(False).to_torch().cpu().numpy()[rb]
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), \
            (where, name)


def _initial_positions(episode, gw):
    """The test's own computation of a world's initial positions
    (reset_util.initial_positions, shared with the oracle's known answers)."""
    return initial_positions(SEED, A, episode, gw)


# ------------------------------------------------------------------ tests --
def test_reset_everything_equals_fresh():
    W = 5
    mgr = _cpu(W)
    for t in range(6):
        _drive((mgr,), t)
    mgr.reset_worlds(range(W), episodes=[0] * W)
    orc = pyoracle.OracleSim(W, SEED, A)
    for t in range(6, 12):
        for s in (mgr, orc):
            s.step()
        errs = compare(mgr, orc, f"step {t}", prev_too=True)
        assert not errs, errs[:5]
        for s in (mgr, orc):
            s.shift_observations()
        errs = compare(mgr, orc, f"shift {t}", prev_too=True)
        assert not errs, errs[:5]
        for s in (mgr, orc):
            s.write_synthetic_actions(1234, t, True)
    assert _ints(mgr.episode_tensor()) == [0] * W
    assert _ints(mgr.episode_step_tensor()) == [6] * W


def test_partial_reset():
    W = 5
    mgr, twin = _cpu(W, reward_fixed=True), _cpu(W, reward_fixed=True)
    for t in range(6):
        _drive((mgr, twin), t)
    mgr.reset_worlds([1, 3], episodes=[0, 0])
    orcs = {w: pyoracle.OracleSim(1, SEED, A, world_offset=w, reward_fixed=True) for w in (1, 3)}
    for t in range(6, 14):
        for s in [mgr, twin] + list(orcs.values()):
            s.step()
        for w in (1, 3):
            _world_equals_oracle(mgr, w, orcs[w], f"step {t} world {w}")
        for w in (0, 2, 4):
            _world_equals_world(mgr, twin, w, f"step {t} world {w}")
        for s in [mgr, twin] + list(orcs.values()):
            s.shift_observations()
            s.write_synthetic_actions(1234, t, True)
    assert _ints(mgr.episode_step_tensor()) == [14, 8, 14, 8, 14]


def test_episodes():
    W = 5
    mgr = _cpu(W)
    for _ in range(3):
        mgr.reset_worlds([2])
        mgr.step()
    assert _ints(mgr.episode_tensor()) == [0, 0, 3, 0, 0]
    # an explicit episode: the reset world does not move on all-zero actions
    # (its rows are new), so one step later its agents stand where the
    # episode's key put them
    for e in (1, 2):
        m = _cpu(W, world_offset=7)
        _drive((m,), 0)
        m.reset_worlds([7 + 2], [e])
        m.step()
        assert _ints(m.episode_tensor())[2] == e
        got = m.world_state(2)["position"][:A]
        want = _initial_positions(e, 7 + 2)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), e
    # the same explicit episode twice: identical columns for 5 steps; episodes
    # 0 and 1 differ
    a, b, c = _cpu(W), _cpu(W), _cpu(W)
    for t in range(3):
        _drive((a, c), t)
    _drive((b,), 9)   # (another history before the reset)
    a.reset_worlds(range(W), [1] * W)
    b.reset_worlds(range(W), [1] * W)
    c.reset_worlds(range(W), [0] * W)
    differs = False
    for t in range(5):
        _drive((a, b, c), t)
        _same(a, b, f"episode 1 twice, step {t}")
        pa, pc = a.position_tensor().to_torch(), c.position_tensor().to_torch()
        differs = differs or pa.shape != pc.shape or not torch.equal(pa, pc)
    assert differs


def test_flag_path_equals_call_path():
    W = 5
    a, b = _cpu(W), _cpu(W)
    for t in range(4):
        _drive((a, b), t)
    a.reset_tensor().to_torch()[3] = 1
    b.reset_worlds([3])
    assert _ints(b.reset_tensor())[3] == 1
    for t in range(4, 7):
        _drive((a, b), t)
        _same(a, b, f"flag 1, step {t}")
        assert _ints(a.reset_tensor()) == [0] * W
    assert _ints(a.episode_tensor()) == _ints(b.episode_tensor()) == [0, 0, 0, 1, 0]
    # e + 2 selects episode e
    a.reset_tensor().to_torch()[1] = 5 + 2
    b.reset_worlds([1], [5])
    assert _ints(b.reset_tensor())[1] == 7
    for t in range(7, 10):
        _drive((a, b), t)
        _same(a, b, f"flag e + 2, step {t}")
    assert _ints(a.episode_tensor()) == _ints(b.episode_tensor()) == [0, 5, 0, 1, 0]
    assert _ints(a.reset_tensor()) == [0] * W


def test_episode_length():
    """set_episode_length(4) before any step.  With t the 0-based index of a
    step, after step t every world's episode_step is t % 4 + 1 (1, 2, 3, 4, 1,
    ...) and its episode t // 4: the step with index 4 finds episode_step == 4
    at its start, resets the world to episode 1 and steps it, so the step that
    resets counts as the new episode's first.  The same in both modes."""
    W = 3
    mgr, twin = _cpu(W), _cpu(W)
    mgr.set_episode_length(4)
    assert mgr.schedule_info()["episodes_armed"]
    for t in range(11):
        if t and t % 4 == 0:
            twin.reset_worlds(range(W))
        _drive((mgr, twin), t)
        assert _ints(mgr.episode_step_tensor()) == [t % 4 + 1] * W, t
        assert _ints(mgr.episode_tensor()) == [t // 4] * W, t
        assert _ints(twin.episode_tensor()) == [t // 4] * W, t
        _same(mgr, twin, f"step {t}")
    # the constructor keyword is the same switch
    kw = _cpu(W, episode_length=4)
    ref = _cpu(W)
    ref.set_episode_length(4)
    # a manual reset of world 1 at the step with index 2 staggers only world 1
    for t in range(9):
        if t == 2:
            for m in (kw, ref):
                m.reset_worlds([1])
        _drive((kw, ref), t)
        _same(kw, ref, f"keyword, step {t}")
        want = [t % 4 + 1, (t - 2) % 4 + 1 if t >= 2 else t + 1, t % 4 + 1]
        assert _ints(kw.episode_step_tensor()) == want, t
        assert _ints(kw.episode_tensor()) == [t // 4, (1 + (t - 2) // 4) if t >= 2 else 0, t // 4], t


def test_checkpoint():
    W = 4
    plain, touched = _cpu(W), _cpu(W)
    touched.reset_worlds([])   # a no-op: the manager stays unarmed
    for t in range(3):
        _drive((plain, touched), t)
    # an unarmed manager's blob is the one it always was
    blob = plain.save_checkpoint()
    assert np.array_equal(blob, touched.save_checkpoint())
    armed, twin = _cpu(W), _cpu(W)
    for m in (armed, twin):
        m.set_episode_length(5)
    for t in range(3):
        _drive((armed, twin), t)
    for m in (armed, twin):
        m.reset_worlds([0])
        m.step()
        m.reset_worlds([2], [9])   # pending across the checkpoint
    ablob = armed.save_checkpoint()
    assert ablob.size > blob.size
    other = _cpu(W)   # unarmed: the blob arms it
    other.load_checkpoint(ablob.tobytes())
    assert other.schedule_info()["episodes_armed"]
    for m in (other, twin):
        assert _ints(m.episode_tensor()) == [1, 0, 0, 0]
        assert _ints(m.episode_step_tensor()) == [1, 4, 4, 4]
        assert _ints(m.reset_tensor()) == [0, 0, 11, 0]
    for t in range(3, 7):
        _drive((other, twin), t)
        _same(other, twin, f"after the load, step {t}")
    # (world 0 is 5 steps into episode 1; worlds 1 and 3 expired once, world 2 took its flag)
    assert _ints(other.episode_tensor()) == _ints(twin.episode_tensor()) == [1, 1, 9, 1]
    assert _ints(other.episode_step_tensor()) == [5, 3, 4, 3]
    assert np.array_equal(other.save_checkpoint(), twin.save_checkpoint())
    # an unarmed manager's blob into an armed one: the three arrays zeroed, the
    # armed state and the episode length kept
    twin.reset_worlds([3])
    twin.load_checkpoint(blob.tobytes())
    assert twin.schedule_info()["episodes_armed"]
    assert _ints(twin.episode_tensor()) == _ints(twin.episode_step_tensor()) == _ints(twin.reset_tensor()) == [0] * W
    for t in range(5):
        twin.step()
    assert _ints(twin.episode_step_tensor()) == [5] * W
    twin.step()
    assert _ints(twin.episode_tensor()) == [1] * W   # the length (5) survived


def test_growth_shards_ghost():
    W = 4
    a, b = _cpu(W), _cpu(W, agent_capacity=256)
    for t in range(3):
        _drive((a, b), t)
    for m in (a, b):
        m.reset_worlds([1], [4])
        m.step()
        m.reset_worlds([2])
    a.grow_capacity(256)
    for m in (a, b):
        assert _ints(m.episode_tensor()) == [0, 4, 0, 0]
        assert _ints(m.episode_step_tensor()) == [4, 1, 4, 4]
        assert _ints(m.reset_tensor()) == [0, 0, 1, 0]
    for t in range(3, 7):
        _drive((a, b), t)
        _same(a, b, f"after the growth, step {t}")
    assert _ints(a.episode_tensor()) == [0, 4, 1, 0]

    # two shards of a 7-world run against one manager; world 4 is the first
    # shard's ghost (its last world's species-4 reward reads world 4's row)
    one = _cpu(7)
    s0, s1 = _cpu(4, shard_ghost=True), _cpu(3, world_offset=4)
    for m in (one, s0, s1):
        m.set_episode_length(5)
    for t in range(12):
        if t == 3:
            for m in (one, s0, s1):
                m.reset_worlds([3, 4], [2, 6])
        _drive((one, s0, s1), t)
        n0, n1 = s0.num_agents(), s1.num_agents()
        assert n0 + n1 == one.num_agents()
        # per world, in slot order: the shards' worlds against the single manager's
        for w in range(7):
            m, lw = (s0, w) if w < 4 else (s1, w - 4)
            ra, rb = _world_rows(m, lw), _world_rows(one, w)
            for name, _ in COLUMNS:
                x = getattr(m, name)(False).to_torch().cpu().numpy()[ra]
                y = getattr(one, name)(False).to_torch().cpu().numpy()[rb]
                assert np.array_equal(np.ascontiguousarray(x).view(np.uint8),
                                      np.ascontiguousarray(y).view(np.uint8)), (t, w, name)
        assert _ints(s0.episode_tensor()) + _ints(s1.episode_tensor()) == _ints(one.episode_tensor()), t
        assert _ints(s0.episode_step_tensor()) + _ints(s1.episode_step_tensor()) == _ints(one.episode_step_tensor()), t
    assert _ints(one.episode_tensor())[3:5] == [3, 7]


def test_refusals_and_no_ops():
    W = 4
    mgr = _cpu(W)
    plain = _cpu(W)
    with pytest.raises(ValueError):
        mgr.reset_worlds([0, 1], [0])
    with pytest.raises(RuntimeError):
        mgr.reset_worlds([0], [2 ** 31 - 2])
    mgr.reset_worlds([])
    mgr.reset_worlds([], [])
    assert not mgr.schedule_info()["episodes_armed"]
    assert np.array_equal(mgr.save_checkpoint(), plain.save_checkpoint())
    assert _ints(mgr.episode_step_tensor()) == [0] * W   # (does not arm)
    mgr.step()
    assert _ints(mgr.episode_step_tensor()) == [1] * W
    assert not mgr.schedule_info()["episodes_armed"]
    mgr.reset_worlds([0], [2 ** 31 - 3])   # the largest episode
    assert mgr.schedule_info()["episodes_armed"]
    mgr.step()
    assert _ints(mgr.episode_tensor()) == [2 ** 31 - 3, 0, 0, 0]
    assert _ints(mgr.episode_step_tensor()) == [1, 2, 2, 2]
    # indices outside the manager's worlds are another rank's
    mgr.reset_worlds([4, 100])
    mgr.step()
    assert _ints(mgr.episode_tensor()) == [2 ** 31 - 3, 0, 0, 0]


def test_slim_learner_records_of_reset_rows():
    """Reset rows have provenance -1, so the learner rank's rebuild yields
    zeros for them."""
    W = 3
    mgr = _cpu(W)
    for t in range(3):
        _drive((mgr,), t)
    mgr.reset_worlds([1])
    mgr.step()
    rec = mgr.pack_learner(slim=True)
    src = np.ascontiguousarray(rec.cpu().numpy())[:, 60:64].copy().view(np.int32).reshape(-1)
    rows = _world_rows(mgr, 1)
    assert len(rows) >= A and (src[rows] == -1).all()
    assert (mgr.action_tensor().to_torch().numpy()[rows] == 0).all()
    assert (mgr.hidden_state_tensor(True).to_torch().numpy()[rows] == 0).all()
