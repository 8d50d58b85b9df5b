"""Per-world resets and episodes on the device (reset_worlds_kernel and its
place in mbots_step).  Where the whole manager is reset the reference is the
oracle; otherwise a CPU-mode twin taking the same calls, every current and Prev
column bitwise -- and, in the value-fork, swapped-schedule and captured-graph
cases, an oracle taking them too (it restates resets on its own: see
tests/test_reset_oracle.py, which holds the directed cases against it).
tests/test_reset_cpu.py holds the semantics; here each case
is a schedule the reset pass has to fit: the K1-finder mode (whose K1 does not
wait for the last sensor; the pass must), the value forks just past it, the
swapped schedule, mixed capacity classes (the class list is rebuilt after the
pass), a captured graph, the shard ghost and a growth."""
import numpy as np
import pytest
import torch

import pyoracle
from reset_util import episode_errors
from simpair import COLUMNS, compare
from test_grow_capacity import _breed_heavy

SEED, A = 69, 32

pytestmark = pytest.mark.gpu


def _hip(W, **kw):
    import madrona_bots as mb
    return mb.SimManager(0, W, SEED, A, **kw)


def _cpu(W, **kw):
    import madrona_bots as mb
    return mb.SimManager(0, W, SEED, A, exec_mode="cpu", **kw)


def _drive(sims, t):
    for s in sims:
        s.step()
        s.shift_observations()
        s.write_synthetic_actions(1234, t, True)


def _same(a, b, where):
    """Two managers (either execution mode): every exported column, current
    and Prev, bitwise, and the episode exports."""
    assert a.num_agents() == b.num_agents(), where
    assert torch.equal(a.species_count_tensor().to_torch().cpu(), b.species_count_tensor().to_torch().cpu()), where
    for name in [c[0] for c in COLUMNS] + ["depth_tensor"]:
        for prev in (False, True):
            x = getattr(a, name)(prev).to_torch().cpu()
            y = getattr(b, name)(prev).to_torch().cpu()
            assert x.shape == y.shape, (where, name, prev)
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (where, name, prev)
    for name in ("episode_tensor", "episode_step_tensor", "reset_tensor"):
        assert torch.equal(getattr(a, name)().to_torch().cpu(), getattr(b, name)().to_torch().cpu()), (where, name)


def _check(mgr, orc, where):
    errs = compare(mgr, orc, where, prev_too=True)
    assert not errs, errs[:5]


def _check_episodes(mgr, orc, where):
    """_check and the three episode arrays: an oracle that took the same calls."""
    _check(mgr, orc, where)
    errs = episode_errors(mgr, orc, where)
    assert not errs, errs


def _ints(t):
    return t.to_torch().cpu().numpy().reshape(-1).tolist()


def test_k1_finder_mode_all_and_partial():
    """W = 6 at 128 slots: the K1-finder mode, a partial K1 block and a partial
    4-world block.  Everything reset to episode 0 equals a fresh oracle; then a
    partial reset against the CPU twin."""
    W = 6
    mgr, twin = _hip(W), _cpu(W)
    assert mgr.schedule_info()["k1_finder"] and not mgr.schedule_info()["episodes_armed"]
    for t in range(6):
        _drive((mgr, twin), t)
    for m in (mgr, twin):
        m.reset_worlds(range(W), episodes=[0] * W)
    assert mgr.schedule_info()["episodes_armed"]
    orc = pyoracle.OracleSim(W, SEED, A)
    for t in range(6, 12):
        for s in (mgr, twin, orc):
            s.step()
        _check(mgr, orc, f"step {t}")
        for s in (mgr, twin, orc):
            s.shift_observations()
        _check(mgr, orc, f"shift {t}")
        for s in (mgr, twin, orc):
            s.write_synthetic_actions(1234, t, True)
    _same(mgr, twin, "after the full reset")
    for m in (mgr, twin):
        m.reset_worlds([1, 3], episodes=[0, 0])
    for t in range(12, 20):
        _drive((mgr, twin), t)
        _same(mgr, twin, f"partial, step {t}")
    assert _ints(mgr.episode_step_tensor()) == [14, 8, 14, 8, 14, 14]


def test_value_forks_scan_tile_edges():
    """W = 2052, just past the K1-finder limit (sensor finders, value forks):
    the scan-tile edge and the last world."""
    W = 2052
    mgr, twin = _hip(W), _cpu(W)
    orc = pyoracle.OracleSim(W, SEED, A, num_threads=8)
    assert not mgr.schedule_info()["k1_finder"]
    for t in range(6):
        _drive((mgr, twin, orc), t)
    for m in (mgr, twin, orc):
        m.reset_worlds([0, 1023, 1024, 2051])
    for t in range(6, 12):
        _drive((mgr, twin, orc), t)
        if t in (6, 8, 11):
            _same(mgr, twin, f"step {t}")
            _check_episodes(mgr, orc, f"step {t}")
    want = [0] * W
    for w in (0, 1023, 1024, 2051):
        want[w] = 1
    assert _ints(mgr.episode_tensor()) == want


def test_swapped_schedule_flags_written_by_torch():
    """W = 8200: K1 runs on the internal stream; the flags are written by torch
    on the caller's stream."""
    W = 8200
    mgr, twin = _hip(W), _cpu(W)
    orc = pyoracle.OracleSim(W, SEED, A, num_threads=8)
    for t in range(3):
        _drive((mgr, twin, orc), t)
    idx = [0, 4100, 8199]
    mgr.reset_tensor().to_torch()[idx] = 1
    twin.reset_tensor().to_torch()[idx] = 1
    orc.reset_flags()[idx] = 1
    for t in range(3, 7):
        _drive((mgr, twin, orc), t)
        if t in (3, 6):
            _same(mgr, twin, f"step {t} (swap {mgr.schedule_info()['swap']})")
            _check_episodes(mgr, orc, f"step {t}")
    assert _ints(mgr.reset_tensor()) == [0] * W
    assert [_ints(mgr.episode_tensor())[w] for w in idx] == [1, 1, 1]


def test_mixed_classes_no_double_claim():
    """agent_capacity 512, 8 worlds: after 29 breed-heavy steps every world is
    in the K1 class list; worlds 4 and 5 reset to 32 agents must leave it (the
    128-slot K1 claims them by their live population)."""
    W = 8
    mgr, twin = _hip(W, agent_capacity=512), _cpu(W, agent_capacity=512)
    assert mgr.schedule_info()["mixed_classes"]

    def drive(t):
        for m in (mgr, twin):
            m.step()
            m.shift_observations()
            m.action_tensor().to_torch().copy_(_breed_heavy(m.num_agents(), t).to(m.device))

    for t in range(1, 30):
        drive(t)
    pops = mgr.species_count_tensor().to_torch().sum(1).tolist()
    assert pops == [146, 111, 132, 146, 161, 88, 156, 116]
    _same(mgr, twin, "before the reset")
    for m in (mgr, twin):
        m.reset_worlds([4, 5], [0, 0])
    for t in range(30, 36):
        drive(t)
        _same(mgr, twin, f"step {t}")
    assert mgr.overflow() == twin.overflow() == 0


def test_graph_capture():
    """An armed manager's steps are capturable; the flags are read at replay
    time, so a torch write between replays resets worlds."""
    W = 64
    mgr, twin = _hip(W), _cpu(W)
    orc = pyoracle.OracleSim(W, SEED, A, num_threads=4)
    for t in (0, 1, 2, 3):   # (the steps before the capture and the first replay)
        _drive((orc,), t)
    orc.reset_flags()[[5, 40]] = 1
    for t in (2, 3):         # (the second replay)
        _drive((orc,), t)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for t in range(2):
            _drive((mgr, twin), t)
        flags = mgr.reset_tensor().to_torch()   # (arms the manager)
        twin.reset_tensor()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            with pytest.raises(RuntimeError, match="cannot be captured"):
                mgr.reset_worlds([1])
            _drive((mgr,), 2)
            _drive((mgr,), 3)
            mgr.join()
        g.replay()
        for t in (2, 3):
            _drive((twin,), t)
        torch.cuda.synchronize()
        # (between replays only columns without deferred host-side state are
        # read: a replay repeats the moves recorded at capture, not the ones
        # an accessor has made since)
        assert mgr.num_agents() == twin.num_agents()
        for name in ("position_tensor", "health_tensor", "species_tensor", "episode_step_tensor"):
            assert torch.equal(getattr(mgr, name)().to_torch().cpu(), getattr(twin, name)().to_torch()), name
        flags[[5, 40]] = 1
        twin.reset_worlds([5, 40])
        g.replay()
        for t in (2, 3):
            _drive((twin,), t)
        torch.cuda.synchronize()
        _same(mgr, twin, "second replay")
        _check_episodes(mgr, orc, "second replay")
        assert _ints(mgr.episode_tensor())[5] == _ints(mgr.episode_tensor())[40] == 1
        assert _ints(mgr.episode_step_tensor())[5] == 2


def test_ghost_growth_checkpoint():
    """W = 37 with the shard ghost (global world 37): the ghost and world 36
    reset, an episode length running, then a growth on the device and an armed
    checkpoint round trip."""
    W = 37
    mgr, twin = _hip(W, shard_ghost=True), _cpu(W, shard_ghost=True)
    for m in (mgr, twin):
        m.set_episode_length(7)
    for t in range(4):
        _drive((mgr, twin), t)
    for m in (mgr, twin):
        m.reset_worlds([36, 37], [3, 3])
    for t in range(4, 7):
        _drive((mgr, twin), t)
        _same(mgr, twin, f"step {t}")
    for m in (mgr, twin):
        m.reset_worlds([2])   # pending across the growth
        m.grow_capacity(256)
    _same(mgr, twin, "after the growth")
    for t in range(7, 10):
        _drive((mgr, twin), t)
        _same(mgr, twin, f"step {t} at 256")
    assert _ints(mgr.episode_tensor())[36] == 3 and _ints(mgr.episode_tensor())[2] == 1
    # a version-5 blob arms the manager that loads it; an unarmed manager's is version 4
    blob = mgr.save_checkpoint()
    assert int(np.frombuffer(blob.tobytes()[8:12], np.uint32)[0]) == 5
    fresh = _hip(W, shard_ghost=True, agent_capacity=256)
    assert int(np.frombuffer(fresh.save_checkpoint().tobytes()[8:12], np.uint32)[0]) == 4
    fresh.load_checkpoint(blob.tobytes())
    assert fresh.schedule_info()["episodes_armed"]
    for t in range(10, 13):
        _drive((fresh, twin), t)
        _same(fresh, twin, f"after the load, step {t}")
