"""Capacity growth in place (mbots_grow_capacity / mbots_set_auto_capacity;
SimManager.grow_capacity, auto_grow=True).

After a growth the manager must be indistinguishable from a fresh manager of
the new capacity that loaded its checkpoint -- and so from an oracle that
never drops an agent -- bitwise, on every column after every later step.  The
CPU tests run the host re-layout (cpu::Sim::grow), the GPU tests the
device-side move (grow_slots_kernel and the device-to-device copies)."""
import numpy as np
import pytest
import torch

import pyoracle
from simpair import COLUMNS, compare


def _cpu(W, A=32, **kw):
    import madrona_bots as mb
    return mb.SimManager(0, W, 69, A, exec_mode="cpu", **kw)


def _synthetic(sims, t):
    for s in sims:
        s.write_synthetic_actions(1234, t, True)
        s.step()


def _shift(sims):
    for s in sims:
        s.shift_observations()


def _check(mgr, orc, where):
    errs = compare(mgr, orc, where)
    assert not errs, errs[:5]


def _same(a, b, where):
    """Two managers (either execution mode): every exported column, current
    and Prev, bitwise."""
    assert a.num_agents() == b.num_agents(), where
    assert torch.equal(a.species_count_tensor().to_torch().cpu(), b.species_count_tensor().to_torch().cpu()), where
    for name in [c[0] for c in COLUMNS] + ["depth_tensor"]:
        for prev in (False, True):
            x = getattr(a, name)(prev).to_torch().cpu()
            y = getattr(b, name)(prev).to_torch().cpu()
            assert x.shape == y.shape, (where, name, prev)
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (where, name, prev)


# ---------------------------------------------------------------- CPU mode --
def test_in_place_equals_hand_over_cpu():
    """grow_capacity(512) on a 128-slot manager equals a fresh 512-slot manager
    that loaded the checkpoint saved just before, and the oracle."""
    W = 16
    a = _cpu(W, agent_capacity=128)
    orc = pyoracle.OracleSim(W, 69, 32, cap=512, num_threads=4)
    for t in range(6):
        _synthetic((a, orc), t)
        _shift((a, orc))
    blob = a.save_checkpoint()
    h = a._h
    a.grow_capacity(512)
    assert a._h is h and a.agent_capacity == 512
    b = _cpu(W, agent_capacity=512)
    b.load_checkpoint(blob.tobytes())
    _same(a, b, "after the growth")
    _check(a, orc, "after the growth")
    for t in range(6, 10):
        _synthetic((a, b, orc), t)
        _check(a, orc, f"in place, step {t}")
        _check(b, orc, f"hand-over, step {t}")
        _same(a, b, f"step {t}")
        _shift((a, b, orc))
        _check(a, orc, f"in place, shift {t}")
        _same(a, b, f"shift {t}")
    assert np.array_equal(a.save_checkpoint(), b.save_checkpoint())
    assert a.overflow() == 0


def test_auto_grow_from_an_int_cpu():
    """auto_grow=True from agent_capacity=96: the largest world stays at 32
    through the second step and holds 35 after the third, so the run leaves 96
    for 128 before its fourth step (2 * 35 + 32 > 96), never drops, and stays
    the oracle's."""
    W = 8
    mgr = _cpu(W, agent_capacity=96, auto_grow=True)
    orc = pyoracle.OracleSim(W, 69, 32, cap=1024, num_threads=4)
    seen = set()
    for t in range(12):
        _synthetic((mgr, orc), t)
        seen.add(mgr.agent_capacity)
        if t == 0:
            assert mgr.agent_capacity == 96
        _check(mgr, orc, f"step {t}")
        _shift((mgr, orc))
    assert seen == {96, 128}
    assert mgr.agent_capacity == 128
    assert mgr.overflow() == orc.overflow() == 0


def test_refusals_leave_the_manager_intact_cpu():
    W = 8
    mgr = _cpu(W, agent_capacity=128)
    orc = pyoracle.OracleSim(W, 69, 32, cap=128, num_threads=4)
    t = 0
    for _ in range(3):
        _synthetic((mgr, orc), t)
        _shift((mgr, orc))
        t += 1
    for cap, raises in ((64, True), (4097, True), (128, False)):
        if raises:
            with pytest.raises(RuntimeError):
                mgr.grow_capacity(cap)
        else:
            mgr.grow_capacity(cap)
        assert mgr.agent_capacity == 128
        for _ in range(2):
            _synthetic((mgr, orc), t)
            _check(mgr, orc, f"after grow_capacity({cap}), step {t}")
            _shift((mgr, orc))
            t += 1


def test_native_auto_capacity_cpu():
    """mbots_set_auto_capacity for C callers of the CPU mode (the Python
    wrapper's CPU mode keeps its checkpoint hand-over): mbots_step grows
    first, old host views keep their storage, release_retired frees it."""
    import madrona_bots as mb
    W = 8
    mgr = _cpu(W, agent_capacity=96)
    orc = pyoracle.OracleSim(W, 69, 32, cap=1024, num_threads=4)
    mb._check(mb._lib.mbots_set_auto_capacity(mgr._h, 1))
    seen = set()
    for t in range(12):
        if mgr.agent_capacity == 96:   # (kept from the last step before the growth)
            old = mgr.position_tensor()
            before = old.to_torch().clone()
        _synthetic((mgr, orc), t)
        mgr._refresh_capacity()
        seen.add(mgr.agent_capacity)
        _check(mgr, orc, f"step {t}")
        _shift((mgr, orc))
    assert seen == {96, 128}
    assert torch.equal(old.to_torch(), before)
    assert old.to_torch().data_ptr() != mgr.position_tensor().to_torch().data_ptr()
    del old
    mgr.release_retired()
    _synthetic((mgr, orc), 12)
    _check(mgr, orc, "after release_retired")
    assert mgr.overflow() == 0


# ---------------------------------------------------------------- HIP mode --
def _breed_turning(mgr, t):
    """Every agent breeds, as in tests/test_robustness.py::_breed_all, and
    walks or turns by a seeded draw.  (_breed_all itself -- every third agent
    walking, nobody turning -- never fills a world of A = 8: the two agents of
    a species start with the same heading and never get each other into the
    finder's centre ray, so the population stays at 8 for thousands of steps.)"""
    n = mgr.num_agents()
    r = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(500 + t))
    a = torch.zeros((n, 6), dtype=torch.int32)
    a[:, 5] = 1
    a[r == 0, 0] = 1
    a[r == 1, 2] = 1
    a[r == 2, 3] = 1
    mgr.write_actions(a.to(mgr.device))


def _breed_heavy(n, step):
    """tests/test_parity_gpu.py: breed 1/2, forward 1/4, rotate 1/4."""
    g = torch.Generator().manual_seed(1000 + step)
    r = torch.randint(0, 8, (n,), generator=g)
    a = torch.zeros((n, 6), dtype=torch.int32)
    a[r < 4, 5] = 1
    a[(r >= 4) & (r < 6), 0] = 1
    a[r == 6, 2] = 1
    a[r == 7, 3] = 1
    return a


@pytest.fixture
def no_checkpoint_loads(monkeypatch):
    """Counts mbots_load_checkpoint calls: the device path never takes one."""
    import madrona_bots as mb
    calls = []
    real = mb._lib.mbots_load_checkpoint

    def counted(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(mb._lib, "mbots_load_checkpoint", counted)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("W,ghost", [(8, False), (2100, False), (37, True)])
def test_in_place_growth_on_the_device(W, ghost, no_checkpoint_loads):
    """128 -> 256 -> 512 in place: W = 8 leaves the K1-finder mode at 512,
    W = 2100 (above the K1-finder limit) becomes a mixed-class manager, W = 37
    with the shard ghost is an odd world count (the move's grid has a tail),
    compared with a CPU-mode manager taking the same path."""
    import madrona_bots as mb
    mgr = mb.SimManager(0, W, 69, 32, shard_ghost=ghost)
    if ghost:
        ref = _cpu(W, shard_ghost=True)
        check = lambda where: _same(mgr, ref, where)   # noqa: E731
    else:
        ref = pyoracle.OracleSim(W, 69, 32, cap=512, num_threads=16)
        check = lambda where: _check(mgr, ref, where)   # noqa: E731
    h = mgr._h
    assert mgr.schedule_info()["k1_finder"] == (W <= 2048)
    t = 0
    for cap, steps in ((None, 5), (256, 3), (512, 3)):
        if cap:
            mgr.grow_capacity(cap)
            if ghost:
                ref.grow_capacity(cap)
            assert mgr.agent_capacity == cap and mgr._h is h
            check(f"after grow_capacity({cap})")
            info = mgr.schedule_info()
            assert info["k1_finder"] == (W <= 2048 and cap <= 256)
            assert info["mixed_classes"] == (not info["k1_finder"])
        for _ in range(steps):
            _synthetic((mgr, ref), t)
            check(f"step {t} at {mgr.agent_capacity}")
            _shift((mgr, ref))
            check(f"shift {t} at {mgr.agent_capacity}")
            t += 1
    assert mgr.overflow() == 0
    assert not no_checkpoint_loads


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore::madrona_bots.CapacityWarning")
def test_capacities_not_multiples_of_four_and_full_rows():
    """30 -> 77 -> 128 slots (the move's scalar path) from a manager with a full
    world (30 of 30 slots, births dropped): in place equals the hand-over and
    the CPU mode."""
    import madrona_bots as mb
    W, A = 5, 8
    a = mb.SimManager(0, W, 69, A, agent_capacity=30)
    c = _cpu(W, A, agent_capacity=30)
    # (the drops are counted, not the subject: their late CapacityWarning is not awaited)
    for t in range(60):
        for m in (a, c):
            _breed_turning(m, t)
            m.step()
        _same(a, c, "breeding")
        full = int(a.species_count_tensor().to_torch().sum(1).max()) == 30
        _shift((a, c))
        if full and a.overflow() > 0:
            break
    assert full and a.overflow() == c.overflow() > 0
    blob = a.save_checkpoint()
    a.grow_capacity(77)
    c.grow_capacity(77)
    b = mb.SimManager(0, W, 69, A, agent_capacity=77)
    b.load_checkpoint(blob.tobytes())
    _same(a, b, "after the growth")
    _same(a, c, "after the growth (cpu)")
    for t in range(6):
        _synthetic((a, b, c), t)
        _same(a, b, f"step {t}")
        _same(a, c, f"step {t} (cpu)")
        _shift((a, b, c))
        _same(a, b, f"shift {t}")
        _same(a, c, f"shift {t} (cpu)")
    a.grow_capacity(128)
    c.grow_capacity(128)
    for t in range(6, 9):
        _synthetic((a, c), t)
        _same(a, c, f"step {t} at 128")
        _shift((a, c))
        _same(a, c, f"shift {t} at 128")
    assert a.overflow() == c.overflow()


@pytest.mark.gpu
def test_through_every_class_on_the_device(no_checkpoint_loads):
    """agent_capacity="auto" under the breed-heavy stream: 2 n + 32 passes 128,
    256, 512 and 1024 after steps 12, 27, 46 and 73 and the largest world holds
    1364 agents after 130 steps -- through 2048 into 4096 with nothing dropped."""
    import madrona_bots as mb
    W = 2
    mgr = mb.SimManager(0, W, 69, 32, agent_capacity="auto")
    orc = pyoracle.OracleSim(W, 69, 32, cap=4096, num_threads=16)
    h = mgr._h
    seen = {mgr.agent_capacity}
    for t in range(130):
        a = _breed_heavy(mgr.num_agents(), t)
        mgr.action_tensor(False).to_torch().copy_(a.to(mgr.device))
        orc.column(pyoracle.COL_ACTION)[:] = a.numpy()
        cap = mgr.agent_capacity
        mgr.step()
        orc.step()
        seen.add(mgr.agent_capacity)
        if mgr.agent_capacity != cap or t % 10 == 9:
            _check(mgr, orc, f"step {t} cap {mgr.agent_capacity}")
        mgr.shift_observations()
        orc.shift_observations()
    _check(mgr, orc, "the end")
    assert {128, 256, 512, 1024, 2048, 4096} <= seen
    assert int(mgr.species_count_tensor().to_torch().sum(1).max()) == 1364
    assert mgr._h is h and not no_checkpoint_loads
    assert mgr.overflow() == 0 and orc.overflow() == 0


@pytest.mark.gpu
def test_old_views_slim_records_counters():
    import madrona_bots as mb
    mgr = mb.SimManager(0, 4, 69, 32)
    mgr.enable_kernel_timing(True)
    mgr.write_synthetic_actions(1234, 0, True)
    mgr.step()
    old = mgr.position_tensor()
    before = old.to_torch().clone()
    slim = mgr.pack_learner(slim=True).clone()
    steps0 = mgr.agent_steps()
    launches0 = mgr.kernel_times()["world_step"][1]
    assert launches0 == 1
    mgr.grow_capacity(256)
    assert torch.equal(mgr.pack_learner(slim=True), slim)
    assert torch.equal(old.to_torch(), before)
    assert torch.equal(mgr.position_tensor().to_torch(), before)
    assert mgr.agent_steps() == steps0
    mgr.shift_observations()
    mgr.write_synthetic_actions(1234, 1, True)
    mgr.step()
    assert torch.equal(old.to_torch(), before)
    assert old.to_torch().data_ptr() != mgr.position_tensor().to_torch().data_ptr()
    assert mgr.kernel_times()["world_step"][1] == launches0 + 1
    assert mgr.agent_steps() > steps0
    del old
    mgr.release_retired()
    mgr.shift_observations()
    mgr.write_synthetic_actions(1234, 2, True)
    mgr.step()
    assert mgr.num_agents() >= 4 * 32


@pytest.mark.gpu
def test_graphs_pin_the_capacity():
    """A step with automatic capacity on cannot be captured; once a manager's
    steps were captured its capacity is pinned; both keep working."""
    import madrona_bots as mb
    W = 64
    auto = mb.SimManager(0, W, 69, 32, auto_grow=True)
    mgr = mb.SimManager(0, W, 69, 32)
    orc = pyoracle.OracleSim(W, 69, 32, num_threads=8)
    orc_auto = pyoracle.OracleSim(W, 69, 32, num_threads=8)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for m in (mgr, orc, auto, orc_auto):
            m.write_synthetic_actions(1234, 0)
            m.step()
            m.shift_observations()
            m.write_synthetic_actions(1234, 1)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            with pytest.raises(RuntimeError, match="automatic capacity"):
                auto.step()
            mgr.step(); mgr.shift_observations(); mgr.write_synthetic_actions(1234, 2)
            mgr.step(); mgr.shift_observations(); mgr.write_synthetic_actions(1234, 3)
            mgr.join()
    with pytest.raises(RuntimeError, match="captured graphs"):
        mgr.grow_capacity(256)
    assert mgr.agent_capacity == 128
    g.replay()
    for t in (2, 3):
        orc.step(); orc.shift_observations(); orc.write_synthetic_actions(1234, t)
    _check(mgr, orc, "after the replay")
    with torch.cuda.stream(s):
        mgr.step(); orc.step()
        _check(mgr, orc, "a step after the replay")
        auto.step(); orc_auto.step()
        _check(auto, orc_auto, "the automatic manager after its refused capture")
