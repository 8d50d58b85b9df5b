"""The rasteriser on the device (render_kernel of csrc/mbots_kernels.hip): HIP
mode equals CPU mode bitwise in all three outputs -- stepped worlds at every
scale (also against tests/render_ref.py at scales 1 and 4), the directed seam
scenes, worlds of 300 and of 4096 agents (more than one 256-slot pass) -- and
the call's stream ordering: a queued render reads the state it was enqueued
behind, whatever steps follow it, and it is refused under graph capture.  The
CPU mode is held against the numpy restatement in tests/test_render_cpu.py."""
import numpy as np
import pytest
import torch

import render_ref as rr
import render_scenes as rs

pytestmark = pytest.mark.gpu

HIP, CPU = "hip", "cpu"


def _both(build, *args, **kw):
    return build(HIP, *args, **kw), build(CPU, *args, **kw)


@pytest.fixture(scope="module")
def stepped():
    return _both(rs.stepped_manager)


@pytest.mark.parametrize("scale", rs.SCALES)
def test_stepped_worlds_equal_cpu_mode(stepped, scale):
    mh, mc = stepped
    got = rs.rendered(mh, None, scale)
    rs.assert_same(got, rs.rendered(mc, None, scale), f"stepped scale {scale}")
    assert got["cls"].max() >= 8 and (got["cls"] == 2).any()
    if scale in (1, 4):
        rs.assert_same(got, rr.render_all(mh, range(8), scale), f"stepped against the reference, scale {scale}")
    # a list (uploaded) and a single output give the same bytes
    only = mh.render_worlds([6, 0, 6], scale, rgb=False, slot=True)
    assert set(only) == {"slot"} and np.array_equal(only["slot"].cpu().numpy(), got["slot"][[6, 0, 6]])


@pytest.fixture(scope="module")
def seam():
    return _both(rs.seam_manager)


@pytest.mark.parametrize("scale", rs.SCALES)
def test_seam_scenes_equal_cpu_mode(seam, scale):
    mh, mc = seam
    got = rs.rendered(mh, [0, 1, 2, 3], scale)
    rs.assert_same(got, rs.rendered(mc, [0, 1, 2, 3], scale), f"seams scale {scale}")
    assert len(np.unique(got["slot"][0])) >= rs.SEAM_AGENTS - 8 and (got["cls"][2] == 2).sum() >= 22 * scale * scale


def test_special_cases_equal_cpu_mode():
    (mh, lo, hi), (mc, _, _) = _both(rs.special_manager)
    for scale in rs.SCALES:
        got = rs.rendered(mh, [0, 1], scale)
        rs.assert_same(got, rs.rendered(mc, [0, 1], scale), f"special scale {scale}")
        assert (got["slot"][0] == lo).any() and not (got["slot"][0] == hi).any()


def test_more_agents_than_one_pass_equal_cpu_mode():
    """300 agents in 512 slots: two passes of render_scenes.STAGE = 256 slots."""
    mh, mc = _both(rs.big_manager)
    for scale in (1, 4):
        got = rs.rendered(mh, [0, 1], scale)
        rs.assert_same(got, rs.rendered(mc, [0, 1], scale), f"300 agents scale {scale}")
    assert got["slot"].max() >= rs.STAGE
    for m in (mh, mc):
        for t in range(3):
            m.write_synthetic_actions(1234, t, True)
            m.step()
    for scale in (2, 8):
        rs.assert_same(rs.rendered(mh, [1, 0], scale), rs.rendered(mc, [1, 0], scale), f"300 agents stepped, scale {scale}")


def test_4096_slots_equal_cpu_mode():
    """One world of 4096 agents in a 4096-slot manager: 16 passes."""
    mh, mc = _both(rs.make, 1, 3, 4096, agent_capacity=4096)
    for scale in (1, 2):
        got = rs.rendered(mh, [0], scale)
        rs.assert_same(got, rs.rendered(mc, [0], scale), f"4096 agents scale {scale}")
    assert got["slot"].max() >= 4096 - rs.STAGE            # an agent of the last pass shows


def test_lifecycle_equals_reference():
    mgr = rs.stepped_manager(HIP, worlds=4, seed=7, agents=16, steps=5)
    blob = mgr.save_checkpoint()
    mgr.reset_worlds([2])
    mgr.write_synthetic_actions(1234, 5, True)
    mgr.step()
    rs.assert_equals_ref(mgr, [0, 1, 2, 3], 2, "after a reset")
    mgr.load_checkpoint(blob)
    rs.assert_equals_ref(mgr, [2, 3], 2, "after a load")
    mgr.grow_capacity(256)
    rs.assert_equals_ref(mgr, [2, 3], 4, "after growth")


def test_a_queued_render_reads_the_state_it_followed():
    """16400 worlds (the swapped schedule: K1 runs on the manager's internal
    stream): a render enqueued behind step 3, followed at once by two more
    steps with no synchronisation, shows the worlds as they stood after step 3."""
    W, worlds = 16400, [0, 8191, 16399]
    mgr = rs.make(HIP, W, 21, 16)
    assert mgr.schedule_info()["swap"]
    for t in range(3):
        mgr.write_synthetic_actions(1234, t, True)
        mgr.step()
    states = [mgr.world_state(w) for w in worlds]          # (synchronises)
    out = mgr.render_worlds(worlds, 2, rgb=True, cls=True, slot=True)
    for t in (3, 4):
        mgr.write_synthetic_actions(1234, t, True)
        mgr.step()
    torch.cuda.synchronize()
    assert mgr.schedule_info()["steps"] == 5
    refs = [rr.render_ref(s, 2) for s in states]
    want = {k: np.stack([r[i] for r in refs]) for i, k in enumerate(rs.KEYS)}
    rs.assert_same({k: out[k].cpu().numpy() for k in rs.KEYS}, want, "queued render")
    # ... and the worlds have moved on since
    assert any(not np.array_equal(mgr.world_state(w)["position"], s["position"]) for w, s in zip(worlds, states))


def test_a_render_leaves_the_step_as_it_was():
    """A manager that renders launches, per kernel class of the step, what one
    that never does launches, under the same schedule."""
    counts = []
    for render in (False, True):
        mgr = rs.make(HIP, 64, 9, 16)
        mgr.enable_kernel_timing(True)
        for t in range(3):
            mgr.write_synthetic_actions(1234, t, False)
            mgr.step()
            if render:
                mgr.render_worlds([1, 2], 1, cls=True)
        counts.append(({k: v[1] for k, v in mgr.kernel_times().items()}, mgr.schedule_info()))
    assert counts[0] == counts[1]


def test_errors_leave_device_outputs_untouched():
    mgr = rs.make(HIP, 3, 1, 8)
    out = {"cls": torch.full((1, 96, 128), 0xAB, dtype=torch.uint8, device=mgr.device)}
    with pytest.raises(RuntimeError, match=r"status -4"):
        mgr.render_worlds([3], 1, out=out)
    bad = {"cls": torch.full((1, 288, 384), 0xAB, dtype=torch.uint8, device=mgr.device)}
    with pytest.raises(RuntimeError, match="scale"):
        mgr.render_worlds([0], 3, out=bad)
    torch.cuda.synchronize()
    assert bool((out["cls"] == 0xAB).all()) and bool((bad["cls"] == 0xAB).all())


def test_render_is_refused_under_capture():
    """The world list is uploaded from the host: refused while the stream is
    captured, with the capture and the manager left usable."""
    mgr = rs.make(HIP, 64, 9, 16)
    before = rs.rendered(mgr, [5], 1)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        mgr.write_synthetic_actions(1234, 0, False)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            with pytest.raises(RuntimeError, match="cannot be captured"):
                mgr.render_worlds([5], 1)
            with pytest.raises(RuntimeError, match="cannot be captured"):
                mgr.render_worlds(None, 1)
            for t in (0, 1):
                mgr.step()
                mgr.write_synthetic_actions(1234, t + 1, False)
            mgr.join()
        g.replay()
        torch.cuda.synchronize()
        after = rs.assert_equals_ref(mgr, [5], 1, "after the replay")
    assert not np.array_equal(after["slot"], before["slot"])
