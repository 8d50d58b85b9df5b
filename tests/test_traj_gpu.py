"""The trajectory window on the device (traj_push_kernel, the `next` inversion
and traj_sweep_kernel of csrc/mbots_kernels.hip): HIP mode equals CPU mode
bitwise on every view, in the scenarios of tests/test_traj_cpu.py, above the
K1-finder mode's world count, and with the push and the compute on side
streams.  The CPU mode is held against the numpy restatement there.  The
paths that file alone used to run -- the ring after clear(keep_last), a second
compute, shards with world_offset and the ghost, a truncated table, emptying on
load and set_world_state -- run here through the same bodies (traj_util)."""
import numpy as np
import pytest
import torch

import traj_util as tu

pytestmark = pytest.mark.gpu


def _both(scenario, *args, **kw):
    """The scenario on a HIP-mode and a CPU-mode manager: the two windows."""
    return scenario(tu.hip, *args, **kw), scenario(tu.cpu, *args, **kw)


def _equal(win_hip, win_cpu, params, where):
    a, b = tu.to_numpy(win_hip.compute(*params)), tu.to_numpy(win_cpu.compute(*params))
    tu.assert_same(a, b, where=where)
    assert np.array_equal(win_hip.lifelines(1).cpu().numpy(), win_cpu.lifelines(1).numpy()), where
    return a


@pytest.mark.parametrize("with_values", [False, True])
def test_plain_scenario_equals_cpu_mode(with_values):
    (mh, wh), (mc, wc) = _both(tu.scenario_plain, with_values)
    for params in tu.PARAMS:
        res = _equal(wh, wc, params, f"plain {params}")
    tu.assert_scenario(res)
    assert mh.schedule_info()["k1_finder"]


@pytest.mark.parametrize("mode", ["flag", "length"])
def test_reset_scenarios_equal_cpu_mode(mode):
    (mh, wh, marks_h), (mc, wc, marks_c) = _both(tu.scenario_reset, mode)
    assert all(np.array_equal(x, y) for x, y in zip(marks_h, marks_c))
    res = _equal(wh, wc, tu.PARAMS[1], mode)
    assert sum(int((e == 2).sum()) for e in res["end"]) >= tu.A
    for t in range(len(res["rows"]) - 1):
        assert np.array_equal(res["end"][t] == 2, marks_h[t + 1][res["world"][t]] != 0), t


def test_growth_scenario_equals_cpu_mode():
    (mh, wh, cap0), (mc, wc, _) = _both(tu.scenario_growth, "auto")
    assert cap0 == 128 and mh.agent_capacity == mc.agent_capacity == 256
    res = _equal(wh, wc, tu.PARAMS[1], "growth")
    tu.assert_scenario(res)


def test_above_the_k1_finder_mode():
    """2049 worlds x 4 tables: the schedule in which K1 reads the sensor's
    finder slots, whose provenance comes from the same export kernel through
    another stream order; one world in three is reset mid-window."""
    W = 2049
    resets = list(range(0, W, 3))

    def run(make):
        mgr = make(W)
        win = tu.run_window(mgr, steps=3, with_values=True, actions=None, max_rows=3 * W * tu.A,
                            before_step=lambda m, t: m.reset_worlds(resets) if t == 1 else None)
        return mgr, win
    (mh, wh), (mc, wc) = run(tu.hip), run(tu.cpu)
    assert not mh.schedule_info()["k1_finder"]
    res = _equal(wh, wc, tu.PARAMS[1], "2049 worlds")
    assert res["rows"][0] == W * tu.A
    cut = np.isin(res["world"][1], resets)
    assert np.array_equal(res["end"][1] == 2, cut) and cut.sum() >= len(resets) * tu.A


def test_push_and_compute_on_side_streams():
    """step() and the push right behind it on one side stream, compute on
    another: the manager's stream ordering alone puts the push after the step's
    export and the compute after the pushes."""
    mc, wc = tu.scenario_plain(tu.cpu, True)
    mgr = tu.hip()
    win = mgr.trajectory_window(tu.STEPS + 1, 4096)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    win.push(tu.values_for(mgr.num_agents(), 0).to(mgr.device))
    for t in range(tu.STEPS):
        n = mgr.num_agents()
        mgr.write_actions(tu.breed_shoot(n, t).to(mgr.device))
        with torch.cuda.stream(s1):
            mgr.step()
            v = tu.values_for(mgr.num_agents(), t + 1).to(mgr.device)
            win.push(v)
    with torch.cuda.stream(s2):
        out = win.compute(*tu.PARAMS[1])
        a = {k: ([x.clone() for x in v] if k != "rows" else v) for k, v in out.items()}
    s2.synchronize()
    tu.assert_same(tu.to_numpy(a), tu.to_numpy(wc.compute(*tu.PARAMS[1])), where="side streams")


def test_a_window_leaves_the_step_as_it_was():
    """A manager that pushes into a window launches, per kernel class of the
    step, what a manager without one launches, under the same schedule."""
    counts = []
    for with_window in (False, True):
        mgr = tu.hip()
        mgr.enable_kernel_timing(True)
        win = mgr.trajectory_window(4, 4096) if with_window else None
        for t in range(3):
            mgr.write_synthetic_actions(1234, t, False)
            mgr.step()
            if win:
                win.push()
        if win:
            win.compute(0.99)
        counts.append(({k: v[1] for k, v in mgr.kernel_times().items()}, mgr.schedule_info()))
    assert counts[0] == counts[1]


def test_push_and_compute_are_refused_under_capture():
    """Both keep host state (the table count, the row counts): refused while
    the stream is captured, with the capture and the window left usable."""
    mgr = tu.hip(64)
    win = mgr.trajectory_window(4, 4096)
    win.push()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        mgr.write_synthetic_actions(1234, 0, False)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            with pytest.raises(RuntimeError, match="cannot be captured"):
                win.push()
            with pytest.raises(RuntimeError, match="cannot be captured"):
                win.compute(0.99)
            for t in (0, 1):
                mgr.step()
                mgr.write_synthetic_actions(1234, t + 1, False)
            mgr.join()
        g.replay()
        torch.cuda.synchronize()
        assert win.num_tables == 1
        win.push()
        out = win.compute(0.99)
        assert out["rows"] == [64 * tu.A, mgr.num_agents()]


# ---- the device halves of tests/test_traj_cpu.py's window paths (the bodies
# are traj_util's, run there with the CPU-mode factory) ----------------------
def test_chained_windows_keep_every_transition_on_device():
    """The ring on the device: clear(keep_last) leaves base != 0 and the second
    window's pushes and sweeps wrap around the slots."""
    tu.chained_windows_keep_every_transition(tu.hip)


def test_compute_twice_gives_the_same_bits_on_device():
    """A second compute rewrites next / end / adv / ret in place: the third
    result equals the first, and the numpy restatement."""
    mgr, win = tu.scenario_plain(tu.hip, True)
    first = tu.to_numpy(win.compute(*tu.PARAMS[1]))
    again = tu.compute_twice_gives_the_same_bits(win, first)
    tu.assert_scenario(again)
    tu.check_against_restatement(again, [np.zeros(tu.W, np.int32)] * len(again["rows"]), *tu.PARAMS[1])


def test_two_shards_equal_one_manager_on_device():
    """world_offset in the push kernel's world column and in the sweep's mark
    lookup, and the ghost's rows left out of the pushed table."""
    tu.two_shards_equal_one_manager(tu.hip)


def test_errors_and_emptying_on_device():
    """A table of more rows than max_rows on the device: the push kernel's
    r < lim guard keeps the neighbouring slot intact, compute refuses with
    status -4 until the table has left; a load and set_world_state empty the
    window."""
    tu.errors_and_emptying(tu.hip)
