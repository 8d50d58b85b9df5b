"""The trajectory window's sequences, batches and gathers on the device (the
count / scan / walk kernels, the batch scatter, traj_batch_obs_kernel and
traj_gather_kernel of csrc/mbots_kernels.hip): every body of
tests/test_seq_cpu.py runs in HIP mode against the numpy restatement
(tests/seq_ref.py), and its outcome equals the CPU mode's bitwise.  Device
only: the whole sequence of calls on side streams, a batch enqueued before
later steps and read after them, and the refusals under stream capture."""
import pytest
import torch

import seq_ref as sr
import traj_util as tu

pytestmark = pytest.mark.gpu


def _both(body, *args):
    got = body(sr.hip, *args)
    sr.same_tree(got, body(sr.cpu, *args), body.__name__)
    return got


def test_sequences_equal_the_restatement_and_cpu_mode():
    _both(sr.numbering_scenarios)


@pytest.mark.parametrize("fixd", [False, True])
@pytest.mark.parametrize("reset", [False, True])
def test_batches_equal_the_restatement_and_cpu_mode(reset, fixd):
    """The full batch runs the 16-B store path, the pieces the partial tile;
    the records are 64 B (fixd off) and 96 B."""
    _both(sr.batches_scenario, reset, fixd)


@pytest.mark.parametrize("fixd", [False, True])
def test_obs_equal_the_oracle(fixd):
    _both(sr.oracle_obs_scenario, fixd)


def test_gather_equals_numpy_indexing():
    _both(sr.gather_scenario)


def test_ring_wrap_keeps_the_kept_tables_records():
    _both(sr.ring_scenario)


def test_growth_leaves_the_records_intact():
    _both(sr.growth_scenario)


def test_errors_and_a_flagless_window():
    _both(sr.errors_scenario)


def test_two_shards_equal_one_manager():
    _both(sr.shards_scenario)


def test_unaligned_obs_takes_the_scalar_stores():
    """An obs tensor 4 bytes off a 16-B boundary: the same bits."""
    mh, wh = sr.run20(sr.hip)
    S, L = sr.numbered(wh)[1], wh.num_tables
    aligned = sr.np_(wh.batch(keys=["obs"])["obs"])
    buf = torch.zeros(L * S * 69 + 4, device=mh.device)
    out = buf[1:1 + L * S * 69].view(L, S, 69)
    assert out.data_ptr() % 16 == 4
    wh.batch(out={"obs": out})
    sr.same(sr.np_(out), aligned, "unaligned")
    assert not sr.np_(buf)[0] and not sr.np_(buf)[-3:].any()


def test_side_streams_and_a_batch_read_after_later_steps():
    """The pushes (records and state behind their own waits, no accessor in
    between) on one side stream, compute / sequences / batch / gather on another,
    then steps enqueued behind the batch before anything is read."""
    mc, wc = sr.run20(sr.cpu)
    res = sr.numbered(wc)[0]
    expected = sr.to_np(wc.batch())
    logp = [torch.full((r, 1), float(t)) + torch.arange(r).reshape(-1, 1) for t, r in enumerate(res["rows"])]
    expected_g = sr.np_(wc.gather(logp))
    mgr = sr.hip()
    win = mgr.trajectory_window(tu.STEPS + 1, sr.MAX_ROWS, **sr.ALL)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        sr.write_memory(mgr, 98)                    # (as run20 does before table 0)
        tu.run_window(mgr, with_values=True, win=win, before_step=sr.write_memory)
    dev = [x.to(mgr.device) for x in logp]
    torch.cuda.current_stream().synchronize()
    with torch.cuda.stream(s2):
        win.compute(*sr.PARAMS)
        S = win.sequences()
        got = win.batch()
        got_g = win.gather(dev)
    with torch.cuda.stream(s1):
        for t in range(3):
            mgr.write_actions(tu.breed_shoot(mgr.num_agents(), 20 + t).to(mgr.device))
            mgr.step()
    torch.cuda.synchronize()
    assert S == len(expected["len"])
    sr.same_dict(sr.to_np(got), expected, "side streams")
    sr.same(sr.np_(got_g), expected_g, "side streams gather")


def test_sequences_and_batches_are_refused_under_capture():
    mgr = sr.hip(64, tu.A)
    win = mgr.trajectory_window(4, 4096, **sr.ALL)
    win.push()
    win.compute(0.99)
    S = win.sequences()
    out = {"len": torch.zeros(S, dtype=torch.int32, device=mgr.device)}
    tab = [torch.zeros((S, 1), device=mgr.device)]
    gout = torch.zeros((1, S, 1), device=mgr.device)
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        mgr.write_synthetic_actions(1234, 0, False)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s, capture_error_mode="relaxed"):
            for call in (win.sequences, lambda: win.batch(out=out), lambda: win.gather(tab, out=gout)):
                with pytest.raises(RuntimeError, match="cannot be captured"):
                    call()
            for t in (0, 1):
                mgr.step()
                mgr.write_synthetic_actions(1234, t + 1, False)
            mgr.join()
        g.replay()
        torch.cuda.synchronize()
        assert win.sequences() == S                                         # the window is still usable
        win.batch(out=out)
        assert (sr.np_(out["len"]) == 1).all()


@pytest.mark.parametrize("W", [2049, 8200])
def test_the_other_schedules_equal_cpu_mode(W):
    """Above the K1-finder mode (2049 worlds: the push's wait for the sensor
    crosses queues) and on the swapped schedule (8200 worlds: K1 and K2 run on
    the manager's internal stream), the recording pushes with no accessor in
    between, one world in three reset mid-window: every batch key equals the CPU
    mode's, which the smaller scenarios hold against the restatement."""
    resets = list(range(0, W, 3))

    def before(m, t):
        sr.write_memory(m, t)
        if t == 1:
            m.reset_worlds(resets)

    def run(make):
        mgr = make(W, tu.A)
        mgr.write_synthetic_actions(1234, 99, False)
        sr.write_memory(mgr, 99)                    # (so table 0 holds a recurrent state)
        mgr.step()
        win = mgr.trajectory_window(4, 3 * W * tu.A, **sr.ALL)
        tu.run_window(mgr, steps=3, with_values=True, win=win, actions=None, before_step=before)
        win.compute(*sr.PARAMS)
        return mgr, win.sequences(), sr.to_np(win.batch())
    (mh, Sh, bh), (mc, Sc, bc) = run(sr.hip), run(sr.cpu)
    assert not mh.schedule_info()["k1_finder"] and mh.schedule_info()["swap"] == (W > 8192)
    assert Sh == Sc >= W * tu.A and (bh["end"] == 2).sum() >= len(resets) * tu.A
    sr.same_dict(bh, bc, W)
    assert bh["obs"].any() and bh["action_in"].any() and bh["hidden0"].any()
