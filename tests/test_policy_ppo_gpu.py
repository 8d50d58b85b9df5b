"""GPU: PPO on the device (DESIGN.md "PPO on the device") -- the moments, loss
and gate kernels against the host path bit for bit on the CPU tests' cases,
which cross every chunk and accumulator boundary; a captured three-epoch update
whose KL gate stops one group, against the eager and the CPU-tensor updates;
and the two PPO harnesses, HIP mode against CPU mode."""
import os
import sys

import numpy as np
import pytest
import torch

import policy_ppo_ref as pr
import policy_ppo_util as u

pytestmark = pytest.mark.gpu


def same(got, want):
    for name, a, b in zip(("g_logp", "g_value", "g_entropy"), got, want):
        assert np.array_equal(pr.bits32(a), pr.bits32(b)), name
    assert np.array_equal(pr.bits64(got[3]), pr.bits64(want[3])), "stats"
    if want[4] is not None:
        assert np.array_equal(pr.bits64(got[4]), pr.bits64(want[4])), "moments"


OPTIONS = [dict(), dict(moments=False), dict(value_clip=False), dict(end=False)]


@pytest.fixture(scope="module")
def case():
    return u.ppo_case()


@pytest.fixture(scope="module")
def seqs():
    return u.seq_case()


@pytest.mark.parametrize("opt", OPTIONS, ids=("all", "no-moments", "no-value-clip", "no-end"))
def test_rows_on_the_device_equal_the_host_path(case, opt):
    import madrona_bots as mb
    host = u.run_case(mb, case, "cpu", **opt)
    dev = u.run_case(mb, case, "cuda", **opt)
    same(dev, host)
    assert dev[3][0, 4] > 0 and dev[3][2].tolist() == [0.0] * 6
    again = u.run_case(mb, case, "cuda", stats=dev[3], **opt)                  # accumulates, the same workspace
    same(again, u.run_case(mb, case, "cpu", stats=host[3], **opt))


@pytest.mark.parametrize("opt", OPTIONS[:3], ids=("all", "no-moments", "no-value-clip"))
def test_sequences_on_the_device_equal_the_host_path(seqs, opt):
    import madrona_bots as mb
    host = u.run_seq(mb, seqs, "cpu", **opt)
    dev = u.run_seq(mb, seqs, "cuda", **opt)
    same(dev, host)
    assert dev[3][0, 4] > 0 and dev[3][2].tolist() == [0.0] * 6
    again = u.run_seq(mb, seqs, "cuda", stats=dev[3], **opt)
    same(again, u.run_seq(mb, seqs, "cpu", stats=host[3], **opt))


def test_an_order_entry_outside_the_batch_is_a_column_of_length_zero():
    """The host path refuses such an entry; the device reads it as an empty
    column -- against the float32 restatement, which does the same."""
    import madrona_bots as mb
    bad = u.seq_case(bad_order=True)
    same(u.run_seq(mb, bad, "cuda"), u.ref_seq(bad))
    with pytest.raises(RuntimeError, match="is outside the"):
        u.run_seq(mb, bad, "cpu")


def test_gate_on_the_device():
    import madrona_bots as mb
    stats = np.zeros((5, 6))
    stats[:, 4] = [0.01, 0.03, np.nan, 0.0, 0.02]
    rows = np.array([7, 9, 11, 0, 13], np.int64)
    gate = np.array([7, 9, 11, 0, 0], np.int64)
    got = mb.ppo_kl_gate(u.t(stats, "cuda"), u.t(rows, "cuda"), 0.02, u.t(gate, "cuda")).cpu().numpy()
    assert got.tolist() == pr.gate(gate, rows, stats, 0.02).tolist() == [7, 0, 0, 0, 0]


def bits_equal(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def test_a_captured_three_epoch_update_replays_and_the_gate_stops_a_group():
    """old_logp is the old policy's own output, so the first epoch's KL is
    exactly 0 and both groups step; from the second epoch on group 0's KL lies
    above its target and its gate stays closed -- one step against three.
    Recorded after one warm call on a side stream and replayed twice: three
    eager updates on the device and on CPU tensors, bit for bit, in
    parameters, optimiser state and statistics."""
    import madrona_bots as mb
    targets = (1e-9, float("inf"))
    runs = {}
    for device in ("cuda", "cpu"):
        opt, stats, gate, update = u.update_case(mb, device, noisy_old=False, targets=targets)
        for _ in range(3):
            update()
        runs[device] = ([p.detach().cpu().clone() for p in opt.params], {k: v.cpu() for k, v in opt.state_dict().items()},
                        stats.cpu().clone(), gate.cpu().clone())
    opt, stats, gate, update = u.update_case(mb, "cuda", noisy_old=False, targets=targets)
    before = [p.detach().clone() for p in opt.params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        update()                                             # the warm call: workspaces and .grad bindings exist from here on
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update()                                             # (recorded, not run)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for which in ("cuda", "cpu"):
        params, sd, want_stats, want_gate = runs[which]
        assert all(bits_equal(a, b) for a, b in zip(opt.params, params)), which
        assert all(bits_equal(a, b) for a, b in zip(opt.state_dict().values(), sd.values())), which
        assert np.array_equal(pr.bits64(stats.cpu().numpy()), pr.bits64(want_stats.numpy())), which
        assert torch.equal(gate.cpu(), want_gate), which
    st = stats.cpu().numpy()
    assert opt.steps.tolist() == [1, 9]                # (the later updates find group 0 past its target at once)
    assert gate.tolist()[0] == 0 and gate.tolist()[1] > 0
    assert (st[0, :, 4] > 1e-9).all() and np.isfinite(st).all()               # (the third update's first epoch)
    assert sum(not torch.equal(a, b.detach()) for a, b in zip(before, opt.params)) >= len(before) // 2


def harness(name):
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import test_policy_ppo_cpu as ff
    import test_policy_ppo_seq_cpu as rec
    return (ff if name == "ppo_groups" else rec).harness_run


@pytest.mark.parametrize("name", ("ppo_groups", "ppo_recurrent_groups"))
def test_harness_hip_mode_leaves_the_cpu_mode_s_parameters(name):
    """64 worlds, two updates of three epochs: HIP mode and CPU mode end with
    the same bits in every parameter and the same statistics."""
    run = harness(name)
    before, after, log = run("hip", "cuda")
    host_before, host_after, host_log = run("cpu", "cpu")
    assert all(bits_equal(a, b) for g in range(4) for a, b in zip(before[g], host_before[g]))
    assert log == host_log and np.isfinite(np.array([r["stats"] for r in log])).all()
    for g in range(4):
        assert all(bits_equal(a, b) for a, b in zip(after[g], host_after[g])), g
    assert sum(not bits_equal(a, b) for a, b in zip(before[0], after[0])) >= len(before[0]) // 2
