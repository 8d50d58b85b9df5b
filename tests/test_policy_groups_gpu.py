"""GPU: policy groups on the device (DESIGN.md "Policy groups") -- the grouped
act kernel (the net table in device memory, the segment table and its scan in
LDS) against the CPU mode, bitwise, over every shape of policy_groups_util;
the same nets in every group against an ungrouped manager; policy_segments()
against numpy, with no host wait; and the capture of grouped act() + step()
into a graph with a weight refresh of one group between replays."""
import numpy as np
import pytest
import torch

import policy_ref as pr
import policy_groups_util as gu
import test_policy_cpu as tp
import test_policy_groups_cpu as tg
from simpair import compare

pytestmark = pytest.mark.gpu


def pair(shape, first=0, **kw):
    """A device and a CPU-mode manager of the shape with the same mixed nets."""
    g, c = gu.make_sim(shape, "hip", **kw), gu.make_sim(shape, "cpu", **kw)
    starts = gu.SHAPES[shape][1]
    nets = gu.make_group_nets(c, len(starts), first)
    needed = gu.needed_groups(starts, 0, gu.SHAPES[shape][0][0])
    for m in (g, c):
        gu.set_group_nets(m, nets, groups=needed)
    return g, c, nets


def assert_columns(g, c, where):
    for name in ("action_tensor", "hidden_state_tensor"):
        a, b = gu.bits(getattr(g, name)().to_torch()), gu.bits(getattr(c, name)().to_torch())
        assert a.shape == b.shape, (where, name)
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert not len(bad), (where, name, len(bad), int(bad[0]))


# ---- 1. device equals CPU mode, bitwise -----------------------------------------
@pytest.mark.parametrize("pattern", ["plain", "shift", "grow"])
@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_device_equals_cpu_mode(shape, pattern):
    g, c, _ = pair(shape)
    for t in range(6):
        if pattern == "grow" and t == 3:
            g.grow_capacity(256)
            c.grow_capacity(256)
        gu.assert_same_outputs(g.act(), c.act(), f"{shape} {pattern} round {t}")
        assert_columns(g, c, f"{shape} {pattern} round {t} after act")
        for m in (g, c):
            m.step()
            if pattern == "shift":
                m.shift_observations()
        assert_columns(g, c, f"{shape} {pattern} round {t} after step")
    errs = compare(g, tp._AsOracle(c), f"{shape} {pattern}")
    assert not errs, errs[:4]
    assert g.policy_groups == c.policy_groups == gu.SHAPES[shape][1]   # a growth leaves the groups alone


def test_mixed_memory_heads_on_the_device():
    tg.run_mixed_memory_heads("hip")


def test_lazy_hidden_state_under_mixed_memory_heads():
    """Nothing reads HiddenState between the shift and act(): the stretch of
    tests/test_lazy_hidden.py leaves the column owed as a row map, and act()
    with memory heads in group 0 only must copy out the rows group 1 keeps
    before it writes group 0's; with no memory head anywhere (no net reads the
    column either) it stays owed.  Outputs and the column against the CPU mode."""
    import madrona_bots as mb
    W, A = 40, 32
    big = tp.make_nets(gu.CASES[3], np.abs(np.random.default_rng(0).normal(0, 30, (64, 85))).astype(np.float32))
    none = tp.make_nets(gu.CASES[2], np.abs(np.random.default_rng(1).normal(0, 30, (64, 69))).astype(np.float32))
    for mixed in (True, False):
        g, c = (mb.SimManager(0, W, tp.SEED, A, exec_mode=e) for e in ("hip", "cpu"))
        for m in (g, c):
            m.set_policy_groups([0, 17])
            m.set_policy([pr.policy_net(n, m.device) for n in (big if mixed else none)], group=0)
            m.set_policy([pr.policy_net(n, m.device) for n in none], group=1)
        gen = torch.Generator().manual_seed(3)

        def write(memory):
            rows = c.num_rows()
            a = (torch.rand((rows, 6), generator=gen) < 0.5).to(torch.int32)
            mem = (torch.arange(rows * 16, dtype=torch.float32) + 1.0).reshape(rows, 16) if memory else None
            for m in (g, c):
                m.write_actions(a.to(m.device), None if mem is None else mem.to(m.device))
        write(True)
        for memory in (True, False, False, False):     # one eager step, then steps that leave the memory alone
            for m in (g, c):
                m.step()
                m.shift_observations()
            write(memory)
        assert g.schedule_info()["hidden_lazy"]
        gu.assert_same_outputs(g.act(), c.act(), f"lazy act, mixed={mixed}")
        assert g.schedule_info()["hidden_lazy"] == (not mixed)
        assert_columns(g, c, f"after the lazy act, mixed={mixed}")
        for m in (g, c):
            m.step()
            m.shift_observations()
        errs = compare(g, tp._AsOracle(c), f"a step after the lazy act, mixed={mixed}")
        assert not errs, errs[:4]


def test_shard_ghost_in_a_group_of_its_own_on_the_device():
    """A shard of four worlds with its ghost, starts [0, 2, 4]: the ghost
    (global world 4) is group 2's only world here.  Every row, the ghost's after
    row N included, against the CPU mode over act + step rounds."""
    import madrona_bots as mb
    W, A, starts = 4, 16, [0, 2, 4]
    g, c = (mb.SimManager(0, W, tp.SEED, A, exec_mode=e, shard_ghost=True) for e in ("hip", "cpu"))
    nets = gu.make_group_nets(c, 3, first=1)
    for m in (g, c):
        m.set_policy_groups(starts)
        gu.set_group_nets(m, nets)
    for t in range(4):
        rows, n = c.num_rows(), c.num_agents()
        assert g.num_rows() == rows > n
        outs = []
        for m in (g, c):
            out = {"action": torch.zeros((rows, 1), dtype=torch.int32, device=m.device),
                   "logp": torch.zeros((rows, 1), device=m.device), "value": torch.zeros((rows, 1), device=m.device)}
            m.act(out=out)
            outs.append(out)
            m.step()
            m.shift_observations()
        gu.assert_same_outputs(outs[0], outs[1], f"round {t}")
        assert (outs[1]["value"][n:] != 0).all()       # the ghost's rows were written
        assert np.array_equal(g.policy_segments().cpu().numpy(), c.policy_segments().numpy())
    errs = compare(g, tp._AsOracle(c), "after the rounds")
    assert not errs, errs[:4]


# ---- 2. the same nets in every group: an ungrouped manager ----------------------
@pytest.mark.parametrize("shape", ["B", "D"])
def test_same_nets_in_every_group_equal_an_ungrouped_manager_on_the_device(shape):
    tg.run_same_nets("hip", shape, "shift")


# ---- 3. segments ------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["B", "C", "D"])
def test_segments_on_the_device_equal_numpy_without_a_host_wait(shape):
    """policy_segments() after steps and shifts: one small launch that leaves
    the deferred columns owed and launches no kernel of the step's classes
    (schedule_info / kernel_times, counted as tests/test_defer_launches.py
    counts), and that a stream capture accepts -- a host wait would end one."""
    g = gu.make_sim(shape, "hip")
    starts = gu.SHAPES[shape][1]
    g.enable_kernel_timing(True)
    for t in range(3):
        g.write_synthetic_actions(99, t, True)
        g.step()
        g.shift_observations()
        info, launches = g.schedule_info(), {k: v[1] for k, v in g.kernel_times().items()}
        seg = g.policy_segments()
        assert g.schedule_info() == info
        assert {k: v[1] for k, v in g.kernel_times().items()} == launches
        sc = g.species_count_tensor().to_torch().cpu().numpy()
        assert seg.device == g.device and np.array_equal(seg.cpu().numpy(), gu.segments_numpy(sc, starts)), t
    g.enable_kernel_timing(False)
    out = torch.zeros((len(starts), 4, 2), dtype=torch.int32, device=g.device)
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
            for _ in range(2):            # (a captured sequence holds an even number of steps)
                g.step()
            g.policy_segments(out=out)
            g.join()
        for rep in range(2):
            graph.replay()
            torch.cuda.synchronize()
            sc = g.species_count_tensor().to_torch().cpu().numpy()
            assert np.array_equal(out.cpu().numpy(), gu.segments_numpy(sc, starts)), rep


# ---- 4. graph capture ---------------------------------------------------------------
def test_graph_capture_of_grouped_act_and_step():
    """Two act() + step() pairs with three groups recorded into a graph and
    replayed twice equal the eager rounds of the CPU mode, bitwise; between the
    replays set_policy(group=1) with the same architecture refreshes that
    group's weights in place, and the replay acts through them."""
    import madrona_bots as mb
    W, A, starts = 40, 32, [0, 13, 27]
    g, c = (mb.SimManager(0, W, tp.SEED, A, exec_mode=e) for e in ("hip", "cpu"))
    for m in (g, c):
        for t in range(3):
            m.write_synthetic_actions(4321, t, True)
            m.step()
        m.set_policy_groups(starts)
    nets = gu.make_group_nets(c, 3)
    # group 1's second set of weights: the same architecture (its codes kept)
    fresh = tp.make_nets(gu.CASES[1], pr.inputs(c, True) * np.float32(0.5))
    for n_old, n_new in zip(nets[1], fresh):
        n_new["trunk"] = [(w, b, code) for (w, b, _), (_, _, code) in zip(n_new["trunk"], n_old["trunk"])]
    for m in (g, c):
        gu.set_group_nets(m, nets)
    rows = W * 128
    outs = [{"action": torch.zeros((rows, 1), dtype=torch.int32, device=g.device),
             "logp": torch.zeros((rows, 1), dtype=torch.float32, device=g.device),
             "value": torch.zeros((rows, 1), dtype=torch.float32, device=g.device)} for _ in range(2)]
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
            for o in outs:
                assert g.act(out=o) is o
                with pytest.raises(RuntimeError, match="policy groups cannot be changed during a graph capture"):
                    g.set_policy_groups([0, 5])
                g.step()
            g.join()
        assert g.policy_groups == starts
        for rep in range(2):
            if rep == 1:
                g.set_policy([pr.policy_net(n, g.device) for n in fresh], group=1)
                # (what the refresh changes, in the CPU mode: group 1's values and no others)
                seg = c.policy_segments().tolist()
                draw = c.policy_draw
                old = c.act(write=False)["value"]
                c.set_policy([pr.policy_net(n) for n in fresh], group=1)
                new = c.act(write=False)["value"]
                c.policy_draw = draw
                for grp in range(3):
                    for lo, hi in seg[grp]:
                        assert hi > lo and torch.equal(old[lo:hi], new[lo:hi]) == (grp != 1)
            graph.replay()
            torch.cuda.synchronize()
            for o in outs:
                n = c.num_agents()
                oc = c.act()
                c.step()
                gu.assert_same_outputs({k: v[:n] for k, v in o.items()}, oc, f"replay {rep}")
        errs = compare(g, tp._AsOracle(c), "after the replays")
        assert not errs, errs[:4]
        assert g.policy_draw == c.policy_draw == 4
