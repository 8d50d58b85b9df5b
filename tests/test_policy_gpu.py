"""GPU: the device actor's HIP kernel (v_mfma_f32_16x16x4_f32 over 64-row
tiles) against the CPU mode, bitwise -- outputs, Action and HiddenState over
the whole grid of tests/test_policy_cpu.py and over act + step rounds --, its
capture into a graph next to step(), and a weight refresh between two calls
with no synchronisation."""
import numpy as np
import pytest
import torch

import policy_ref as pr
import test_policy_cpu as tp
from simpair import compare

pytestmark = pytest.mark.gpu


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def assert_same(o_hip, o_cpu, where):
    for k in ("action", "logp", "value"):
        g, c = bits(o_hip[k]), bits(o_cpu[k])
        assert g.shape == c.shape, (where, k, g.shape, c.shape)
        bad = np.nonzero(g != c)[0]
        assert not len(bad), (where, k, len(bad), int(bad[0]), o_hip[k][bad[0]].item(), o_cpu[k][bad[0]].item())


def pair(case, **kw):
    g, c = tp.make_sim(case, "hip", **kw), tp.make_sim(case, "cpu", **kw)
    nets = tp.make_nets(case, pr.inputs(c, case[3]))
    g.set_policy([pr.policy_net(n, g.device) for n in nets])
    c.set_policy([pr.policy_net(n) for n in nets])
    return g, c, nets


@pytest.mark.parametrize("case", tp.GRID, ids=tp.grid_id)
def test_hip_equals_cpu_mode_on_the_grid(case):
    g, c, _ = pair(case)
    for m in (g, c):
        m.policy_draw = 11
    assert_same(g.act(), c.act(), "sampled")
    errs = compare(g, tp._AsOracle(c), "after act")
    assert not errs, errs[:4]
    assert_same(g.act(greedy=True, write=False), c.act(greedy=True, write=False), "greedy")
    errs = compare(g, tp._AsOracle(c), "after a greedy act without the write", prev_too=False)
    assert not errs, errs[:4]


@pytest.mark.parametrize("pattern", ["plain", "shift", "shift4", "reset", "cap2048"])
def test_hip_equals_cpu_mode_over_rounds(pattern):
    """Six act + step rounds: every output and every column, bitwise; with the
    shift patterns of the learner loop, across a reset, and in a 2048-slot
    manager."""
    case = ("40x32", 48, 4, True, True) if pattern != "cap2048" else ("3x5", 128, 1, True, True)
    g, c, _ = pair(case, **({"agent_capacity": 2048} if pattern == "cap2048" else {}))
    for t in range(6):
        if pattern == "reset" and t == 2:
            g.reset_worlds([1, 7])
            c.reset_worlds([1, 7])
        assert_same(g.act(), c.act(), f"{pattern} round {t}")
        for m in (g, c):
            m.step()
            if pattern == "shift":
                m.shift_observations()
            elif pattern == "shift4":
                for _ in range(4):
                    m.shift_observations()
        errs = compare(g, tp._AsOracle(c), f"{pattern} round {t}")
        assert not errs, errs[:4]


@pytest.mark.parametrize("pattern", ["plain", "shift", "shift4", "grow"])
def test_hip_act_equals_three_call_sequence(pattern):
    tp.run_equivalence("hip", pattern)


def test_activation_sweep_device_equals_host_bitwise():
    import madrona_bots as mb
    x = tp.sweep()
    xd = torch.from_numpy(x).cuda()
    for name in list(pr.CODES.values()) + ["exp"]:
        assert np.array_equal(bits(mb.policy_activation(name, xd)), bits(mb.policy_activation(name, torch.from_numpy(x)))), name
    xl = np.concatenate([np.linspace(1.0, 7.0, 2_000_001), np.abs(x.astype(np.float64))]).astype(np.float32)
    assert np.array_equal(bits(mb.policy_activation("log", torch.from_numpy(xl).cuda())),
                          bits(mb.policy_activation("log", torch.from_numpy(xl))))


def test_graph_capture_of_act_and_step():
    """act() + step() recorded into a graph (a pair of rounds: a captured
    sequence holds an even number of steps) and replayed five times equals the
    ten eager rounds of the CPU mode, bitwise: the draw counter advances on
    every replayed act, and nothing in act() waits for the host."""
    case = ("40x32", 48, 4, True, True)
    g, c, _ = pair(case)
    rows = 41 * 128
    outs = [{"action": torch.zeros((rows, 1), dtype=torch.int32, device=g.device),
             "logp": torch.zeros((rows, 1), dtype=torch.float32, device=g.device),
             "value": torch.zeros((rows, 1), dtype=torch.float32, device=g.device)} for _ in range(2)]
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
            with pytest.raises(ValueError, match="out="):
                g.act()
            for o in outs:
                assert g.act(out=o) is o
                g.step()
            g.join()
        for rep in range(5):
            graph.replay()
            torch.cuda.synchronize()
            for o in outs:
                n = c.num_agents()
                oc = c.act()
                c.step()
                assert_same({k: v[:n] for k, v in o.items()}, oc, f"replay {rep}")
        errs = compare(g, tp._AsOracle(c), "after the replays")
        assert not errs, errs[:4]
        assert g.policy_draw == c.policy_draw == 10


def test_weight_refresh_between_two_acts():
    """set_policy with the same architecture and new weights from device
    tensors, issued between two act() calls with no synchronisation, takes
    effect on the second call and only there."""
    case = ("40x32", 128, 4, False, True)
    g, c, nets = pair(case)
    new = tp.make_nets(("40x32", 128, 4, False, True), pr.inputs(c, False) * np.float32(0.5))
    for n_old, n_new in zip(nets, new):      # the same architecture: the old activation codes
        n_new["trunk"] = [(w, b, code) for (w, b, _), (_, _, code) in zip(n_new["trunk"], n_old["trunk"])]
    g.policy_draw = 5
    first = g.act(write=False)
    fresh = [pr.policy_net(n, g.device) for n in new]
    g.policy_draw = 5
    g.set_policy(fresh)
    del fresh
    junk = [torch.full((128, 128), 7.0, device=g.device) for _ in range(40)]   # (reuses what the upload read)
    second = g.act(write=False)
    del junk
    c.policy_draw = 5
    assert_same(first, c.act(write=False), "before the refresh")
    c.set_policy([pr.policy_net(n) for n in new])
    c.policy_draw = 5
    assert_same(second, c.act(write=False), "after the refresh")
    assert not torch.equal(first["value"], second["value"])
