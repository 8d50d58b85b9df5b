"""GPU: PolicyNet.evaluate_sequences and its backward kernel through time
against the CPU path of the same library, bitwise, on the grid of
tests/policy_seq_ref.py; against act() along the window's lifelines on a HIP
manager; and captured into a graph."""
import numpy as np
import pytest
import torch

import policy_seq_ref as sr
import test_policy_seq_cpu as ts

pytestmark = pytest.mark.gpu

NAMES = ["logp", "value", "entropy", "hidden"]


@pytest.mark.parametrize("case", sr.CASES, ids=sr.case_id)
def test_device_equals_cpu_path_bitwise(case):
    """Every output, hidden and every gradient; two device calls in a row agree too."""
    b = sr.build(case)
    cpu = sr.flat(sr.run_sequences(*b))
    dev = sr.flat(sr.run_sequences(*b, device="cuda"))
    again = sr.flat(sr.run_sequences(*b, device="cuda"))
    for name, c, d, e in zip(NAMES + sr.param_names(b[0]), cpu, dev, again):
        if c is None:
            assert d is None and e is None
            continue
        bad = np.nonzero(sr.bits(c).ravel() != sr.bits(d).ravel())[0]
        assert not len(bad), (name, len(bad), int(bad[0]), c.ravel()[bad[0]], d.ravel()[bad[0]])
        assert np.array_equal(sr.bits(d), sr.bits(e)), name


def test_same_bits_as_act_through_the_window_on_a_hip_manager():
    ts.check_window_bits("hip")


def test_forward_and_backward_in_a_graph():
    """evaluate_sequences + backward captured once and replayed on changed
    rows equal the CPU path of those rows (a single-stream capture; no queue
    setting is touched here)."""
    case = sr.CASES[5]
    net, obs, action, length, hidden0, g = sr.build(case)
    _, obs2, action2, length2, hidden2, g2 = sr.build(case, seed=1)
    p, ps = sr.policy_net(net, "cuda")
    t = lambda a: torch.from_numpy(a).cuda()
    s_in = [t(obs), t(action), t(length), t(hidden0)]
    s_g = [t(q) for q in g]

    def run():
        out = p.evaluate_sequences(*s_in, return_hidden=True)
        grads = torch.autograd.grad(sum((q * o).sum() for q, o in zip(s_g, out[:3])), ps)
        return list(out) + list(grads)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                  # warm-up: the workspace and the allocator's blocks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run()
    for rows, gs in (((obs, action, length, hidden0), g), ((obs2, action2, length2, hidden2), g2)):
        for dst, src in zip(s_in + s_g, list(rows) + list(gs)):
            dst.copy_(t(src))
        graph.replay()
        torch.cuda.synchronize()
        want = sr.flat(sr.run_sequences(net, *rows, gs))
        for name, a, b in zip(NAMES + sr.param_names(net), res, want):
            assert np.array_equal(sr.bits(a.detach().cpu().numpy()), sr.bits(b)), name
