"""GPU: PolicyNet.evaluate and its backward kernel (v_mfma_f32_16x16x4_f32 for
both gradient products) against the CPU path of the same library, bitwise, on
the grid of tests/test_policy_grad_cpu.py; against act() on a HIP manager; and
captured into a graph."""
import numpy as np
import pytest
import torch

import policy_ref as pr
import policy_grad_ref as gr
import test_policy_cpu as tp
import test_policy_grad_cpu as tg

pytestmark = pytest.mark.gpu


def flat(o):
    return list(o[:3]) + o[3]


@pytest.mark.parametrize("case", tg.CASES, ids=tg.case_id)
def test_device_equals_cpu_path_bitwise(case):
    """Every output and every gradient; two device calls in a row agree too."""
    net, obs, hidden, action, g = tg.build(case)
    cpu = flat(tg.run_evaluate(net, obs, hidden, action, g))
    dev = flat(tg.run_evaluate(net, obs, hidden, action, g, "cuda"))
    again = flat(tg.run_evaluate(net, obs, hidden, action, g, "cuda"))
    names = ["logp", "value", "entropy"] + gr.param_names(net)
    for name, c, d, e in zip(names, cpu, dev, again):
        if c is None:
            assert d is None and e is None
            continue
        bad = np.nonzero(tg.bits(c).ravel() != tg.bits(d).ravel())[0]
        assert not len(bad), (name, len(bad), int(bad[0]), c.ravel()[bad[0]], d.ravel()[bad[0]])
        assert np.array_equal(tg.bits(d), tg.bits(e)), name


@pytest.mark.parametrize("shift", [False, True], ids=["plain", "shifted"])
def test_evaluate_reproduces_act_on_a_hip_manager(shift):
    import madrona_bots as mb
    sim = mb.SimManager(0, 16, tp.SEED, 32, exec_mode="hip")
    for t in range(3):
        sim.write_synthetic_actions(4321, t, True)
        sim.step()
    if shift:
        sim.shift_observations()
    case = ("40x32", 128, 4, True, True)
    nets = [pr.policy_net(n, sim.device) for n in tp.make_nets(case, pr.inputs(sim, True))]
    sim.set_policy(nets)
    o = sim.act(write=False)
    obs, hidden = sim.construct_obs(), sim.hidden_state_tensor().to_torch()
    end = np.cumsum(sim.species_count_tensor().to_torch().cpu().numpy().sum(axis=0))
    lo = 0
    for s in range(4):
        hi = int(end[s])
        logp, value, _ = nets[s].evaluate(obs[lo:hi], o["action"][lo:hi], hidden[lo:hi])
        assert torch.equal(logp.view(torch.int32), o["logp"][lo:hi, 0].view(torch.int32))
        assert torch.equal(value.view(torch.int32), o["value"][lo:hi, 0].view(torch.int32))
        lo = hi
    assert lo == sim.num_agents() and lo > 64


def test_forward_and_backward_in_a_graph():
    """evaluate + backward captured once and replayed on changed rows equal
    the CPU path of those rows (the capture needs the machine's default of at
    least 4 hardware queues; no queue setting is touched here)."""
    case = tg.CASES[5]
    net, obs, hidden, action, g = tg.build(case)
    net2, obs2, _, action2, g2 = tg.build(case, seed=1)
    p, ps = gr.policy_net(net, "cuda")
    t = lambda a: torch.from_numpy(a).cuda()
    s_obs, s_act, s_g = t(obs), t(action), [t(q) for q in g]

    def run():
        out = p.evaluate(s_obs, s_act)
        grads = torch.autograd.grad(sum((q * o).sum() for q, o in zip(s_g, out)), ps)
        return list(out) + list(grads)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                  # warm-up: the workspace and the allocator's blocks
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run()
    for rows, acts, gs in ((obs, action, g), (obs2, action2, g2)):
        s_obs.copy_(t(rows))
        s_act.copy_(t(acts))
        for dst, src in zip(s_g, gs):
            dst.copy_(t(src))
        graph.replay()
        torch.cuda.synchronize()
        want = flat(tg.run_evaluate(net, rows, None, acts, gs))
        for name, a, b in zip(["logp", "value", "entropy"] + gr.param_names(net), res, want):
            assert np.array_equal(tg.bits(a.detach().cpu().numpy()), tg.bits(b)), name
