"""GPU: madrona_bots.evaluate_groups on the device (DESIGN.md "Grouped
evaluate": policy_eval_groups_kernel, the backward's waves and their reduce)
on the fixture of tests/policy_eval_groups_util.py -- against the per-net
evaluate() loop on the device and against the CPU mode, bit for bit; against
act() on a grouped manager; and recorded into a graph that is replayed on
other contents of `segments`."""
import numpy as np
import pytest
import torch

import policy_ref as pr
import policy_grad_ref as gr
import policy_groups_util as gu
import policy_eval_groups_util as u
import test_policy_cpu as tp

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def grouped():
    nets, seg, n, obs, hidden, action, g = u.fixture()
    return u.run_grouped(nets, seg, obs, hidden, action, g, DEV)


# ---- 1. to 3. of the CPU file, on the device ------------------------------------------
def test_outputs_and_gradients_equal_the_per_net_loop(grouped):
    nets, seg, n, obs, hidden, action, g = u.fixture()
    u.assert_same(grouped, u.run_loop(nets, seg, obs, hidden, action, g, DEV), "device")
    assert all(float(o.abs().max()) > 0 for o in grouped[0])
    assert all(float(q.abs().max()) > 0 for q in grouped[1][0][0] + grouped[1][1][3] + grouped[1][2][1])
    assert all(not q.any() for q in grouped[1][0][1])                         # the empty segment: zeros


def test_rows_outside_are_zero_and_change_nothing(grouped):
    nets, seg, n, obs, hidden, action, g = u.fixture()
    outside = u.outside_rows(seg, n, nets)
    for o in grouped[0]:
        assert not o.cpu().view(torch.int32)[torch.from_numpy(outside)].any()
    rng = np.random.default_rng(5)
    obs2, hidden2, action2 = obs.copy(), hidden.copy(), action.copy()
    obs2[outside] = rng.normal(0, 1e6, (int(outside.sum()), 69)).astype(np.float32)
    obs2[np.nonzero(outside)[0][0]] = np.nan
    hidden2[outside] = 3.0
    action2[outside] = 77
    g2 = [gi.copy() for gi in g]
    for gi in g2:
        gi[outside] = 1e30
    u.assert_same(u.run_grouped(nets, seg, obs2, hidden2, action2, g2, DEV), grouped, "outside rows changed")


def test_one_net_for_four_species_equals_four_evaluate_calls():
    """As the CPU file's test 3: outputs bit for bit; each shared parameter's
    gradient within the three roundings of autograd's four-term f32 sum."""
    import madrona_bots as mb
    nets, _, _, obs, hidden, action, g = u.fixture()
    d = nets[0][0]
    seg, n = u.segments_of([[65, 1, 64, 63]], [(0, 2), (0, 0), (0, 3), (0, 1)])
    obs, action, g = obs[:n], action[:n], [gi[:n] for gi in g]
    ref = u.run_loop([[d, d, d, d]], seg, obs, None, action, g, DEV)
    net, ps = gr.policy_net(d, DEV)
    to, ta, ts, *tg = u.to(DEV, obs, action, seg, *g)
    out = mb.evaluate_groups([net], to, ta, ts)
    sum((gi * oi).sum() for gi, oi in zip(tg, out)).backward()
    for a, b in zip(out, ref[0]):
        assert torch.equal(a.detach(), b)
    for i, q in enumerate(ps):
        parts = torch.stack([ref[1][0][s][i] for s in range(4)]).double()
        bound = 3 * 2.0 ** -24 * parts.abs().sum(0)
        assert bool(((q.grad.double() - parts.sum(0)).abs() <= bound).all()), i


# ---- the device's bits are the CPU mode's -------------------------------------------------
def test_device_equals_cpu_mode(grouped):
    nets, seg, n, obs, hidden, action, g = u.fixture()
    u.assert_same(grouped, u.run_grouped(nets, seg, obs, hidden, action, g, "cpu"), "device against CPU mode")


# ---- act()'s logp and value on a grouped manager ---------------------------------------------
def test_reproduces_act_on_a_grouped_manager():
    import madrona_bots as mb
    sim = mb.SimManager(0, 48, tp.SEED, 16, exec_mode="hip")
    for t in range(3):
        sim.write_synthetic_actions(4321, t, True)
        sim.step()
    sim.set_policy_groups([0, 16, 32])
    nets = gu.make_group_nets(sim, 3)                       # small / big with memory_in / small
    pn = [[pr.policy_net(d, sim.device) for d in four] for four in nets]
    for grp in range(3):
        sim.set_policy(pn[grp], group=grp)
    obs, hidden = sim.construct_obs().clone(), sim.hidden_state_tensor().to_torch().clone()
    seg = sim.policy_segments()
    o = sim.act(write=False)
    n = sim.num_agents()
    assert obs.shape[0] == n and int((seg[..., 1] - seg[..., 0]).sum()) == n
    logp, value, entropy = mb.evaluate_groups(pn, obs, o["action"], seg, hidden)
    assert torch.equal(logp.view(torch.int32), o["logp"][:, 0].view(torch.int32))
    assert torch.equal(value.view(torch.int32), o["value"][:, 0].view(torch.int32))
    assert bool(((entropy > 0) & (entropy <= np.log(6.0) + 1e-5)).all())


# ---- graph capture ---------------------------------------------------------------------------------
def test_graph_capture_and_replay_on_other_segments(grouped):
    """Forward and backward recorded after one warm call (one stream, nothing
    forked), replayed twice on other contents of `segments`: each replay
    equals the eager call on those segments."""
    import madrona_bots as mb
    nets, seg, n, obs, hidden, action, g = u.fixture()
    other, n2 = u.segments_of([[16385, 63, 1, 64], [1, 65, 64, 0], [64, 65, 65, 63]], u.ORDER[::-1])
    assert n2 <= n
    pn, params = u.policy_nets(nets, DEV)
    to, th, ta, ts, *tg = u.to(DEV, obs, hidden, action, seg, *g)
    live = [q for four in params for ps in four for q in ps or [] if q is not None]

    def call():
        out = mb.evaluate_groups(pn, to, ta, ts, th)
        return list(out), torch.autograd.grad(sum((gi * oi).sum() for gi, oi in zip(tg, out)), live)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                               # the warm call: the workspace exists from here on
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = call()
    for contents, want in ((other, None), (seg, grouped)):
        ts.copy_(torch.from_numpy(contents))
        graph.replay()
        torch.cuda.synchronize()
        if want is None:
            want = u.run_grouped(nets, contents, obs, hidden, action, g, DEV)
        for k, a, b in zip(("logp", "value", "entropy"), out, want[0]):
            assert torch.equal(a.detach(), b), k
        flat = [q for four in want[1] for ps in four for q in ps or [] if q is not None]
        assert len(flat) == len(grads) and all(torch.equal(a, b) for a, b in zip(grads, flat))
