"""GPU: the gated memory head (DESIGN.md "Gated memory head") on the device
against the CPU path of the same library, bitwise -- the sigmoid, act() in the
one-group and the grouped launch, evaluate_sequences and its backward kernel on
the cases of tests/policy_gate_ref.py, the grouped call, act() along the
window's lifelines on a HIP manager, a graph of forward and backward, and the
refusal of a gated net over an ungated one under capture."""
import numpy as np
import pytest
import torch

import policy_ref as pr
import policy_gate_ref as gg
import policy_groups_util as pgu
import policy_seq_groups_util as psu
import test_policy_cpu as tpc
import test_policy_gate_cpu as tg

pytestmark = pytest.mark.gpu

NAMES = ["logp", "value", "entropy", "hidden"]


def test_sigmoid_device_equals_host_bitwise():
    import madrona_bots as mb
    x = np.concatenate([tpc.sweep(), np.array([200.0, -200.0, 17.0, 18.0, -104.5, np.nan, np.inf, -np.inf], np.float32)])
    dev = mb.policy_activation("Sigmoid", torch.from_numpy(x).cuda()).cpu().numpy()
    host = mb.policy_activation("Sigmoid", torch.from_numpy(x)).numpy()
    assert np.array_equal(gg.bits(dev), gg.bits(host))


def managers(H, grouped):
    """A HIP and a CPU manager of 16 worlds with the same nets: four gated ones
    of width H, or two groups that mix gated and ungated nets of width H and 48."""
    import madrona_bots as mb
    out = []
    for mode in ("hip", "cpu"):
        s = mb.SimManager(0, 16, 77, 32, exec_mode=mode)
        for t in range(3):
            s.write_synthetic_actions(4321, t, True)
            s.step()
        out.append(s)
    x = pr.inputs(out[1], True)
    rng = np.random.default_rng(100 + H)
    mk = lambda h, codes: pr.calibrate_actor(pr.make_net(rng, h, len(codes), codes, True, True, pr.in_scale(x)), x)
    codes = [3, 1, 4][:1 if H == 16 else 3]
    if not grouped:
        dicts = [[gg.add_gate(rng, mk(H, codes)) for _ in range(4)]]
    else:
        dicts = [[gg.add_gate(rng, mk(H, codes)), mk(48, [2]), gg.add_gate(rng, mk(48, [5, 0])), mk(H, codes)],
                 [mk(H, codes), gg.add_gate(rng, mk(H, codes)), mk(48, [4]), gg.add_gate(rng, mk(H, codes))]]
    for s in out:
        if grouped:
            s.set_policy_groups([0, 7])
        for u, four in enumerate(dicts):
            s.set_policy([gg.policy_net(d, s.device, False)[0] for d in four], group=u if grouped else None)
    return out


@pytest.mark.parametrize("grouped", [False, True], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("H", [16, 128])
def test_act_device_equals_cpu_mode(H, grouped):
    g, c = managers(H, grouped)
    for t in range(3):
        pgu.assert_same_outputs(g.act(), c.act(), f"round {t}")
        a, b = (pgu.bits(m.hidden_state_tensor().to_torch()) for m in (g, c))
        assert np.array_equal(a, b), t
        for m in (g, c):
            m.step()
    # NO_WRITE leaves the column alone
    before = g.hidden_state_tensor().to_torch().clone()
    pgu.assert_same_outputs(g.act(write=False), c.act(write=False), "no write")
    assert torch.equal(before.view(torch.int32), g.hidden_state_tensor().to_torch().view(torch.int32))


@pytest.mark.parametrize("case", gg.CASES, ids=gg.case_id)
def test_sequences_device_equals_cpu_path_bitwise(case):
    """Every output, hidden and every gradient (the gate's included); two device calls in a row agree too."""
    b = gg.build(case)
    cpu = gg.flat(gg.run_sequences(*b))
    dev = gg.flat(gg.run_sequences(*b, device="cuda"))
    again = gg.flat(gg.run_sequences(*b, device="cuda"))
    for name, c, d, e in zip(NAMES + gg.param_names(b[0]), cpu, dev, again):
        if c is None:
            assert d is None and e is None
            continue
        bad = np.nonzero(gg.bits(c).ravel() != gg.bits(d).ravel())[0]
        assert not len(bad), (name, len(bad), int(bad[0]), c.ravel()[bad[0]], d.ravel()[bad[0]])
        assert np.array_equal(gg.bits(d), gg.bits(e)), name


def test_grouped_sequences_device_equals_cpu_path_bitwise():
    fx = tg.group_fixture()
    cpu = psu.run_grouped(*fx, pn_params=tg.group_policy_nets(fx[0]))
    dev = psu.run_grouped(*fx, device="cuda", pn_params=tg.group_policy_nets(fx[0], "cuda"))
    psu.assert_same(cpu, dev, "grouped, device against CPU path")


def test_same_bits_as_act_through_the_window_on_a_hip_manager():
    tg.check_window_bits("hip")


def test_forward_and_backward_in_a_graph():
    """evaluate_sequences + backward of a gated net captured once and replayed
    on changed rows equal the CPU path of those rows (a single-stream capture)."""
    case = gg.CASES[3]
    net, obs, action, length, hidden0, g = gg.build(case)
    _, obs2, action2, length2, hidden2, g2 = gg.build(case, seed=1)
    p, ps = gg.policy_net(net, "cuda")
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
        want = gg.flat(gg.run_sequences(net, *rows, gs))
        for name, a, b in zip(NAMES + gg.param_names(net), res, want):
            assert np.array_equal(gg.bits(a.detach().cpu().numpy()), gg.bits(b)), name


def test_gated_net_over_an_ungated_one_is_refused_under_capture():
    """Gatedness is part of the architecture: the gated twin of the net in
    place allocates, so a capture refuses it; the net in place stays."""
    import madrona_bots as mb
    g = mb.SimManager(0, 16, 77, 32, exec_mode="hip")
    for t in range(3):
        g.write_synthetic_actions(4321, t, True)
        g.step()
    x = pr.inputs(g, True)
    nets = tpc.make_nets(("40x32", 48, 4, True, True), x)
    rng = np.random.default_rng(3)
    plain = [gg.policy_net(n, g.device, False)[0] for n in nets]
    gated = [gg.policy_net(gg.add_gate(rng, n), g.device, False)[0] for n in nets]
    g.set_policy(plain)
    g.policy_draw = 3
    want = g.act(write=False)
    rows = 17 * 128
    o = {"action": torch.zeros((rows, 1), dtype=torch.int32, device=g.device),
         "logp": torch.zeros((rows, 1), dtype=torch.float32, device=g.device),
         "value": torch.zeros((rows, 1), dtype=torch.float32, device=g.device)}
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
            with pytest.raises(RuntimeError, match="new architecture allocates"):
                g.set_policy(gated)
            g.set_policy(plain)                 # the same architecture: re-uploads, capturable
            g.act(out=o, write=False)
            g.join()
        g.policy_draw = 3
        graph.replay()
        torch.cuda.synchronize()
    n = want["logp"].shape[0]
    pgu.assert_same_outputs({k: v[:n] for k, v in o.items()}, want, "the ungated net stayed in place")
    g.set_policy(gated)                         # outside a capture it allocates and is accepted
    g.act()
