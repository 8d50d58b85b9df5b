"""GPU: the device learner step on the device (DESIGN.md "Device learner step":
policy_adam_kernel, policy_a2c_loss_kernel) -- the cases of
test_policy_adam_cpu.py on device tensors against the host path, bit for bit; a
whole update recorded into a graph and replayed; and harness/a2c_groups.py
--device-update in HIP mode against CPU mode."""
import numpy as np
import pytest
import torch

import policy_adam_util as u
import test_policy_adam_cpu as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def test_adam_on_the_device_equals_the_host_path():
    import madrona_bots as mb
    opt, before, trace = u.run_adam(mb, DEV)
    host_opt, host_before, host_trace = u.run_adam(mb, "cpu")
    assert sum(p.data_ptr() % 16 != 0 for p in opt.params) == 1 and len(opt.params) > 64
    assert all(same(a, b) for a, b in zip(before, host_before))
    for k, ((params, sd), (host_params, host_sd)) in enumerate(zip(trace, host_trace)):
        for i, (a, b) in enumerate(zip(params, host_params)):
            assert same(a, b), f"step {k}, {opt.names[i]}"
        assert same(sd["m"], host_sd["m"]) and same(sd["v"], host_sd["v"]), f"step {k}"
        assert torch.equal(sd["state"], host_sd["state"]), f"step {k}"
    assert trace[-1][1]["state"][:, 0].tolist() == [0 if g == u.IDLE_GROUP else u.STEPS for g in range(u.GROUPS)]


@pytest.mark.parametrize("end", (True, False), ids=("end", "no-end"))
def test_loss_on_the_device_equals_the_host_path(end):
    import madrona_bots as mb
    got, want = tc.run_loss(DEV, end), tc.run_loss("cpu", end)
    for name, a, b in zip(("g_logp", "g_value", "g_entropy"), got, want):
        assert np.array_equal(tc.bits(a), tc.bits(b)), name
    assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64)) and got[3][0] != 0
    twice = tc.run_loss(DEV, end, loss=tc.t(got[3].copy(), DEV))[3]
    assert np.array_equal(twice.view(np.uint64), tc.run_loss("cpu", end, loss=tc.t(want[3].copy()))[3].view(np.uint64))
    segments = tc.t(u.loss_case()[2], DEV)
    total = torch.zeros(u.LOSS_G, dtype=torch.int64, device=DEV)
    mb.policy_group_rows(segments, total)
    mb.policy_group_rows(segments, total)
    assert total.tolist() == [2 * 299, 2 * 1840, 2 * 60]


def update_case(device, seed=31):
    """Two groups of four H = 16 nets, 300 recorded rows in segments with a
    gap, and everything an update reads; update() is one whole device update."""
    import madrona_bots as mb
    rng = np.random.default_rng(seed)
    nets = [[u.make_net(mb, rng, 16, device) for _ in range(4)] for _ in range(2)]
    n = 300
    obs = tc.t(np.abs(rng.normal(0.0, 3.0, (n, 69))).astype(np.float32), device)
    action = tc.t(rng.integers(0, 6, n).astype(np.int32), device)
    adv, ret = (tc.t(rng.standard_normal(n).astype(np.float32), device) for _ in range(2))
    end = tc.t(rng.integers(0, 4, n).astype(np.int32), device)
    seg = torch.tensor([[[0, 70], [70, 71], [71, 71], [71, 140]],
                        [[150, 215], [215, 280], [280, 290], [290, 300]]], dtype=torch.int32, device=device)
    opt = mb.PolicyAdam(nets, lr=1e-2)
    rows = mb.policy_group_rows(seg, torch.zeros(2, dtype=torch.int64, device=device))
    loss = torch.zeros(2, dtype=torch.float64, device=device)

    def update():
        opt.zero_grad()
        loss.zero_()
        outs = mb.evaluate_groups(nets, obs, action, seg)
        g = mb.a2c_loss_groups(*outs, adv, ret, end, seg, rows, 0.5, 0.01, loss=loss)
        torch.autograd.backward(list(outs), list(g[:3]))
        opt.step(rows)
    return opt, loss, update


def test_a_captured_update_replays():
    """Forward, loss, backward, zero_grad and step recorded after one eager
    warm-up call and replayed twice: three eager updates, bit for bit, on the
    device and in CPU mode."""
    runs = {}
    for device in (DEV, "cpu"):
        opt, loss, update = update_case(device)
        for _ in range(3):
            update()
        runs[device] = [p.detach().cpu().clone() for p in opt.params], opt.state_dict(), loss.cpu().clone()
    opt, loss, update = update_case(DEV)
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
    for which in (DEV, "cpu"):
        params, sd, want_loss = runs[which]
        assert all(same(a.detach(), b) for a, b in zip(opt.params, params)), which
        assert all(same(a, b) if a.is_floating_point() else torch.equal(a.cpu(), b.cpu())
                   for a, b in zip(opt.state_dict().values(), sd.values())), which
        assert torch.equal(loss.cpu(), want_loss), which
    assert opt.state_dict()["state"][:, 0].tolist() == [3, 3]
    assert sum(not torch.equal(a, b.detach()) for a, b in zip(before, opt.params)) >= len(before) // 2


def test_harness_device_update_leaves_the_cpu_mode_s_parameters():
    """harness/a2c_groups.py --device-update, 64 worlds, two updates: HIP mode
    and CPU mode end with the same bits in every parameter, and the same
    losses -- the end-to-end claim of the device learner step."""
    before, after, losses = tc.harness_run("hip", DEV)
    host_before, host_after, host_losses = tc.harness_run("cpu", "cpu")
    assert all(same(a, b) for g in range(4) for a, b in zip(before[g], host_before[g]))
    assert np.isfinite(losses).all() and losses == host_losses
    for g in range(4):
        assert all(same(a, b) for a, b in zip(after[g], host_after[g])), g
    assert sum(not same(a, b) for a, b in zip(before[0], after[0])) >= len(before[0]) // 2
