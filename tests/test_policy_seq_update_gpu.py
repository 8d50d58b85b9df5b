"""GPU: the recurrent update on the device (DESIGN.md "Device learner step":
policy_seq_group_rows_kernel, policy_seq_a2c_loss_kernel, the kernels of
mbots_policy_adam_clip) -- the cases of test_policy_seq_loss_cpu.py and
test_policy_clip_cpu.py on device tensors against the host path, bit for bit; a
whole recurrent update recorded into a graph and replayed on new batches; and
harness/a2c_recurrent_groups.py --device-update in HIP mode against CPU mode."""
import os
import sys

import numpy as np
import pytest
import torch

import policy_adam_util as au
import policy_seq_loss_util as u

pytestmark = pytest.mark.gpu
DEV = "cuda"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


@pytest.mark.parametrize("last_table", [u.LAST_TABLE, -1], ids=["last_table_4", "no_bound"])
def test_sequence_loss_on_the_device_equals_the_host_path(last_table):
    import madrona_bots as mb
    case = u.seq_case()
    start = np.array([1.5, -2.25, -0.0], np.float64)
    for loss in (None, start):
        got, want = u.seq_run(mb, case, DEV, last_table, loss), u.seq_run(mb, case, "cpu", last_table, loss)
        for name, a, b in zip(("order", "segments", "rows"), got[:3], want[:3]):
            assert np.array_equal(a, b), name
        for name, a, b in zip(("g_logp", "g_value", "g_entropy"), got[3:6], want[3:6]):
            assert np.array_equal(bits(a), bits(b)), name
        assert np.array_equal(got[6].view(np.uint64), want[6].view(np.uint64)) and got[6][0] != 0
    assert (got[2][u.DEAD_GROUP] == 0) == (last_table >= 0)


def test_the_device_clamps_what_the_host_refuses():
    """A segment past B, an order entry outside [0, B) and a length past L: the
    calls run, such a column counts as min(len, L) steps or none, and nothing
    outside the [L, B] outputs is written (the elements behind them stay)."""
    import madrona_bots as mb
    case = u.seq_case()
    c = u.seq_tensors(case, DEV)
    order, seg = mb.sequence_segments(c["net_id"], u.SEQ_G)
    seg = seg.clone()
    last = int(seg[2, 3, 1])
    seg[2, 3, 1] = u.SEQ_B + 1000                          # the last pair's segment runs past the columns
    order = order.clone()
    first = int(order[0])
    order[1] = u.SEQ_B + 5
    order[2] = -3
    length = c["length"].clone()
    length[first] = u.SEQ_L + 7
    rows = mb.sequence_group_rows(length, c["t0"], c["end"], order, seg,
                                  torch.zeros(u.SEQ_G, dtype=torch.int64, device=DEV), -1)
    big = [torch.full((u.SEQ_L + 1, u.SEQ_B), 7.0, device=DEV) for _ in range(5)]
    for dst, k in zip(big, ("logp", "value", "entropy", "adv", "ret")):
        dst[:u.SEQ_L] = c[k]
    out = mb.a2c_loss_sequences(*[x[:u.SEQ_L] for x in big], length, c["t0"], c["end"], order, seg, rows, -1)
    torch.cuda.synchronize()
    assert all(torch.isfinite(x).all() for x in out) and rows[0] > 0
    assert all((x[u.SEQ_L] == 7.0).all() for x in big)
    assert int(seg[2, 3, 0]) <= last                       # (the clamp is the kernel's; the tensor is the caller's)
    n = u.SEQ_L - (1 if int(c["end"][first]) == 2 else 0)       # the length read as min(len, L)
    assert int((out[0][:, first] != 0).sum()) == n


def test_clipped_adam_on_the_device_equals_the_host_path():
    import madrona_bots as mb
    got, want = u.run_clip(mb, DEV), u.run_clip(mb, "cpu")
    for k, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(("param", "m", "v"), a[:3], b[:3]):
            for i in range(u.CLIP_TENSORS):
                assert np.array_equal(bits(x[i]), bits(y[i])), f"step {k}, {name} of tensor {i}"
        assert np.array_equal(a[3], b[3]) and np.array_equal(bits(a[4]), bits(b[4])), f"step {k}"
    assert got[-1][3][:, 0].tolist() == [3, 3, 0, 2] and np.isinf(got[0][4][u.INF])


def test_policy_adam_options_on_the_device():
    """max_grad_norm = inf and the defaults leave today's bits; with options the
    device equals the host path after three steps, grad_norm included."""
    import madrona_bots as mb

    def three_steps(device, **kw):
        opt = mb.PolicyAdam(au.make_groups(mb, device), **au.HYPER, **kw)
        rows = au.rows_of(device)
        for k in range(au.STEPS):
            au.set_gradients(opt, au.gradients(opt, k))
            opt.step(rows)
        return opt
    plain = au.run_adam(mb, DEV)[0]
    for other in (three_steps(DEV), three_steps(DEV, max_grad_norm=float("inf"))):
        assert all(same(a.detach(), b.detach()) for a, b in zip(plain.params, other.params))
        assert all(torch.equal(a, b) for a, b in zip(plain.state_dict().values(), other.state_dict().values()))
    dev, host = (three_steps(d, max_grad_norm=0.5, weight_decay=0.01) for d in (DEV, "cpu"))
    assert all(same(a.detach(), b.detach()) for a, b in zip(dev.params, host.params))
    assert same(dev.grad_norm, host.grad_norm) and (dev.grad_norm > 0.5).any()
    assert all(same(a, b) if a.is_floating_point() else torch.equal(a.cpu(), b)
               for a, b in zip(dev.state_dict().values(), host.state_dict().values()))


# ---- a whole update, eager and captured ---------------------------------------------------------
UP_L, UP_B, UP_G, UP_LAST = 3, 330, 2, 4


def update_batches(seed=41):
    """Three batches of 330 padded sequences for two groups of four gated nets."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        b = dict(net_id=rng.integers(-1, 4 * UP_G + 1, UP_B).astype(np.int32),
                 length=rng.integers(0, UP_L + 1, UP_B).astype(np.int32),
                 t0=rng.integers(0, 5, UP_B).astype(np.int32), end=rng.integers(0, 4, UP_B).astype(np.int32),
                 obs=np.abs(rng.normal(0.0, 3.0, (UP_L, UP_B, 69))).astype(np.float32),
                 action=rng.integers(0, 6, (UP_L, UP_B)).astype(np.int32),
                 hidden0=rng.uniform(-1.0, 1.0, (UP_B, 16)).astype(np.float32),
                 adv=rng.standard_normal((UP_L, UP_B)).astype(np.float32),
                 ret=rng.standard_normal((UP_L, UP_B)).astype(np.float32))
        out.append(b)
    return out


def update_case(device, seed=31):
    """(opt, loss, static batch tensors, update): update() is one whole
    recurrent device update of the batch the static tensors hold."""
    import madrona_bots as mb
    rng = np.random.default_rng(seed)
    nets = [[au.make_net(mb, rng, 48, device, memory=True) for _ in range(4)] for _ in range(UP_G)]
    opt = mb.PolicyAdam(nets, lr=1e-2, max_grad_norm=0.25, weight_decay=0.01)
    s = {k: torch.from_numpy(v).to(device) for k, v in update_batches()[0].items()}
    rows = torch.zeros(UP_G, dtype=torch.int64, device=device)
    loss = torch.zeros(UP_G, dtype=torch.float64, device=device)

    def update():
        order, seg = mb.sequence_segments(s["net_id"], UP_G)
        outs = mb.evaluate_sequences_groups(nets, s["obs"], s["action"], s["length"], s["hidden0"], order, seg)
        rows.zero_()
        mb.sequence_group_rows(s["length"], s["t0"], s["end"], order, seg, rows, UP_LAST)
        opt.zero_grad()
        loss.zero_()
        g = mb.a2c_loss_sequences(*outs, s["adv"], s["ret"], s["length"], s["t0"], s["end"], order, seg, rows, UP_LAST,
                                  0.5, 0.01, loss=loss)
        torch.autograd.backward(list(outs), list(g[:3]))
        opt.step(rows)
    return opt, loss, s, update


def load(static, batch):
    for k, v in batch.items():
        static[k].copy_(torch.from_numpy(v))


def test_a_captured_update_replays_on_new_batches():
    """sequence_segments, evaluate_sequences_groups, the count, the loss, the
    backward, zero_grad and the clipped step recorded after one eager warm-up
    update and replayed on two further batches: three eager updates on the
    same batches, bit for bit, on the device and in CPU mode."""
    batches = update_batches()
    runs = {}
    for device in (DEV, "cpu"):
        opt, loss, static, update = update_case(device)
        for b in batches:
            load(static, b)
            update()
        runs[device] = ([p.detach().cpu().clone() for p in opt.params], opt.state_dict(), loss.cpu().clone(),
                        opt.grad_norm.cpu().clone())
    opt, loss, static, update = update_case(DEV)
    before = [p.detach().clone() for p in opt.params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        update()                                             # the warm call on batch 0: workspaces and .grad bindings
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        update()                                             # (recorded, not run)
    for b in batches[1:]:
        load(static, b)
        graph.replay()
    torch.cuda.synchronize()
    for which in (DEV, "cpu"):
        params, sd, want_loss, want_norm = runs[which]
        assert all(same(a.detach(), b) for a, b in zip(opt.params, params)), which
        assert all(same(a, b) if a.is_floating_point() else torch.equal(a.cpu(), b.cpu())
                   for a, b in zip(opt.state_dict().values(), sd.values())), which
        assert torch.equal(loss.cpu(), want_loss) and same(opt.grad_norm, want_norm), which
    assert opt.state_dict()["state"][:, 0].tolist() == [3, 3] and (opt.grad_norm > 0.25).all()
    assert sum(not torch.equal(a, b.detach()) for a, b in zip(before, opt.params)) >= len(before) // 2


# ---- the harness --------------------------------------------------------------------------------
def harness_run(exec_mode, device, gated, **kw):
    """harness/a2c_recurrent_groups.py: 64 worlds, four groups, two updates;
    the parameters before and after, and the losses."""
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c_recurrent
    import a2c_recurrent_groups
    sim = mb.SimManager(0, 64, 69, 8, exec_mode=exec_mode)
    modules = [a2c_recurrent.make_modules(H, device, 20 + i, gated) for i, H in enumerate((16, 32, 16, 32))]
    optimizers = None if kw.get("device_update") else \
        [[torch.optim.Adam(m.parameters(), lr=1e-3) for m in four] for four in modules]
    before = [p.detach().cpu().clone() for four in modules for m in four for p in m.parameters()]
    losses = a2c_recurrent_groups.train(sim, [0, 16, 32, 48], modules, optimizers, iters=2, horizon=4, lr=1e-3, **kw)
    after = [p.detach().cpu().clone() for four in modules for m in four for p in m.parameters()]
    return before, after, losses


@pytest.mark.parametrize("gated", (False, True), ids=("plain", "gated"))
def test_harness_device_update_leaves_the_cpu_mode_s_parameters(gated):
    """--device-update with clipping and weight decay, HIP mode against CPU
    mode: the same bits in every parameter and the same losses -- the
    end-to-end claim."""
    kw = dict(device_update=True, max_grad_norm=0.5, weight_decay=0.01)
    before, after, losses = harness_run("hip", DEV, gated, **kw)
    host_before, host_after, host_losses = harness_run("cpu", "cpu", gated, **kw)
    assert all(same(a, b) for a, b in zip(before, host_before))
    assert np.isfinite(losses).all() and losses == host_losses and len(losses) == 2 and len(losses[0]) == 4
    assert all(same(a, b) for a, b in zip(after, host_after))
    assert sum(not same(a, b) for a, b in zip(before, after)) >= len(before) // 2


def test_harness_without_device_update_is_unchanged():
    """device_update=False runs the code it ran before the device update
    existed: the per-net loop and --grouped-evaluate, which the suite equates
    in CPU mode (test_policy_seq_groups_cpu.py), leave the same bits in HIP
    mode too.  To compare with an earlier commit, check it out, run this
    function's two harness_run calls there and here, and compare
    hashlib.sha256 of the concatenated parameter bytes; no constant is kept
    here."""
    loop = harness_run("hip", DEV, True)
    grouped = harness_run("hip", DEV, True, grouped_evaluate=True)
    assert all(same(a, b) for a, b in zip(loop[0], grouped[0]))
    assert all(same(a, b) for a, b in zip(loop[1], grouped[1]))
    assert sum(not same(a, b) for a, b in zip(loop[0], loop[1])) >= len(loop[0]) // 2
