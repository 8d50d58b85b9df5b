"""The device learner step on host tensors (DESIGN.md "Device learner step"):
mbots_policy_adam and mbots_policy_a2c_loss against their float32 restatement
bit for bit and against float64 within a derived bound, the wrappers'
refusals, and harness/a2c_groups.py --device-update.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import policy_adam_ref as ar
import policy_adam_util as u
import policy_grad_ref as gr
import test_policy_grad_cpu as tg


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def t(a, device="cpu"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


@pytest.fixture(scope="module")
def adam_run():
    import madrona_bots as mb
    return u.run_adam(mb, "cpu")


# ---- 1. Adam, bit for bit ---------------------------------------------------------------------
def test_adam_case_covers_the_lengths_and_paths(adam_run):
    opt = adam_run[0]
    lengths = {p.numel() for p in opt.params}
    assert lengths >= {1, 6, 16, 16 * 69, 48 * 85}
    assert len(opt.params) > 64 and opt.groups == u.GROUPS                    # more than one launch's descriptors
    assert sum(p.data_ptr() % 16 != 0 for p in opt.params) == 1             # the 4-byte offset view
    assert all((opt._m.data_ptr() + 4 * o) % 16 == 0 for o in opt.offsets)
    shared = [i for i, g in enumerate(opt.param_group) if g == u.SHARED_GROUP]
    assert len(shared) == 10                                                 # one net's tensors, once, not four times


def test_adam_three_steps_equal_the_float32_restatement(adam_run):
    """Every param, m, v and state after each of three steps; the group with
    rows == 0 untouched with t == 0; a parameter without .grad passed over."""
    opt, before, trace = adam_run
    rows = u.rows_of("cpu").tolist()
    P = [b.numpy().copy() for b in before]
    M, V = [np.zeros_like(a) for a in P], [np.zeros_like(a) for a in P]
    state = ar.adam_state(u.GROUPS)
    for k, (params, sd) in enumerate(trace):
        G = u.gradients(opt, k)
        ar.adam_f32([(P[i], G[i], M[i], V[i], opt.param_group[i]) for i in range(len(P))], state, rows, **u.HYPER)
        got_m, got_v = u.slices(opt, sd["m"]), u.slices(opt, sd["v"])
        for i in range(len(P)):
            where = f"step {k}, {opt.names[i]}"
            assert np.array_equal(bits(params[i].numpy()), bits(P[i])), where
            assert np.array_equal(bits(got_m[i]), bits(M[i])) and np.array_equal(bits(got_v[i]), bits(V[i])), where
        st = sd["state"].numpy()
        for g, (tt, b1t, b2t) in enumerate(state):
            assert st[g].tolist() == [tt, int(np.float32(b1t).view(np.int32)), int(np.float32(b2t).view(np.int32))]
    st = trace[-1][1]["state"].numpy()
    assert st[u.IDLE_GROUP].tolist() == [0, 0x3F800000, 0x3F800000] and st[0, 0] == u.STEPS
    idle = [i for i, g in enumerate(opt.param_group) if g == u.IDLE_GROUP]
    assert idle and all(torch.equal(trace[-1][0][i].view(torch.int32), before[i].view(torch.int32)) for i in idle)
    assert all(not u.slices(opt, trace[-1][1]["m"])[i].any() for i in idle)
    moved = [i for i, g in enumerate(opt.param_group) if g != u.IDLE_GROUP and i > 1]      # (0: zeros, 1: tiny)
    assert all(not torch.equal(trace[0][0][i], before[i]) for i in moved)
    assert torch.equal(trace[0][0][0], before[0])                             # the all-zero gradient: no move


def test_adam_against_float64(adam_run):
    """After one step from the common f32 state |p' - p'_64| <= 2 (2^-24 |p'| +
    16 * 2^-24 |delta_64|): one rounding of p' and the nine of delta, with a
    margin of two."""
    opt, before, trace = adam_run
    G = u.gradients(opt, 0)
    worst = 0.0
    for i, p0 in enumerate(before):
        if opt.param_group[i] == u.IDLE_GROUP:
            continue
        z = np.zeros_like(p0.numpy())
        want, delta = ar.adam_f64(p0.numpy(), G[i], z, z, 0, **u.HYPER)
        got = trace[0][0][i].numpy().astype(np.float64)
        bound = 2.0 * (2.0 ** -24 * np.abs(got) + 16.0 * 2.0 ** -24 * np.abs(delta))
        err = np.abs(got - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
        assert (err <= bound).all(), opt.names[i]
    print(f"worst error / bound: {worst:.3f}")


def test_adam_shared_tensors_and_refusals():
    import madrona_bots as mb
    rng = np.random.default_rng(0)
    a, b = u.make_net(mb, rng, 16, "cpu"), u.make_net(mb, rng, 16, "cpu")
    with pytest.raises(ValueError, match=r"nets\[1\]\[0\].*feature Linear 0 weight.*nets\[0\]\[0\].*shared across groups"):
        mb.PolicyAdam([[a] * 4, [a, b, b, b]])
    assert len(mb.PolicyAdam([a, b, a, b]).params) == 20 and mb.PolicyAdam(a).groups == 1   # flat four / one net: a group
    frozen = u.make_net(mb, rng, 16, "cpu")
    for w, bb, _ in frozen.trunk + frozen.actor:
        w.requires_grad_(False), bb.requires_grad_(False)
    opt = mb.PolicyAdam([frozen])
    assert len(opt.params) == 4                                               # the critic's, requires_grad only
    with pytest.raises(ValueError, match="rows must be"):
        opt.step(torch.zeros(2, dtype=torch.int64))
    opt.zero_grad()
    assert all(p.grad is not None and not p.grad.any() for p in opt.params)
    ptrs = [p.grad.data_ptr() for p in opt.params]
    for p in opt.params:
        p.grad.add_(1.0)
    opt.step()
    sd = opt.state_dict()
    assert sd["state"][0, 0] == 1 and sd["m"].any()
    opt.zero_grad()
    assert ptrs == [p.grad.data_ptr() for p in opt.params] and all(not p.grad.any() for p in opt.params)
    other = mb.PolicyAdam([frozen])
    other.load_state_dict(sd)
    assert all(torch.equal(x, y) for x, y in zip(other.state_dict().values(), sd.values()))
    with pytest.raises(ValueError, match="state_dict"):
        mb.PolicyAdam(a).load_state_dict(sd)


# ---- 2. the loss ------------------------------------------------------------------------------
def run_loss(device, end=True, loss=None):
    import madrona_bots as mb
    cols, e, segments, rows = u.loss_case()
    got = mb.a2c_loss_groups(*[t(c, device) for c in cols], t(e, device) if end else None, t(segments, device),
                             t(rows, device), 0.5, 0.01, loss=loss)
    return [x.cpu().numpy() for x in got]


@pytest.mark.parametrize("end", (True, False), ids=("end", "no-end"))
def test_loss_equals_the_float32_restatement(end):
    cols, e, segments, rows = u.loss_case()
    assert (e == ar.END_RESET).sum() > 100 and {257, 1, 0, 512, 1298} <= {int(b - a) for a, b in segments.reshape(-1, 2)}
    want = ar.loss_f32(*cols, e if end else None, segments, rows, 0.5, 0.01)
    got = run_loss("cpu", end)
    for name, a, b in zip(("g_logp", "g_value", "g_entropy"), got, want):
        assert np.array_equal(bits(a), bits(b)), name
    assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))
    assert got[3][0] != 0 and got[3][1] != 0 and got[3][2] == 0               # rows == 0: scale 0
    outside = np.ones(u.LOSS_N, bool)
    for a, b in segments.reshape(-1, 2):
        outside[a:b] = False
    assert outside.sum() > 300 and all(not bits(x)[outside].any() for x in got[:3])     # +0, not -0
    assert all(not x[2200:2260].any() for x in got[:3])
    if end:
        assert all(not x[e == ar.END_RESET].any() for x in got[:3])
    # and the distance to float64: a per_row value carries at most 7 roundings of its terms' sizes, the f64 sums
    # none worth counting
    ref = ar.loss_f64(*cols, e if end else None, segments, rows, 0.5, 0.01)
    c = [np.abs(a.astype(np.float64)) for a in cols]
    size = np.zeros(u.LOSS_G)
    for g in range(u.LOSS_G):
        for a, b in segments[g]:
            d = c[1][a:b] + c[4][a:b]
            size[g] += float(np.sum(c[3][a:b] * c[0][a:b] + 0.5 * d * d + 0.01 * c[2][a:b])) / max(int(rows[g]), 1)
    assert (np.abs(got[3] - ref[3]) <= 8 * 2.0 ** -24 * size).all()


def test_loss_accumulates_and_group_rows_add_up_over_two_tables():
    import madrona_bots as mb
    cols, e, segments, rows = u.loss_case()
    once = run_loss("cpu")[3]
    twice = run_loss("cpu", loss=t(once.copy()))[3]
    want = ar.loss_f32(*cols, e, segments, rows, 0.5, 0.01, loss=once)[3]
    assert np.array_equal(twice.view(np.uint64), want.view(np.uint64)) and not np.array_equal(once, twice)
    total = torch.zeros(u.LOSS_G, dtype=torch.int64)
    assert mb.policy_group_rows(t(segments), total) is total
    assert total.tolist() == [299, 1840, 60]
    other = segments.copy()
    other[0] = [[0, 5], [5, 5], [5, 7], [7, 7]]
    mb.policy_group_rows(t(other), total)
    assert total.tolist() == [299 + 7, 2 * 1840, 2 * 60]


def test_loss_refusals():
    import madrona_bots as mb
    cols, e, segments, rows = u.loss_case()
    args = [t(c) for c in cols] + [t(e)]
    for bad, what in (([[0, 257], [256, 300]], "overlap"), ([[0, 257], [2500, 2601]], "not inside"),
                      ([[0, 257], [300, 299]], "not inside")):
        s = segments.copy()
        s[0, :2] = bad
        with pytest.raises(RuntimeError, match=what):
            mb.a2c_loss_groups(*args, t(s), t(rows))
    with pytest.raises(RuntimeError, match="no row range"):
        s = segments.copy()
        s[2, 0] = [5, 4]
        mb.policy_group_rows(t(s), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="rows must be"):
        mb.a2c_loss_groups(*args, t(segments), t(rows.astype(np.int32)))
    with pytest.raises(ValueError, match="adv must be"):
        mb.a2c_loss_groups(*args[:3], args[3][:5], args[4], args[5], t(segments), t(rows))
    with pytest.raises(ValueError, match="loss must be"):
        mb.a2c_loss_groups(*args, t(segments), t(rows), loss=torch.zeros(3))


def test_backward_with_the_loss_gradients_against_torch_autograd():
    """autograd.backward with a2c_loss_groups' g_* against torch autograd of the
    harness's loss expression in float64: per parameter tensor the error is at
    most 8 x that of torch's own float32 autograd -- the yardstick of
    test_policy_grad_cpu.test_gradients_against_float64, on one of its cases.
    The critic's last bias is left out of the net: its gradient is the plain
    sum of g_value, one number, for which the yardstick would compare two
    single roundings (that test's dyadic upstream gradients avoid the same;
    here g_value follows from the value head and cannot be chosen)."""
    import madrona_bots as mb
    case = tg.CASES[5]                                                        # H = 128, two layers, 201 rows
    net, obs, hidden, action, _ = tg.build(case)
    net = gr.strip_biases(net, ("critic1",))
    n = case[5]
    rng = np.random.default_rng(5)
    adv, ret = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    end = np.where(rng.random(n) < 0.1, ar.END_RESET, 0).astype(np.int32)
    keep = (end != ar.END_RESET)

    def torch_grads(dtype):
        lv = [torch.from_numpy(a).to(dtype).requires_grad_() for a in gr.evaluate_torch(net, obs, action, dtype)[:3]]
        a, r, k = (torch.from_numpy(x).to(dtype) for x in (adv, ret, keep))
        per_row = -a * lv[0] + 0.5 * (lv[1] - r) ** 2 - 0.01 * lv[2]           # harness/a2c_groups.py's expression
        g = torch.autograd.grad((per_row * k).sum() / n, lv)
        return gr.evaluate_torch(net, obs, action, dtype, [x.numpy() for x in g])[3]
    ref, t32 = torch_grads(torch.float64), torch_grads(torch.float32)
    p, ps = gr.policy_net(net)
    outs = p.evaluate(t(obs), t(action))
    segments = torch.tensor([[[0, n], [n, n], [n, n], [n, n]]], dtype=torch.int32)
    g = mb.a2c_loss_groups(*outs, t(adv), t(ret), t(end), segments, torch.tensor([n]), 0.5, 0.01)
    torch.autograd.backward(list(outs), list(g[:3]))
    failed = []
    for name, q, b, c in zip(gr.param_names(net), ps, t32, ref):
        if c is None:
            continue
        err, yard = float(np.abs(q.grad.numpy() - c).max()), float(np.abs(b - c).max())
        print(f"{name}: error {err:.3g}, torch f32 {yard:.3g}, scale {float(np.abs(c).max()):.3g}")
        if not err <= 8.0 * yard:
            failed.append((name, err, yard))
    assert not failed, failed


# ---- 3. the harness ---------------------------------------------------------------------------
def harness_run(exec_mode, device):
    """harness/a2c_groups.py --device-update: 64 worlds, four groups -- the
    last one's range starts past the manager's worlds, so it never has a row --
    two updates; the parameters before and after, and the losses."""
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c
    import a2c_groups
    sim = mb.SimManager(0, 64, 69, 8, exec_mode=exec_mode)
    modules = [a2c.make_modules(H, device, seed=20 + i) for i, H in enumerate((16, 32, 16, 32))]
    before = [[p.detach().cpu().clone() for m in four for p in m.parameters()] for four in modules]
    losses = a2c_groups.train(sim, [0, 21, 42, 64], modules, None, iters=2, horizon=4, device_update=True, lr=1e-3)
    after = [[p.detach().cpu().clone() for m in four for p in m.parameters()] for four in modules]
    return before, after, losses


def test_harness_device_update_is_reproducible_and_leaves_an_empty_group_alone():
    runs = [harness_run("cpu", "cpu") for _ in range(2)]
    before, after, losses = runs[0]
    assert len(losses) == 2 and len(losses[0]) == 4 and np.isfinite(losses).all()
    assert all(l[3] == 0.0 and l[0] != 0.0 for l in losses)
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(same(a, b) for a, b in zip(before[3], after[3]))               # the group without worlds
    for g in range(3):
        assert sum(not same(a, b) for a, b in zip(before[g], after[g])) >= len(before[g]) // 2
    assert all(same(a, b) for g in range(4) for a, b in zip(after[g], runs[1][1][g]))
    assert losses == runs[1][2]


def test_harness_a2c_device_update_runs():
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c
    sim = mb.SimManager(0, 8, 69, 8, exec_mode="cpu")
    modules = a2c.make_modules(16, "cpu", seed=3)
    before = [p.detach().clone() for m in modules for p in m.parameters()]
    losses = a2c.train(sim, modules, None, iters=2, horizon=4, device_update=True)
    assert len(losses) == 2 and np.isfinite(losses).all()
    after = [p.detach() for m in modules for p in m.parameters()]
    assert sum(not torch.equal(a, b) for a, b in zip(before, after)) >= len(before) // 2
