"""CPU mode: the gated memory head (DESIGN.md "Gated memory head") -- the
sigmoid, the two exact ends of the blend (an open gate is the ungated net, a
closed gate holds the state), act()'s and evaluate_sequences' bits, gradients
against a float64 restatement with torch's own f32 autograd as the yardstick,
the gradient's way across time and into the gate, padding / threads / empty
batches, the refusals, mixed gated and ungated policy groups, and the example
loop's --gated flag."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_ref as pr
import policy_grad_ref as gr
import policy_seq_ref as sr
import policy_gate_ref as gg
import policy_groups_util as pgu
import policy_seq_groups_util as psu
import test_policy_cpu as tpc
from policy_gate_ref import CASES, G, TILE, bits, same_bits, value_equal


def test_cases_are_the_issues():
    want = {(16, (3,), 1, 1, "full"), (16, (1, 2), 2, 63, "ragged"), (48, (4, 5, 3), 5, 64, "full"),
            (128, (0, 3, 1, 5), 5, 65, "ragged"), (128, (0, 3, 1), 2, 3 * 64 + 9, "tileshort"),
            (16, (2,), 2, 64 * 256 + 1, "wrapzero"), (16, (3, 1), 2, 64 * 256 + 1, "tilezero")}
    have = {(c[0], tuple(c[1]), c[3], c[4], c[5]) for c in CASES if "gate" not in c[2]}
    assert have == want
    assert sum("gate" in c[2] for c in CASES) == 1
    for c in CASES:
        net = gg.build(c)[0]
        assert (net["gate"][1] is None) == ("gate" in c[2])


# ---- 1. the sigmoid -----------------------------------------------------------------
def test_sigmoid():
    """Code 8 within test_policy_cpu's 4 ulp of float64 over its own sweep
    (measured: 2.27 ulp, DESIGN.md "Gated memory head"); exactly 1 at +200,
    exactly 0 at -200, 0.5 at +-0, NaN for NaN."""
    import madrona_bots as mb
    assert mb.ACTIVATIONS["Sigmoid"] == 8
    x = tpc.sweep()
    y = mb.policy_activation("Sigmoid", torch.from_numpy(x)).numpy()
    x64 = x.astype(np.float64)
    ref = np.where(x64 >= 0, 1.0 / (1.0 + np.exp(-np.abs(x64))), np.exp(-np.abs(x64)) / (1.0 + np.exp(-np.abs(x64))))
    e = tpc.ulps(y, ref)
    print(f"Sigmoid: max {e.max():.3f} ulp at x = {x[e.argmax()]!r}")
    assert e.max() <= 4.0, (e.max(), x[e.argmax()])
    edge = np.array([200.0, -200.0, 0.0, -0.0, np.nan, np.inf, -np.inf], np.float32)
    got = mb.policy_activation(8, torch.from_numpy(edge)).numpy()
    assert bits(got[:4]).tolist() == bits(np.array([1.0, 0.0, 0.5, 0.5], np.float32)).tolist()
    assert np.isnan(got[4]) and got[5] == 1.0 and got[6] == 0.0


# ---- 2. / 3. the two ends of the blend ------------------------------------------------
def act_pair(bias, exec_mode="cpu", case=("40x32", 48, 4, True, True)):
    """(twin manager with ungated nets, manager with the same nets behind a
    gate of zero weights and `bias`, the net dicts): 16 worlds, HiddenState
    nonzero from the synthetic actions."""
    import madrona_bots as mb

    def sim():
        s = mb.SimManager(0, 16, 77, 32, exec_mode=exec_mode)
        for t in range(3):
            s.write_synthetic_actions(4321, t, True)
            s.step()
        return s
    a, b = sim(), sim()
    nets = tpc.make_nets(case, pr.inputs(a, True))
    a.set_policy([gg.policy_net(n, a.device, False)[0] for n in nets])
    gated = [gg.const_gate(n, bias) for n in nets]
    b.set_policy([gg.policy_net(n, b.device, False)[0] for n in gated])
    return a, b, nets, gated


def test_open_gate_is_the_ungated_net_in_act():
    import madrona_bots as mb
    one = mb.policy_activation("Sigmoid", torch.tensor([200.0]))
    assert one.item() == 1.0 and bits(one.numpy())[0] == 0x3F800000
    twin, sim, _, _ = act_pair(200.0)
    assert np.abs(sim.hidden_state_tensor().to_torch().numpy()).max() > 0
    o_a, o_b = twin.act(), sim.act()
    pgu.assert_same_outputs(o_a, o_b, "open gate")
    h_a, h_b = (m.hidden_state_tensor().to_torch().numpy() for m in (twin, sim))
    assert value_equal(h_b, h_a)


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=gg.case_id)
def test_open_gate_is_the_ungated_net_in_evaluate_sequences(case):
    """Outputs and hidden as values (bit for bit where nonzero), every shared
    gradient equal as a value, the gate's gradients zero as values."""
    net, obs, action, length, hidden0, g = gg.build(case)
    plain = {k: v for k, v in net.items() if k != "gate"}
    a = gg.run_sequences(plain, obs, action, length, hidden0, g)
    b = gg.run_sequences(gg.const_gate(net, 200.0), obs, action, length, hidden0, g)
    for name, x, y in zip(("logp", "value", "entropy", "hidden"), a[:4], b[:4]):
        assert value_equal(y, x), name
    names = gg.param_names(net)
    for name, x, y in zip(names, a[4], b[4]):
        assert (x is None) == (y is None), name
        if x is not None:
            assert np.array_equal(x, y), (name, float(np.abs(x - y).max()))
    assert np.abs(a[4][names.index("memory.w")]).max() > 0
    gw, gb = b[4][names.index("gate.w")], b[4][names.index("gate.b")]
    assert not np.any(gw) and not np.any(gb)


def test_closed_gate_holds_the_state():
    _, sim, _, gated = act_pair(-200.0)
    before = sim.hidden_state_tensor().to_torch().numpy().copy()
    assert np.abs(before).max() > 0
    sim.act()
    assert value_equal(sim.hidden_state_tensor().to_torch().numpy(), before)
    net, obs, action, length, hidden0, g = gg.build(CASES[3])
    out = gg.run_sequences(gg.const_gate(net, -200.0), obs, action, length, hidden0, g)
    hidden = out[3]
    for k in range(obs.shape[0]):
        m = k < length
        assert value_equal(hidden[k][m], hidden0[m]), k
    names = gg.param_names(net)
    # z == 0: d mem_pre is zero, so the memory head receives no gradient at all
    assert not np.any(out[4][names.index("memory.w")]) and not np.any(out[4][names.index("memory.b")])


# ---- 4. forward bits ----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=gg.case_id)
def test_forward_is_evaluate_step_by_step(case):
    """logp, value and entropy are evaluate()'s bits on (obs[k], action[k],
    hidden[k]) at present elements and +0 elsewhere; h_0 is hidden0; h_{k+1}
    agrees with the float64 restatement of the gated step within 8 x torch
    f32's error on the same rows (the rule of tests/test_policy_seq_cpu.py)."""
    net, obs, action, length, hidden0, g = gg.build(case)
    L, B = obs.shape[:2]
    logp, value, entropy, hidden, _ = gg.run_sequences(net, obs, action, length, hidden0, g)
    p, _ = gg.policy_net(net)
    t = torch.from_numpy
    for k in range(L):
        m = k < length
        want = [o.detach().numpy() for o in p.evaluate(t(obs[k]), t(action[k]), t(hidden[k]))]
        for name, a, b in zip(("logp", "value", "entropy"), (logp, value, entropy), want):
            assert np.array_equal(bits(a[k][m]), bits(b[m])), (name, k)
            assert not bits(a[k][~m]).any(), (name, k)
        assert not bits(hidden[k][~m]).any()
        if k == 0:
            assert np.array_equal(bits(hidden[0][m]), bits(hidden0[m]))
        if k + 1 < L:
            m1 = k + 1 < length
            if m1.any():
                x = np.concatenate([obs[k], hidden[k]], axis=1)[m1]
                h64, h32 = gg.next_h(net, x, torch.float64), gg.next_h(net, x, torch.float32)
                yard = np.abs(h32 - h64).max()
                err = np.abs(hidden[k + 1][m1] - h64).max()
                print(f"k {k}: h error {err:.3g}, torch f32 {yard:.3g}")
                assert err <= 8 * yard


# ---- 5. the same bits as act() through the window ----------------------------------------
def rollout_through_window(exec_mode):
    """tests/test_policy_seq_cpu.py's rollout_through_window with four gated nets."""
    import madrona_bots as mb
    sim = mb.SimManager(0, 16, 77, 32, exec_mode=exec_mode, episode_length=7)
    for t in range(4):
        sim.write_synthetic_actions(4321, t, True)
        sim.step()
    case = ("40x32", 48, 4, True, True)
    rng = np.random.default_rng(77)
    nets = [gg.policy_net(gg.add_gate(rng, n), sim.device, False)[0]
            for n in tpc.make_nets(case, pr.inputs(sim, True))]
    sim.set_policy(nets)
    T = 6
    win = sim.trajectory_window(T, max_rows=sim.num_worlds * sim.agent_capacity, record_obs=True, record_state=True)
    keep = {"action": [], "logp": [], "value": [], "hidden": [], "species": []}
    for t in range(T):
        win.push()
        keep["hidden"].append(sim.hidden_state_tensor().to_torch().clone())
        o = sim.act()
        for k in ("action", "logp", "value"):
            keep[k].append(o[k])
        count = sim.species_count_tensor().to_torch().sum(dim=0).to(torch.int64)
        keep["species"].append(torch.repeat_interleave(torch.arange(4, device=count.device), count)
                               .to(torch.int32).reshape(-1, 1))
        if t + 1 < T:
            sim.step()
    win.compute(gamma=0.99)
    win.sequences()
    b = {k: v.clone() for k, v in win.batch().items()}
    got = {k: win.gather(v) for k, v in keep.items()}
    win.close()
    return nets, b, got


def check_window_bits(exec_mode):
    nets, b, got = rollout_through_window(exec_mode)
    L, B = b["rows"].shape
    length, end, t0 = b["len"].cpu().numpy(), b["end"].cpu().numpy(), b["t0"].cpu().numpy()
    sp = got["species"][0, :, 0].cpu().numpy()
    assert ((end == 1) & (t0 + length < L)).any(), "no sequence ends by death before the last table"
    assert (t0 > 0).any(), "no sequence starts after table 0"
    assert (end == 2).any(), "no sequence ends by reset"
    assert max(int((sp == s).sum()) for s in range(4)) > 64
    assert torch.equal(got["hidden"][0].view(torch.int32), b["hidden0"].view(torch.int32))
    present = (torch.arange(L, device=b["len"].device)[:, None] < b["len"][None, :])
    moved = 0
    for s in range(4):
        cols = torch.nonzero(got["species"][0, :, 0] == s).reshape(-1)
        take = lambda x: x.index_select(1, cols).contiguous()
        logp, value, _, hidden = nets[s].evaluate_sequences(take(b["obs"]), take(got["action"])[:, :, 0],
                                                            b["len"][cols], b["hidden0"][cols], return_hidden=True)
        m = take(present)
        for name, a, w in (("logp", logp, take(got["logp"])[:, :, 0]), ("value", value, take(got["value"])[:, :, 0]),
                           ("hidden", hidden, take(got["hidden"]))):
            assert torch.equal(a[m].view(torch.int32), w[m].view(torch.int32)), (name, s)
        moved += int((hidden[1:][m[1:]] != hidden[:-1][m[1:]]).sum())
    assert moved > 0                       # (the state is carried, not constant)


def test_same_bits_as_act_through_the_window():
    check_window_bits("cpu")


# ---- 6. gradients against float64 ------------------------------------------------------
def ratios(case, g=None):
    """[(name, error, torch f32's error)] of the outputs (from 63 elements on) and of every parameter's gradient."""
    net, obs, action, length, hidden0, g0 = gg.build(case)
    g = g0 if g is None else g
    ref = gg.evaluate_seq_torch(net, obs, action, length, hidden0, torch.float64, g)
    t32 = gg.evaluate_seq_torch(net, obs, action, length, hidden0, torch.float32, g)
    got = gg.run_sequences(net, obs, action, length, hidden0, g)
    names = ["logp", "value", "entropy", "hidden"] + gg.param_names(net)
    out = []
    for i, (name, a, b, c) in enumerate(zip(names, gg.flat(got), gg.flat(t32), gg.flat(ref))):
        if c is None:
            assert a is None
            continue
        assert a.shape == c.shape and a.dtype == np.float32
        if i < 4 and case[3] * case[4] < 63:
            continue
        err = float(np.abs(a.astype(np.float64) - c).max()) if a.size else 0.0
        yard = float(np.abs(b - c).max()) if a.size else 0.0
        out.append((name, err, yard))
    return out, got


def judge(rows):
    worst, failed = 0.0, []
    for name, err, yard in rows:
        ratio = err / yard if yard > 0 else (0.0 if err == 0 else np.inf)
        worst = max(worst, ratio)
        print(f"{name}: error {err:.3g}, torch f32 {yard:.3g}, ratio {ratio:.2f}")
        if not err <= 8.0 * yard:
            failed.append((name, err, yard))
    print(f"worst ratio {worst:.2f}")
    assert not failed, failed


@pytest.mark.parametrize("case", CASES, ids=gg.case_id)
def test_gradients_against_float64(case):
    """Per parameter tensor (the gate's included) the max-abs error against the
    float64 restatement is at most 8 x that of torch's own f32 autograd over
    the same chain; the outputs likewise from B L >= 63 on.  The worst ratio
    found is recorded in DESIGN.md "Gated memory head"."""
    rows, got = ratios(case)
    names = gg.param_names(gg.build(case)[0])
    assert ("gate.w" in names) and (got[4][names.index("gate.b")] is None) == ("gate" in case[2])
    judge(rows)


# ---- 7. the gradient crosses time, and reaches the gate ------------------------------------
def test_gradient_crosses_time_and_reaches_the_gate():
    case = CASES[3]
    net, obs, action, length, hidden0, _ = gg.build(case)
    L, B = obs.shape[:2]
    assert L == 5
    g = np.zeros((L, B), np.float32)
    cols = np.nonzero(length > 0)[0]
    g[length[cols] - 1, cols] = sr.dyadic(np.random.default_rng(5), len(cols), -7)
    rows, got = ratios(case, [g, None, None])
    grads = dict(zip(gg.param_names(net), got[4]))
    for name in ("gate.w", "gate.b", "memory.w", "memory.b"):
        assert np.abs(grads[name]).max() > 0, name
    assert np.abs(grads["trunk0.w"][:, 69:85]).max() > 0
    judge(rows)


def test_no_second_step_no_gate_gradient():
    case = CASES[3]
    net, obs, action, length, hidden0, g = gg.build(case)
    got = gg.run_sequences(net, obs, action, np.minimum(length, 1).astype(np.int32), hidden0, [g[2], g[2], g[2]])
    grads = dict(zip(gg.param_names(net), got[4]))
    for name in ("gate.w", "gate.b", "memory.w", "memory.b"):
        assert not bits(grads[name]).any(), name
    assert np.abs(grads["trunk0.w"]).max() > 0


# ---- 8. padding, threads, empty batches ----------------------------------------------------
@pytest.mark.parametrize("how", ["steps", "columns", "a tile of columns"])
def test_padding_changes_no_bit(how):
    case = CASES[4]
    net, obs, action, length, hidden0, g = gg.build(case)
    L, B = obs.shape[:2]
    base = gg.run_sequences(net, obs, action, length, hidden0, g)
    rng = np.random.default_rng(11)
    dl, db = (3, 0) if how == "steps" else (0, 1 if how == "columns" else TILE + 5)
    obs2 = np.abs(rng.normal(0.0, 30.0, (L + dl, B + db, 69))).astype(np.float32)
    act2 = rng.integers(0, 6, (L + dl, B + db)).astype(np.int32)
    hid2 = rng.uniform(-1, 1, (B + db, 16)).astype(np.float32)
    len2 = np.zeros(B + db, np.int32)
    g2 = [rng.uniform(-1, 1, (L + dl, B + db)).astype(np.float32) for _ in g]
    obs2[:L, :B], act2[:L, :B], hid2[:B], len2[:B] = obs, action, hidden0, length
    for a, b in zip(g2, g):
        a[:L, :B] = b
    more = gg.run_sequences(net, obs2, act2, len2, hid2, g2)
    assert same_bits(base[4], more[4])
    assert same_bits(base[:4], [q[:L, :B] for q in more[:4]])
    for q in more[:4]:
        assert not bits(q[L:]).any() and not bits(q[:, B:]).any()


def test_bits_do_not_depend_on_host_threads(monkeypatch):
    b = gg.build(CASES[5])            # accumulator 0 holds two tiles
    runs = []
    for threads in ("1", "3", "16"):
        monkeypatch.setenv("MBOTS_CPU_THREADS", threads)
        runs.append(gg.flat(gg.run_sequences(*b)))
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])


@pytest.mark.parametrize("L,B", [(0, 5), (3, 0), (0, 0)])
def test_empty_batches(L, B):
    net = gg.build(CASES[2])[0]
    p, ps = gg.policy_net(net)
    out = p.evaluate_sequences(torch.zeros(L, B, 69), torch.zeros(L, B, dtype=torch.int32),
                               torch.zeros(B, dtype=torch.int32), torch.zeros(B, 16), return_hidden=True)
    assert [tuple(o.shape) for o in out] == [(L, B)] * 3 + [(L, B, 16)]
    sum(o.sum() for o in out[:3]).backward()
    assert len(ps) == 2 * (3 + 4 + 2)
    assert all(q.grad is not None and not q.grad.any() for q in ps)


# ---- 9. refusals ----------------------------------------------------------------------------
def test_refusals():
    import madrona_bots as mb
    nn = torch.nn
    H = 32
    feature = lambda n_in=85: nn.Sequential(nn.Linear(n_in, H), nn.Tanh())
    actor = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 6))
    critic = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1))
    memory = nn.Sequential(nn.Linear(H, 16), nn.Tanh())
    gate = nn.Sequential(nn.Linear(H, 16), nn.Sigmoid())
    net = mb.PolicyNet.from_torch(feature(), actor, critic, memory, memory_in=True, gate=gate)
    assert net.gate is not None and tuple(net.gate[0].shape) == (16, H)
    with pytest.raises(ValueError, match="a gate needs a memory head and memory_in=True"):
        mb.PolicyNet.from_torch(feature(), actor, critic, None, memory_in=True, gate=gate)
    with pytest.raises(ValueError, match="a gate needs a memory head and memory_in=True"):
        mb.PolicyNet.from_torch(feature(69), actor, critic, memory, memory_in=False, gate=gate)
    with pytest.raises(ValueError, match="gate.*expected Linear\\(H, 16\\)"):
        mb.PolicyNet.from_torch(feature(), actor, critic, memory, True, nn.Sequential(nn.Linear(H, 8), nn.Sigmoid()))
    with pytest.raises(ValueError, match="gate: expected Linear\\(32, 16\\)"):
        mb.PolicyNet.from_torch(feature(), actor, critic, memory, True, nn.Sequential(nn.Linear(48, 16), nn.Sigmoid()))
    with pytest.raises(ValueError, match="gate\\[1\\] \\(Tanh\\)"):
        mb.PolicyNet.from_torch(feature(), actor, critic, memory, True, nn.Sequential(nn.Linear(H, 16), nn.Tanh()))
    with pytest.raises(ValueError, match="feature\\[1\\] \\(Sigmoid\\)"):
        mb.PolicyNet.from_torch(nn.Sequential(nn.Linear(85, H), nn.Sigmoid()), actor, critic, memory, True, gate)
    # the C ABI's own checks, through set_policy: a gate of another width
    sim = mb.SimManager(0, 2, 1, 4, exec_mode="cpu")
    w, b, c = net.gate
    net.gate = (torch.zeros(16, 48), b, c)
    with pytest.raises(RuntimeError, match="the gate head must be Linear\\(32, 16\\)"):
        sim.set_policy([net] * 4)
    net.gate = (torch.zeros(8, H), None, c)
    with pytest.raises(RuntimeError, match="the gate head must be Linear\\(32, 16\\)"):
        sim.set_policy([net] * 4)
    net.gate = (w, b, c)
    sim.set_policy([net] * 4)
    sim.act()
    # a parameter of another dtype, named
    net.gate = (w.detach().double(), b, c)
    with pytest.raises(ValueError, match="gate Linear weight must be float32"):
        net.evaluate_sequences(torch.zeros(1, 1, 69), torch.zeros(1, 1, dtype=torch.int32),
                               torch.ones(1, dtype=torch.int32), torch.zeros(1, 16))


# ---- 10. groups: gated and ungated nets side by side -----------------------------------------
GROUP_ARCH = [[(16, [3], True), (48, [4, 1], False), (128, [0, 3, 1], True), (16, [2], False)],
              [(128, [4, 2], False), (16, [1], True), None, (48, [5, 3], True)]]
GROUP_SIZES = [[65, 64, 63, 1], [130, 0, 7, 64]]          # columns per (group, species); (1, 2) has no net


def group_fixture():
    rng = np.random.default_rng(4242)
    probe = gr.net_input(*gr.random_rows(rng, 256, True)[:2])
    nets = []
    for four in GROUP_ARCH:
        row = []
        for a in four:
            if a is None:
                row.append(None)
                continue
            H, codes, gated = a
            n = pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, True, True, pr.in_scale(probe)), probe)
            row.append(gg.add_gate(rng, n) if gated else n)
        nets.append(row)
    ids = [4 * g + s for g in range(2) for s in range(4) for _ in range(GROUP_SIZES[g][s])] + [-1, 8, 99]
    net_id = np.asarray(ids, np.int32)[rng.permutation(len(ids))]
    L, B = 4, len(net_id)
    obs, _, action = gr.random_rows(rng, L * B, False)
    obs, action = np.ascontiguousarray(obs.reshape(L, B, 69)), np.ascontiguousarray(action.reshape(L, B))
    hidden0 = rng.uniform(-1.0, 1.0, (B, 16)).astype(np.float32)
    length = rng.integers(0, L + 1, B).astype(np.int32)
    g = [sr.dyadic(rng, (L, B), -int(np.ceil(np.log2(L * B)))) for _ in range(3)]
    return nets, net_id, obs, action, length, hidden0, g


def group_policy_nets(nets, device="cpu"):
    made = [[(None, None) if d is None else gg.policy_net(d, device) for d in four] for four in nets]
    return [[p for p, _ in four] for four in made], [[ps for _, ps in four] for four in made]


def test_grouped_sequences_mix_gated_and_ungated():
    """evaluate_sequences_groups over two groups whose nets are gated or not,
    with different H, equals the per-net evaluate_sequences calls bit for bit:
    outputs, hidden and every gradient (the gates' included)."""
    fx = group_fixture()
    nets = fx[0]
    assert any(d is not None and "gate" in d for four in nets for d in four)
    assert any(d is not None and "gate" not in d for four in nets for d in four)
    loop = psu.run_loop(*fx, pn_params=group_policy_nets(nets))
    pn, params = group_policy_nets(nets)
    grouped = psu.run_grouped(*fx, pn_params=(pn, params))
    psu.assert_same(loop, grouped, "mixed groups")
    assert len(params[0][0]) == 2 * (1 + 4 + 2) and len(params[0][1]) == 2 * (2 + 4 + 1)
    assert all(q.grad is not None and q.grad.abs().max() > 0 for q in params[0][0][-2:])     # a gate's gradients


def test_act_with_mixed_groups_is_the_one_group_managers():
    """act() on a two-group manager whose groups hold gated and ungated nets
    equals, per group's worlds, a one-group manager of that group's nets."""
    import madrona_bots as mb
    starts = [0, 7]

    def sim():
        s = mb.SimManager(0, 16, 77, 32, exec_mode="cpu")
        for t in range(3):
            s.write_synthetic_actions(4321, t, True)
            s.step()
        return s
    both, ones = sim(), [sim(), sim()]
    x = pr.inputs(both, True)
    rng = np.random.default_rng(8)
    mk = lambda H, codes: pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, True, True, pr.in_scale(x)), x)
    dicts = [[gg.add_gate(rng, mk(48, [3, 1])), mk(16, [4]), gg.add_gate(rng, mk(128, [0, 2, 5])), mk(48, [1])],
             [mk(128, [4, 4]), gg.add_gate(rng, mk(16, [2])), mk(16, [3]), gg.add_gate(rng, mk(128, [1, 3, 0, 5]))]]
    both.set_policy_groups(starts)
    for u in range(2):
        both.set_policy([gg.policy_net(d, "cpu", False)[0] for d in dicts[u]], group=u)
        ones[u].set_policy([gg.policy_net(d, "cpu", False)[0] for d in dicts[u]])
    o = both.act()
    want = [m.act() for m in ones]
    sc = both.species_count_tensor().to_torch().numpy()
    gw, _, _ = pr.row_keys(sc)
    grp = pgu.world_group(starts, gw)
    assert set(grp.tolist()) == {0, 1}
    hid = both.hidden_state_tensor().to_torch().numpy()
    for u in range(2):
        rows = np.nonzero(grp == u)[0]
        for k in ("action", "logp", "value"):
            assert np.array_equal(pgu.bits(o[k])[rows], pgu.bits(want[u][k])[rows]), (u, k)
        assert np.array_equal(bits(hid[rows]), bits(ones[u].hidden_state_tensor().to_torch().numpy()[rows])), u


# ---- 11. the example loop --------------------------------------------------------------------
def harness():
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c_recurrent
    return mb, a2c_recurrent


def test_example_loop_trains_the_gate_and_the_default_is_unchanged():
    mb, a2c_recurrent = harness()

    def run(gated):
        sim = mb.SimManager(0, 16, 69, 8, exec_mode="cpu")
        modules = a2c_recurrent.make_modules(16, "cpu", seed=1, gated=gated) if gated is not None \
            else a2c_recurrent.make_modules(16, "cpu", seed=1)
        before = [[q.detach().clone() for q in m.parameters()] for m in modules]
        optimizers = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in modules]
        losses = a2c_recurrent.train(sim, modules, optimizers, iters=3, horizon=5)
        return modules, before, losses
    modules, before, losses = run(True)
    assert len(losses) == 3 and all(np.isfinite(losses))
    for m, b in zip(modules, before):
        assert "gate" in m
        gate_before = b[-2:]
        for q, q0 in zip(m["gate"].parameters(), gate_before):
            assert torch.isfinite(q).all() and not torch.equal(q.detach(), q0)
    # the default path: no gate module, and the same bits whether the flag's argument is passed or not
    plain, _, l0 = run(False)
    again, _, l1 = run(None)
    assert all("gate" not in m for m in plain)
    assert np.array_equal(np.array(l0, np.float64).view(np.uint64), np.array(l1, np.float64).view(np.uint64))
    for a, b in zip(plain, again):
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))


def test_example_loop_command_line_takes_gated():
    mb, _ = harness()
    script = os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness", "a2c_recurrent.py")
    out = subprocess.run([sys.executable, script, "--gated", "--exec-mode", "cpu", "--worlds", "8", "--agents", "8",
                          "--iters", "2", "--horizon", "4", "--hidden", "16"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.count('"loss"') == 2
