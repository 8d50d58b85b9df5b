"""CPU mode: PolicyNet.evaluate and its backward pass (DESIGN.md
"Differentiable evaluate"; mbots_policy_eval / mbots_policy_grad) -- the same
bits as act(), gradients against float64 autograd with torch's own f32
autograd as the yardstick, independence of the host's thread count and of
zero-weight rows, the refusals, and the example loop of harness/a2c.py."""
import os
import sys

import numpy as np
import pytest
import torch

import policy_ref as pr
import policy_grad_ref as gr
import test_policy_cpu as tpc

G = 256                      # kPolGradAcc
TILE = 64                    # kPolGradRows
# (H, trunk codes, memory_in, memory head, layers without a bias, n, which of g_logp / g_value / g_entropy)
CASES = [
    (16, [3], False, False, (), 0, "lve"),
    (16, [1, 2], True, False, (), 1, "lve"),
    (48, [4, 5, 3], False, True, (), 63, "l"),
    (128, [0, 3, 1, 5], True, True, (), 64, "v"),
    (128, [0, 3, 1], False, False, ("trunk1", "actor1"), 65, "e"),
    (128, [4, 2], False, False, (), 3 * TILE + 9, "lve"),
    (48, [2, 4], True, False, (), TILE * G - 1, "lve"),
    (16, [5, 1, 4, 2], False, False, ("critic0",), TILE * G + 1, "lve"),
    (48, [3], False, False, ("trunk0",), 3 * TILE * G + 17, "lve"),
]


def case_id(c):
    return f"H{c[0]}-d{len(c[1])}-{'min' if c[2] else 'nomin'}-{'mem' if c[3] else 'nomem'}-n{c[5]}-{c[6]}"


def test_cases_cover_the_grid():
    assert {c[0] for c in CASES} == {16, 48, 128} and {len(c[1]) for c in CASES} == {1, 2, 3, 4}
    assert {a for c in CASES for a in c[1]} >= {1, 2, 3, 4, 5}
    assert {c[2] for c in CASES} == {False, True} and any(c[3] for c in CASES) and any(c[4] for c in CASES)
    assert {c[6] for c in CASES} >= {"l", "v", "e", "lve"}
    assert {c[5] for c in CASES} >= {0, 1, 63, 64, 65, TILE * G - 1, TILE * G + 1, 3 * TILE * G + 17}
    assert all(c[0] <= 48 for c in CASES if c[5] > TILE * G)


def dyadic(rng, n, scale_log2):
    """Multiples of 2^-8 in [-1, 1] times 2^scale_log2: any sum of up to 2^15
    of them is exact in f32 in any order.  The gradient of the critic's last
    bias is the plain sum of g_value -- one number, whose error against torch's
    pairwise sum would compare two single roundings; with these weights both
    are exact, and every other gradient still rounds at every step."""
    return (rng.integers(-256, 257, n).astype(np.float32) / np.float32(256.0)) * np.float32(2.0 ** scale_log2)


def build(case, seed=0):
    """The case's net, rows and upstream gradients (None where the case leaves one out)."""
    H, codes, mi, mh, nobias, n, which = case
    rng = np.random.default_rng(4000 + CASES.index(case) + 100 * seed)
    probe = gr.net_input(*gr.random_rows(rng, 256, mi)[:2])
    net = pr.calibrate_actor(pr.make_net(rng, H, len(codes), codes, mi, mh, pr.in_scale(probe)), probe)
    net = gr.strip_biases(net, nobias)
    obs, hidden, action = gr.random_rows(rng, n + n // 2 + 64, mi)
    ok = np.nonzero(gr.away_from_kinks(net, gr.net_input(obs, hidden)))[0][:n]   # (see its docstring)
    assert len(ok) == n
    obs, hidden, action = obs[ok], None if hidden is None else hidden[ok], action[ok]
    s = -int(np.ceil(np.log2(max(n, 1))))
    g = [dyadic(rng, n, s) if k in which else None for k in "lve"]
    return net, obs, hidden, action, g


def run_evaluate(net, obs, hidden, action, g, device="cpu"):
    """(logp, value, entropy, grads in gr.param_names() order) of the library, as numpy."""
    p, ps = gr.policy_net(net, device)
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)
    out = p.evaluate(t(obs), t(action), t(hidden))
    terms = [(t(gi) * o).sum() for gi, o in zip(g, out) if gi is not None]
    sum(terms).backward()
    grads = [None if q is None else (torch.zeros_like(q) if q.grad is None else q.grad).cpu().numpy() for q in ps]
    if p.memory is not None:
        assert p.memory[0].grad is None and p.memory[1].grad is None     # the memory head takes no part
    return tuple(o.detach().cpu().numpy() for o in out) + (grads,)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---- 1. the same bits as act() ------------------------------------------------
@pytest.mark.parametrize("case", tpc.GRID, ids=tpc.grid_id)
def test_evaluate_reproduces_act_bitwise(case):
    sim = tpc.make_sim(case)
    nets = [pr.policy_net(n) for n in tpc.make_nets(case, pr.inputs(sim, case[3]))]
    sim.set_policy(nets)
    o = sim.act(write=False)
    obs, hidden = sim.construct_obs(), sim.hidden_state_tensor().to_torch()
    end = np.cumsum(sim.species_count_tensor().to_torch().numpy().sum(axis=0))
    lo = 0
    for s in range(4):
        hi = int(end[s])
        logp, value, entropy = nets[s].evaluate(obs[lo:hi], o["action"][lo:hi], hidden[lo:hi] if case[3] else None)
        assert torch.equal(logp.view(torch.int32), o["logp"][lo:hi, 0].view(torch.int32))
        assert torch.equal(value.view(torch.int32), o["value"][lo:hi, 0].view(torch.int32))
        assert entropy.shape == (hi - lo,) and bool(((entropy > 0) & (entropy <= np.log(6.0) + 1e-5)).all())
        lo = hi
    assert lo == sim.num_agents()


# ---- 2. gradients, logp and entropy against float64 -------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradients_against_float64(case):
    """Per parameter tensor the max-abs error against float64 autograd is at
    most 8 x that of torch's own f32 autograd; logp, value and entropy
    likewise (from 63 rows on).  Measured: worst ratio 3.91, recorded in
    DESIGN.md "Differentiable evaluate" with what the rows and the upstream
    gradients are chosen to avoid (ReLU kinks, a one-number sum)."""
    net, obs, hidden, action, g = build(case)
    x = gr.net_input(obs, hidden)
    ref = gr.evaluate_torch(net, x, action, torch.float64, g)
    t32 = gr.evaluate_torch(net, x, action, torch.float32, g)
    got = run_evaluate(net, obs, hidden, action, g)
    worst = 0.0
    failed = []
    # (logp, value and entropy are judged from 63 rows on: over a single row the
    # ratio would compare one rounding of the library's with one of torch's)
    outputs = list(zip(("logp", "value", "entropy"), got[:3], t32[:3], ref[:3])) if case[5] >= 63 else []
    for name, a, b, c in outputs + list(zip(gr.param_names(net), got[3], t32[3], ref[3])):
        if c is None:
            assert a is None
            continue
        assert a.shape == c.shape and a.dtype == np.float32
        err = float(np.abs(a.astype(np.float64) - c).max()) if a.size else 0.0
        yard = float(np.abs(b - c).max()) if a.size else 0.0
        ratio = err / yard if yard > 0 else (0.0 if err == 0 else np.inf)
        worst = max(worst, ratio)
        print(f"{name}: error {err:.3g}, torch f32 {yard:.3g}, ratio {ratio:.2f}, scale {float(np.abs(c).max()) if a.size else 0:.3g}")
        if not err <= 8.0 * yard:
            failed.append((name, err, yard))
    print(f"worst ratio {worst:.2f}")
    assert not failed, failed
    if case[5] == 0:
        assert all(q is None or not q.any() for q in got[3])


def test_each_upstream_gradient_alone_adds_up():
    """g_logp, g_value and g_entropy alone: the three gradients sum to the
    joint one up to rounding, and an absent g_* equals a zero one bitwise."""
    case = CASES[5]
    net, obs, hidden, action, g = build(case)
    joint = run_evaluate(net, obs, hidden, action, g)[3]
    alone = [run_evaluate(net, obs, hidden, action, [gi if i == k else None for i, gi in enumerate(g)])[3]
             for k in range(3)]
    zeros = run_evaluate(net, obs, hidden, action, [g[0], np.zeros_like(g[1]), np.zeros_like(g[2])])[3]
    assert same_bits(alone[0], zeros)
    for j, a, b, c in zip(joint, *alone):
        s = a.astype(np.float64) + b + c
        assert np.abs(s - j).max() <= 1e-5 * max(np.abs(j).max(), 1e-6)
    assert all(np.abs(a[-1]).max() == 0 for a in (alone[0], alone[2]))   # critic bias: g_value only
    assert all(np.abs(alone[1][i]).max() == 0 for i in range(len(joint) - 8, len(joint) - 4))   # actor: never g_value


# ---- 3. order independence ----------------------------------------------------
def test_bits_do_not_depend_on_host_threads(monkeypatch):
    case = CASES[7]           # accumulators holding two tiles
    net, obs, hidden, action, g = build(case)
    runs = []
    for threads in ("1", "5", "16"):
        monkeypatch.setenv("MBOTS_CPU_THREADS", threads)
        o = run_evaluate(net, obs, hidden, action, g)
        runs.append(list(o[:3]) + o[3])
    assert same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])


@pytest.mark.parametrize("extra", [1, TILE, 2 * TILE * G + 5])
def test_zero_weight_rows_change_nothing(extra):
    case = CASES[5]
    net, obs, hidden, action, g = build(case)
    base = run_evaluate(net, obs, hidden, action, g)
    rng = np.random.default_rng(9)
    o2, _, a2 = gr.random_rows(rng, extra, False)
    more = run_evaluate(net, np.concatenate([obs, o2]), None, np.concatenate([action, a2]),
                        [np.concatenate([gi, np.zeros(extra, np.float32)]) for gi in g])
    assert same_bits(base[3], more[3])
    n = len(obs)
    assert same_bits(base[:3], [q[:n] for q in more[:3]])


# ---- 4. refusals ----------------------------------------------------------------
def test_refusals():
    net, obs, hidden, action, g = build(CASES[1])      # a memory_in net
    net2, obs2, hidden2, action2, _ = build(CASES[5])
    obs2, action2 = obs2[:8], action2[:8]
    p, ps = gr.policy_net(net2)
    t = torch.from_numpy
    with pytest.raises(ValueError, match="obs must be float32"):
        p.evaluate(t(obs2).double(), t(action2))
    with pytest.raises(ValueError, match="obs must be float32"):
        p.evaluate(t(obs2)[:, :68], t(action2))
    with pytest.raises(ValueError, match="action must be int32"):
        p.evaluate(t(obs2), t(action2).long())
    with pytest.raises(ValueError, match="action must be int32"):
        p.evaluate(t(obs2), t(action2)[:5])
    for bad in (6, -1):
        a = action2.copy()
        a[3] = bad
        with pytest.raises(RuntimeError, match="outside 0..5"):
            p.evaluate(t(obs2), t(a))
    pm, _ = gr.policy_net(net)
    with pytest.raises(ValueError, match="needs hidden"):
        pm.evaluate(t(obs), t(action))
    with pytest.raises(ValueError, match="hidden must be float32"):
        pm.evaluate(t(obs), t(action), t(hidden)[:, :8])
    # a parameter of another dtype, named
    w, b, c = p.trunk[1]
    p.trunk[1] = (w.detach().double(), b, c)
    with pytest.raises(ValueError, match="feature Linear 1 weight must be float32"):
        p.evaluate(t(obs2), t(action2))
    p.trunk[1] = (w.detach().to("meta"), b, c)
    with pytest.raises(ValueError, match="feature Linear 1 weight must be float32 on cpu"):
        p.evaluate(t(obs2), t(action2))
    p.trunk[1] = (w, b, c)
    # gradients only where asked, and [n, 1] actions as act() returns them
    ps[0].requires_grad_(False)
    out = p.evaluate(t(obs2), t(action2).reshape(-1, 1))
    out[0].sum().backward()
    assert ps[0].grad is None and ps[2].grad is not None and ps[-1].grad is not None and not ps[-1].grad.any()


# ---- 5. the example loop ---------------------------------------------------------
def test_a2c_example_loop_runs_and_learns_something():
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c
    sim = mb.SimManager(0, 4, 69, 8, exec_mode="cpu")
    modules = a2c.make_modules(16, "cpu", seed=1)
    before = [p.detach().clone() for m in modules for p in m.parameters()]
    optimizers = [torch.optim.Adam(m.parameters(), lr=1e-3) for m in modules]
    losses = a2c.train(sim, modules, optimizers, iters=3, horizon=4)
    assert len(losses) == 3 and all(np.isfinite(losses))
    after = [p.detach() for m in modules for p in m.parameters()]
    assert all(torch.isfinite(q).all() for q in after)
    assert sum(not torch.equal(a, b) for a, b in zip(before, after)) >= len(before) // 2
