"""PPO on the device, host tensors (DESIGN.md "PPO on the device"):
mbots_policy_adv_moments, mbots_policy_ppo_loss and mbots_policy_ppo_gate
against their float32 restatement bit for bit, every option, the gradients
against torch autograd in float64, the KL gate through PolicyAdam, the
refusals, and harness/ppo_groups.py in CPU mode.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import policy_grad_ref as gr
import policy_ppo_ref as pr
import policy_ppo_util as u
import test_policy_grad_cpu as tg

t = u.t


@pytest.fixture(scope="module")
def case():
    return u.ppo_case()


@pytest.fixture(scope="module")
def full(case):
    """The restatement of the whole case, once: ([g_logp, g_value, g_entropy,
    stats, moments], aux)."""
    return u.ref_case(case)


def same(got, want):
    for name, a, b in zip(("g_logp", "g_value", "g_entropy"), got, want):
        assert np.array_equal(pr.bits32(a), pr.bits32(b)), name
    assert np.array_equal(pr.bits64(got[3]), pr.bits64(want[3])), "stats"
    if want[4] is not None:
        assert np.array_equal(pr.bits64(got[4]), pr.bits64(want[4])), "moments"


# ---- 1. the case and the restatement ------------------------------------------------------------
def test_the_restatement_s_exp_is_the_device_actor_s():
    import madrona_bots as mb
    rng = np.random.default_rng(0)
    x = np.concatenate([(rng.standard_normal(50000) * 3).astype(np.float32), np.linspace(-110, 90, 4001).astype(np.float32),
                        np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 88.72284, -104.0], np.float32)])
    got = mb.policy_activation("exp", torch.from_numpy(x)).numpy()
    assert np.array_equal(pr.bits32(got), pr.bits32(pr.pol_exp(x)))


def test_case_covers_every_branch_and_boundary(case, full):
    """Counted from the restatement alone, over the kept rows of the groups
    with rows: each class of the clipped surrogate and each side of the
    value-clip choice at least 100 times; ratios exactly on both clip
    boundaries; advantages of +0 and -0."""
    _, aux = full
    K = pr.CHUNK
    lengths = {int(b - a) for a, b in case["segments"].reshape(-1, 2)}
    assert lengths >= {0, 1, 255, 256, 257, K - 1, K, K + 1, 2 * K + 3}
    assert any(int(a) % 4 for a in case["segments"][:, :, 0].reshape(-1))
    assert case["rows"][2] == 0 and int(case["segments"][2, 1, 1] - case["segments"][2, 1, 0]) > 0
    live = aux["seg"].copy()
    live[int(case["segments"][2, 0, 0]):] = False
    assert (~aux["seg"]).sum() >= u.FIRST + 2 * u.GAP + u.TAIL
    assert ((case["end"] == pr.END_RESET) & live).sum() > 1000
    kept = live & (case["end"] != pr.END_RESET)
    A, ratio, rc = aux["A"], aux["ratio"], aux["rc"]
    hi_c, lo_c = np.float32(1) + np.float32(0.2), np.float32(1) - np.float32(0.2)
    classes = {"above, binding": kept & (ratio > hi_c) & (A > 0), "below, binding": kept & (ratio < lo_c) & (A < 0),
               "clipped, not binding": kept & (rc != ratio) & (aux["s1"] <= aux["s2"]),
               "unclipped": kept & (rc == ratio),
               "value: unclipped side": kept & (aux["v1"] >= aux["v2"]), "value: clipped side": kept & (aux["v2"] > aux["v1"]),
               "value: clipped and saturated": kept & (aux["v2"] > aux["v1"]) & (aux["dc"] != aux["dv"])}
    for name, m in classes.items():
        print(name, int(m.sum()))
        assert m.sum() >= 100, name
    e = case["edge"]
    assert len(e["hi"]) == 4 and (ratio[e["hi"]] == hi_c).all() and len(e["lo"]) == 4 and (ratio[e["lo"]] == lo_c).all()
    assert (rc[e["hi"] + e["lo"]] == ratio[e["hi"] + e["lo"]]).all()           # on the boundary: not clipped
    adv = case["cols"][5]
    assert (adv[e["zero"]] == 0).all() and np.signbit(adv[e["zero"]]).sum() == 3


# ---- 2. bit for bit -----------------------------------------------------------------------------
def test_loss_and_moments_equal_the_float32_restatement(case, full):
    import madrona_bots as mb
    want, _ = full
    got = u.run_case(mb, case, "cpu")
    same(got, want)
    assert (got[3][:2] != 0).all() and not got[3][2].any() and got[4][2, 0] > 0   # rows == 0: w = 0, yet moments count
    assert got[4][0, 0] == ((case["end"] != pr.END_RESET)[3:3 + sum(u.LENGTHS[0])]).sum()
    outside = np.ones(case["n"], bool)
    for a, b in case["segments"].reshape(-1, 2):
        outside[a:b] = False
    assert all(not pr.bits32(x)[outside].any() for x in got[:3])               # +0, not -0
    assert all(not x[case["end"] == pr.END_RESET].any() for x in got[:3])
    # The distance of the sums to float64 arithmetic.  A row's values carry fewer than 16 roundings (the exp's two
    # ulps among them) of the sizes of their terms, the f64 sums none worth counting; the rounding of logp - old_logp
    # reaches the ratio with the size of the two log-probabilities.  The clipped fraction is a count: only the eight
    # rows whose float32 ratio lies exactly on a boundary may fall on the other side.
    ref = pr.loss_rows(case["cols"], case["end"], case["segments"], case["rows"], moments=want[4], dtype=np.float64,
                       **u.HYPER)
    logp, value, entropy, old_logp, old_value, adv, ret = (np.abs(c.astype(np.float64)) for c in case["cols"])
    for g in range(2):
        mean, inv = pr.norm_constants(want[4], g, np.float64)
        w = 1.0 / float(case["rows"][g])
        lo, hi = int(case["segments"][g, 0, 0]), int(case["segments"][g, 3, 1])
        sl = slice(lo, hi)
        lsize = 1.0 + logp[sl] + old_logp[sl]
        rsize = np.abs(ref[4]["ratio"][sl]) * lsize
        M = rsize * (adv[sl] + abs(mean)) * inv
        V = np.maximum(value[sl] + ret[sl], old_value[sl] + u.HYPER["value_clip"] + ret[sl]) ** 2
        size = [M + 0.5 * V + 0.01 * entropy[sl], M, V, entropy[sl], rsize + lsize]
        for k in range(5):
            bound = 16 * 2.0 ** -24 * float(size[k].sum()) * w
            print(f"group {g} slot {k}: error {abs(got[3][g, k] - ref[3][g, k]):.3g}, bound {bound:.3g}")
            assert abs(got[3][g, k] - ref[3][g, k]) <= bound, (g, k)
        assert abs(got[3][g, 5] - ref[3][g, 5]) <= 8 * w + 1e-12


@pytest.mark.parametrize("opt", [dict(moments=False), dict(value_clip=False), dict(end=False),
                                 dict(moments=False, value_clip=False, end=False)],
                         ids=("no-moments", "no-value-clip", "no-end", "none"))
def test_options_equal_the_float32_restatement(case, opt):
    import madrona_bots as mb
    same(u.run_case(mb, case, "cpu", **opt), u.ref_case(case, **opt)[0])


def test_value_clip_needs_old_value_and_a_positive_bound(case):
    import madrona_bots as mb
    want = u.ref_case(case, value_clip=False)[0]
    none = dict(case, cols=case["cols"][:4] + [None] + case["cols"][5:])
    same(u.run_case(mb, none, "cpu"), want)                                      # old_value None
    same(u.run_case(mb, case, "cpu", hyper=dict(u.HYPER, value_clip=0.0)), want)


def test_stats_accumulate_over_two_calls(case, full):
    import madrona_bots as mb
    once = full[0][3]
    want = u.ref_case(case, stats=once)[0]
    got = u.run_case(mb, case, "cpu", stats=once.copy())
    same(got, want)
    assert not np.array_equal(got[3][:2], once[:2])
    seg, adv, end = t(case["segments"]), t(case["cols"][5]), t(case["end"])
    m = mb.advantage_moments_groups(adv, end, seg)
    assert mb.advantage_moments_groups(adv, end, seg, moments=m) is m
    assert np.array_equal(pr.bits64(m.numpy()), pr.bits64(pr.moments_rows(case["cols"][5], case["end"], case["segments"],
                                                                         moments=full[0][4])))


def test_normalisation_of_one_row_and_of_equal_advantages():
    """n < 2: mean 0, inv 1 -- the raw advantage.  All advantages equal: var 0,
    A = (adv - mean) * 1e8 = +-0 -- and a group of them with a spread, whose
    f64 variance formula goes negative, is clamped the same way."""
    import madrona_bots as mb
    rng = np.random.default_rng(2)
    seg, n = u.lay_out([[1, 0, 0, 0], [300, 0, 40, 0], [0, 2, 0, 0]], first=1, gap=2, tail=1)
    cols = [(rng.standard_normal(n) * s).astype(np.float32) for s in (1.0, 2.0, 1.0, 1.0, 2.0, 3.0, 2.0)]
    cols[3] = (cols[0] + rng.standard_normal(n).astype(np.float32) * np.float32(0.2)).astype(np.float32)
    cols[5][int(seg[1, 0, 0]):int(seg[1, 3, 1])] = np.float32(0.1)
    c = dict(cols=cols, end=np.zeros(n, np.int32), segments=seg, rows=np.array([1, 340, 2], np.int64), n=n)
    want, aux = u.ref_case(c)
    same(u.run_case(mb, c, "cpu"), want)
    m = want[4]
    assert m[0, 0] == 1 and pr.norm_constants(m, 0) == (0.0, 1.0)
    assert aux["A"][int(seg[0, 0, 0])] == cols[5][int(seg[0, 0, 0])]
    assert pr.norm_constants(m, 1)[1] == np.float32(1e8) and not aux["A"][int(seg[1, 0, 0]):int(seg[1, 0, 1])].any()
    assert m[2, 0] == 2 and pr.norm_constants(m, 2)[1] < 1e3


def test_with_the_old_policy_itself_the_gradients_are_a2c_s(case):
    """old_logp == logp, old_value == value, no normalisation: ratio is exactly
    1, so g_* are a2c_loss_groups' bits, the KL and the clipped fraction +0."""
    import madrona_bots as mb
    cols = list(case["cols"])
    cols[3], cols[4] = cols[0].copy(), cols[1].copy()
    c = dict(case, cols=cols)
    got = u.run_case(mb, c, "cpu", moments=False)
    a2c = mb.a2c_loss_groups(*[t(x) for x in (cols[0], cols[1], cols[2], cols[5], cols[6])], t(case["end"]),
                             t(case["segments"]), t(case["rows"]), 0.5, 0.01)
    for a, b in zip(got[:3], a2c[:3]):
        assert np.array_equal(pr.bits32(a), pr.bits32(b.numpy()))
    assert not pr.bits64(got[3][:, 4:]).any() and got[3][0, 0] != 0


# ---- 3. the gradients against torch autograd ------------------------------------------------------
def test_backward_with_the_loss_gradients_against_torch_autograd():
    """autograd.backward with ppo_loss_groups' g_* against torch autograd of the
    textbook PPO expression (torch.min, torch.clamp, torch.max) in float64: per
    parameter tensor the error is at most 8 x that of torch's own float32
    autograd (test_policy_adam_cpu's yardstick, on the same case; the critic's
    last bias is left out for the reason given there).  No row lies within 1e-3
    of a clip boundary or of a tie of the two branches, where two compositions
    may legitimately take different sides -- asserted from the float64
    restatement."""
    import madrona_bots as mb
    case = tg.CASES[5]                                                        # H = 128, two layers, 201 rows
    net, obs, hidden, action, _ = tg.build(case)
    net = gr.strip_biases(net, ("critic1",))
    n = case[5]
    rng = np.random.default_rng(5)
    adv, ret = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    end = np.where(rng.random(n) < 0.1, pr.END_RESET, 0).astype(np.int32)
    keep = end != pr.END_RESET
    clip, vclip = 0.2, 0.5
    p, ps = gr.policy_net(net)
    outs = p.evaluate(t(obs), t(action))
    segments = np.array([[[0, n], [n, n], [n, n], [n, n]]], np.int32)
    moments = pr.moments_rows(adv, end, segments)
    mean, inv = pr.norm_constants(moments, 0, np.float64)
    lo_c, hi_c = float(np.float32(1) - np.float32(clip)), float(np.float32(1) + np.float32(clip))

    def torch_grads(dtype):
        lv = [torch.from_numpy(a).to(dtype).requires_grad_() for a in gr.evaluate_torch(net, obs, action, dtype)[:3]]
        a, r, k, ol, ov = (torch.from_numpy(x).to(dtype) for x in (adv, ret, keep, old_logp, old_value))
        A = (a - mean) * inv
        ratio = torch.exp(lv[0] - ol)
        pol = -torch.min(ratio * A, torch.clamp(ratio, lo_c, hi_c) * A)
        clipped = ov + torch.clamp(lv[1] - ov, -vclip, vclip)
        vl = torch.max((lv[1] - r) ** 2, (clipped - r) ** 2)
        per_row = pol + 0.5 * vl - 0.01 * lv[2]
        g = torch.autograd.grad((per_row * k).sum() / n, lv)
        return gr.evaluate_torch(net, obs, action, dtype, [x.numpy() for x in g])[3], [x.detach().numpy() for x in lv]
    # the case: noise on the old policy's outputs, redrawn for the rows that land within 1e-3 of a boundary
    lv64 = gr.evaluate_torch(net, obs, action, torch.float64)[:3]
    base = [outs[0].detach().numpy(), outs[1].detach().numpy()]
    noise = [rng.standard_normal(n) * 0.25, rng.standard_normal(n) * 0.6]

    def margins():
        old = [(b + z.astype(np.float32)).astype(np.float32) for b, z in zip(base, noise)]
        aux = pr.ppo_rows(lv64[0], lv64[1], lv64[2], old[0], old[1], adv, ret, np.ones(n), (mean, inv), clip, vclip, 0.5,
                          0.01, np.float64)[4]
        sat = aux["dc"] != aux["dv"]              # (inside the value clip the two branches are one expression)
        m = np.minimum(np.minimum(np.abs(aux["ratio"] - lo_c), np.abs(aux["ratio"] - hi_c)), np.abs(np.abs(aux["dv"]) - vclip))
        return old, aux, np.where(sat, np.minimum(m, np.abs(aux["v1"] - aux["v2"])), m)
    for _ in range(20):
        (old_logp, old_value), aux, margin = margins()
        near = margin <= 2e-3
        if not near.any():
            break
        noise[0][near], noise[1][near] = rng.standard_normal(near.sum()) * 0.25, rng.standard_normal(near.sum()) * 0.6
    print(f"smallest distance to a boundary or a tie: {margin.min():.3g}")
    assert margin.min() > 1e-3
    (ref, _), (t32, _) = torch_grads(torch.float64), torch_grads(torch.float32)
    assert ((aux["rc"] != aux["ratio"]) & keep).sum() > 20 and ((aux["v2"] > aux["v1"]) & keep).sum() > 20
    g = mb.ppo_loss_groups(*outs, t(old_logp), t(old_value), t(adv), t(ret), t(end), t(segments), torch.tensor([n]),
                           clip=clip, value_clip=vclip, moments=t(moments))
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


# ---- 4. the gate ----------------------------------------------------------------------------------
def test_gate_opens_closes_and_stays_closed():
    import madrona_bots as mb
    stats = np.zeros((5, 6))
    stats[:, 4] = [0.01, 0.03, np.nan, 0.0, 0.02]
    rows = np.array([7, 9, 11, 0, 13], np.int64)
    gate = torch.tensor([7, 9, 11, 5, 0])
    assert mb.ppo_kl_gate(t(stats), t(rows), 0.02, gate) is gate
    # below the target: open; above: closed; NaN: closed; rows == 0: closed; closed before: stays closed
    assert gate.tolist() == [7, 0, 0, 0, 0] == pr.gate(np.array([7, 9, 11, 5, 0]), rows, stats, 0.02).tolist()
    stats[:, 4] = 0.0
    assert mb.ppo_kl_gate(t(stats), t(rows), 0.02, gate).tolist() == [7, 0, 0, 0, 0]
    stats[0, 4] = 0.02
    assert mb.ppo_kl_gate(t(stats), t(rows), 0.02, gate).tolist() == [7, 0, 0, 0, 0]      # kl == target: still open
    assert mb.ppo_kl_gate(t(stats), t(rows), float("inf"), t(rows.copy())).tolist() == [7, 9, 11, 0, 13]
    stats[1, 4] = np.inf
    assert mb.ppo_kl_gate(t(stats), t(rows), float("inf"), t(rows.copy())).tolist() == [7, 9, 11, 0, 13]


def test_a_group_past_its_target_kl_takes_no_step():
    """Three epochs; old_logp carries noise, so the first epoch's KL already
    lies above group 0's target: its gate closes before the first step and
    stays closed -- no step, parameters and moments untouched -- while group
    1, with target inf, takes all three."""
    import madrona_bots as mb
    opt, stats, gate, update = u.update_case(mb, "cpu", noisy_old=True, targets=(1e-4, float("inf")))
    before = [p.detach().clone() for p in opt.params]
    update()
    st = stats.numpy()
    assert np.isfinite(st).all() and (st[:, :, 4] > 1e-4).all()
    assert opt.steps.tolist() == [0, 3] and gate.tolist()[0] == 0 and gate.tolist()[1] > 0
    for p, b, g in zip(opt.params, before, opt.param_group):
        assert torch.equal(p.detach().view(torch.int32), b.view(torch.int32)) == (g == 0)
    m = u_slices(opt)
    assert all((not x.any()) == (g == 0) for x, g in zip(m, opt.param_group))
    assert st[1, 1, 4] != st[0, 1, 4] and np.array_equal(st[0, 0], st[2, 0])    # group 0's nets never moved


def u_slices(opt):
    flat = opt.state_dict()["m"].numpy()
    return [flat[o:o + p.numel()] for o, p in zip(opt.offsets, opt.params)]


# ---- 5. refusals ----------------------------------------------------------------------------------
def test_refusals(case):
    import madrona_bots as mb
    cols = [t(c) for c in case["cols"]]
    end, seg, rows = t(case["end"]), t(case["segments"]), t(case["rows"])
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="clip must lie"):
            mb.ppo_loss_groups(*cols, end, seg, rows, clip=bad)
    with pytest.raises(ValueError, match="value_coef"):
        mb.ppo_loss_groups(*cols, end, seg, rows, value_coef=-1.0)
    with pytest.raises(ValueError, match="old_logp must be float32"):
        mb.ppo_loss_groups(*cols[:3], cols[3].double(), *cols[4:], end, seg, rows)
    with pytest.raises(ValueError, match="adv must be float32"):
        mb.ppo_loss_groups(*cols[:5], cols[5][:9], cols[6], end, seg, rows)
    with pytest.raises(ValueError, match="end must be int32"):
        mb.ppo_loss_groups(*cols, end.long(), seg, rows)
    with pytest.raises(ValueError, match="rows must be"):
        mb.ppo_loss_groups(*cols, end, seg, rows.int())
    with pytest.raises(ValueError, match="segments must be"):
        mb.ppo_loss_groups(*cols, end, seg.reshape(-1, 2), rows)
    with pytest.raises(ValueError, match="stats must be"):
        mb.ppo_loss_groups(*cols, end, seg, rows, stats=torch.zeros(3, 6))
    with pytest.raises(ValueError, match="moments must be"):
        mb.ppo_loss_groups(*cols, end, seg, rows, moments=torch.zeros(3, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="moments must be"):
        mb.advantage_moments_groups(cols[5], end, seg, moments=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="gate must be"):
        mb.ppo_kl_gate(torch.zeros(3, 6, dtype=torch.float64), rows, 0.1, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="stats must be"):
        mb.ppo_kl_gate(torch.zeros(3, 5, dtype=torch.float64), rows, 0.1, rows.clone())
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="adv must be float32"):
            mb.ppo_loss_groups(*cols[:5], cols[5].cuda(), cols[6], end, seg, rows)
    s = case["segments"].copy()
    s[0, 1] = [2, 300]
    with pytest.raises(RuntimeError, match="overlap"):
        mb.ppo_loss_groups(*cols, end, t(s), rows)
    with pytest.raises(RuntimeError, match="overlap"):
        mb.advantage_moments_groups(cols[5], end, t(s))
    # the C calls themselves: a short workspace, the coefficients, the group count
    n, G = case["n"], 3
    need = ctypes.c_uint64()
    mb._check(mb._lib.mbots_policy_ppo_workspace(n, G, ctypes.byref(need)))
    assert need.value >= G * 4 * -(-n // pr.CHUNK) * 6 * 8
    ws = torch.zeros(need.value // 8, dtype=torch.float64)
    g = [torch.empty(n) for _ in range(3)]
    stats, mom = torch.zeros(G, 6, dtype=torch.float64), torch.zeros(G, 3, dtype=torch.float64)
    P = mb._ptr

    def loss(nb, clip=0.2, vcoef=0.5, groups=G):
        return mb._lib.mbots_policy_ppo_loss(*[P(c) for c in cols], P(end), n, P(seg), groups, P(rows), None, clip, 0.5,
                                             vcoef, 0.01, P(g[0]), P(g[1]), P(g[2]), P(stats), P(ws), nb, -1, None)
    exact = G * 4 * -(-n // pr.CHUNK) * 6 * 8
    assert loss(exact) == 0 and stats[0, 0] != 0
    for rc in (loss(exact - 8), loss(exact, clip=1.0), loss(exact, clip=0.0), loss(exact, vcoef=-0.5),
               loss(exact, groups=0), loss(exact, groups=65),
               mb._lib.mbots_policy_adv_moments(P(cols[5]), P(end), n, P(seg), G, P(mom), P(ws), exact - 8, -1, None),
               mb._lib.mbots_policy_ppo_workspace(n, 65, ctypes.byref(need))):
        assert rc == -1                                                          # MBOTS_E_INVALID
    with pytest.raises(RuntimeError, match=r"workspace of \d+ bytes, \d+ needed"):
        mb._check(loss(exact - 8))
    assert not mom.any()


# ---- 6. the harness -------------------------------------------------------------------------------
def harness_run(exec_mode, device):
    """harness/ppo_groups.py: 64 worlds, four groups -- the last one's range
    starts past the manager's worlds, so it never has a row -- two updates of
    three epochs; the parameters before and after, and the updates' stats."""
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c
    import ppo_groups
    sim = mb.SimManager(0, 64, 69, 8, exec_mode=exec_mode)
    modules = [a2c.make_modules(H, device, seed=20 + i) for i, H in enumerate((16, 32, 16, 32))]
    before = [[p.detach().cpu().clone() for m in four for p in m.parameters()] for four in modules]
    log = ppo_groups.train(sim, [0, 21, 42, 64], modules, iters=2, horizon=4, epochs=3, lr=1e-3, max_grad_norm=0.5)
    after = [[p.detach().cpu().clone() for m in four for p in m.parameters()] for four in modules]
    return before, after, log


def test_harness_ppo_groups_in_cpu_mode():
    before, after, log = harness_run("cpu", "cpu")
    assert len(log) == 2
    for rec in log:
        st = np.array(rec["stats"])
        assert st.shape == (3, 4, 6) and np.isfinite(st).all()
        assert rec["rows"][3] == 0 and not st[:, 3].any() and all(r > 0 for r in rec["rows"][:3])
        assert (st[1:, :3, 4] > 0).all() and (st[:, :3, 0] != 0).all()          # KL > 0 from the second epoch on
        assert np.abs(st[0, :3, 4]).max() < 1e-9                               # the first epoch: the old policy itself
    same_bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(same_bits(a, b) for a, b in zip(before[3], after[3]))
    for g in range(3):
        assert sum(not same_bits(a, b) for a, b in zip(before[g], after[g])) >= len(before[g]) // 2
