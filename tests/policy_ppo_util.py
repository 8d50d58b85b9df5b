"""Shared cases of the PPO tests (test_policy_ppo_cpu.py,
test_policy_ppo_seq_cpu.py, test_policy_ppo_gpu.py): built from seeds, so that
every device sees the same numbers."""
import numpy as np
import torch

import policy_ppo_ref as pr

F = np.float32
HYPER = dict(clip=0.2, value_clip=0.5, value_coef=0.5, entropy_coef=0.01)
K = pr.CHUNK
# G = 3: every length the two-level order distinguishes; the last group has rows == 0
LENGTHS = [[1, 255, K, K + 1], [256, 2 * K + 3, 257, K - 1], [0, 41, 30, 10]]
FIRST, GAP, TAIL = 3, 11, 37        # rows before, between the groups and after: in no segment


def t(a, device="cpu"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def lay_out(lengths, first=FIRST, gap=GAP, tail=TAIL):
    """(segments int32 [G, 4, 2], n): the segments in order, `gap` rows in no
    segment after every group, so that lo is rarely a multiple of 4."""
    seg, at = [], first
    for four in lengths:
        seg.append([])
        for m in four:
            seg[-1].append([at, at + m])
            at += m
        at += gap
    return np.array(seg, np.int32), at + tail


def boundary_lr(target):
    """float32 values lr with pol_exp(lr) == target exactly (the restatement's
    exp over the floats around log(target))."""
    c = F(np.log(np.float64(target)))
    cand = [c]
    for _ in range(64):
        cand.append(np.nextafter(cand[-1], F(np.inf)))
    lo = c
    for _ in range(64):
        lo = np.nextafter(lo, F(-np.inf))
        cand.append(lo)
    cand = np.array(cand, np.float32)
    return cand[pr.pol_exp(cand) == target]


def ppo_case(seed=5):
    """dict(cols = [logp, value, entropy, old_logp, old_value, adv, ret], end,
    segments, rows, n, edge): LENGTHS laid out with gaps; END_RESET rows
    throughout; old_logp = logp + noise and old_value = value + noise sized so
    that every branch of the clipped surrogate and of the clipped value loss
    has hundreds of rows; `edge`: rows (of the 2 K + 3 segment) whose ratio is
    exactly 1 + clip or 1 - clip, and rows with adv == +0 and -0."""
    rng = np.random.default_rng(seed)
    segments, n = lay_out(LENGTHS)
    logp, value, entropy, adv, ret = [(rng.standard_normal(n) * s).astype(np.float32) for s in (2.0, 5.0, 1.0, 3.0, 5.0)]
    old_logp = (logp + rng.standard_normal(n).astype(np.float32) * F(0.25)).astype(np.float32)
    old_value = (value + rng.standard_normal(n).astype(np.float32) * F(1.0)).astype(np.float32)
    end = rng.integers(0, 4, n).astype(np.int32)
    lo = int(segments[1, 1, 0]) + 700
    hi_c, lo_c = F(1.0) + F(HYPER["clip"]), F(1.0) - F(HYPER["clip"])
    up, down = boundary_lr(hi_c), boundary_lr(lo_c)
    assert len(up) and len(down), "no float32 whose exp is exactly a clip boundary"
    edge = {"hi": [], "lo": [], "zero": []}
    for j in range(8):
        r = lo + 3 * j
        lr = (up if j % 2 == 0 else down)[(j // 2) % len(up if j % 2 == 0 else down)]
        logp[r], old_logp[r], end[r] = lr, F(0.0), 0
        adv[r] = F(1.5) if j % 4 < 2 else F(-1.5)
        edge["hi" if j % 2 == 0 else "lo"].append(r)
    for j in range(6):
        r = lo + 40 + 5 * j
        adv[r], end[r] = (F(0.0) if j % 2 else F(-0.0)), 0
        edge["zero"].append(r)
    rows = np.array([sum(LENGTHS[0]), sum(LENGTHS[1]), 0], np.int64)
    return dict(cols=[logp, value, entropy, old_logp, old_value, adv, ret], end=end, segments=segments, rows=rows, n=n,
                edge=edge)


def run_case(mb, case, device, end=True, moments=True, value_clip=True, stats=None, hyper=None):
    """advantage_moments_groups and ppo_loss_groups of `case` on `device`:
    (g_logp, g_value, g_entropy, stats, moments) as numpy."""
    h = dict(HYPER if hyper is None else hyper)
    if not value_clip:
        h["value_clip"] = None
    e = t(case["end"], device) if end else None
    seg, rows = t(case["segments"], device), t(case["rows"], device)
    cols = [t(c, device) for c in case["cols"]]
    m = mb.advantage_moments_groups(cols[5], e, seg) if moments else None
    got = mb.ppo_loss_groups(*cols, e, seg, rows, moments=m, stats=t(stats, device), **h)
    return [x.cpu().numpy() for x in got] + [None if m is None else m.cpu().numpy()]


def ref_case(case, end=True, moments=True, value_clip=True, stats=None, hyper=None):
    """The float32 restatement of run_case, and the per-row aux."""
    h = dict(HYPER if hyper is None else hyper)
    if not value_clip:
        h["value_clip"] = None
    e = case["end"] if end else None
    m = pr.moments_rows(case["cols"][5], e, case["segments"]) if moments else None
    *g, st, aux = pr.loss_rows(case["cols"], e, case["segments"], case["rows"], moments=m, stats=stats, **h)
    return g + [st, m], aux


# ---- the sequence case ----
SEQ_L = 5
SK = pr.SEQ_CHUNK
SEQ_LENGTHS = [[1, 255, SK, SK + 1], [256, 2 * SK + 3, 257, SK - 1], [0, 41, 30, 10]]
SEQ_LAST_TABLE = 9


def seq_case(seed=8, bad_order=False):
    """dict(cols [7] of [L, B], len, t0, end, order, segments, rows, B): the
    positions laid out as ppo_case's rows; order a permutation of the columns
    -- bad_order: with three entries out of range inside segments, which the
    device reads as columns of length 0 and the host path refuses; len in
    0..L, t0 so that last_table cuts some columns short, leaves some whole and
    drops some entirely; END_RESET with and without the bound leaving the last
    row in."""
    rng = np.random.default_rng(seed)
    segments, B = lay_out(SEQ_LENGTHS)
    L = SEQ_L
    cols = [(rng.standard_normal((L, B)) * s).astype(np.float32) for s in (2.0, 5.0, 1.0, 3.0, 5.0)]
    logp, value, entropy, adv, ret = cols
    old_logp = (logp + rng.standard_normal((L, B)).astype(np.float32) * F(0.25)).astype(np.float32)
    old_value = (value + rng.standard_normal((L, B)).astype(np.float32) * F(1.0)).astype(np.float32)
    length = rng.integers(0, L + 1, B).astype(np.int32)
    t0 = rng.integers(0, SEQ_LAST_TABLE + 3, B).astype(np.int32)
    end = rng.integers(0, 4, B).astype(np.int32)
    order = rng.permutation(B).astype(np.int32)
    bad = [int(segments[0, 1, 0]) + 7, int(segments[1, 1, 0]) + 600, int(segments[1, 3, 0]) + 1]
    if bad_order:
        order[bad[0]], order[bad[1]], order[bad[2]] = -1, B, B + 1000
    kept = pr.seq_kept(length, t0, end, SEQ_LAST_TABLE, L)
    rows = np.zeros(3, np.int64)
    for g in range(2):
        for lo, hi in segments[g]:
            pos = order[lo:hi]
            ok = (pos >= 0) & (pos < B)
            rows[g] += int(kept[pos[ok]].sum())
    return dict(cols=[logp, value, entropy, old_logp, old_value, adv, ret], len=length, t0=t0, end=end, order=order,
                segments=segments, rows=rows, B=B, bad=bad, kept=kept)


def run_seq(mb, case, device, moments=True, value_clip=True, stats=None, last_table=SEQ_LAST_TABLE):
    h = dict(HYPER)
    if not value_clip:
        h["value_clip"] = None
    cols = [t(c, device) for c in case["cols"]]
    meta = [t(case[k], device) for k in ("len", "t0", "end", "order", "segments")]
    m = mb.advantage_moments_sequences(cols[5], *meta, last_table=last_table) if moments else None
    got = mb.ppo_loss_sequences(*cols, *meta, t(case["rows"], device), last_table=last_table, moments=m,
                                stats=t(stats, device), **h)
    return [x.cpu().numpy() for x in got] + [None if m is None else m.cpu().numpy()]


def ref_seq(case, moments=True, value_clip=True, stats=None, last_table=SEQ_LAST_TABLE):
    h = dict(HYPER)
    if not value_clip:
        h["value_clip"] = None
    meta = [case[k] for k in ("len", "t0", "end", "order", "segments")]
    m = pr.moments_seq(case["cols"][5], *meta, last_table=last_table) if moments else None
    return list(pr.loss_seq(case["cols"], *meta, case["rows"], last_table=last_table, moments=m, stats=stats, **h)) + [m]


# ---- a whole multi-epoch update ----
def update_case(mb, device, noisy_old, targets, epochs=3, seed=31):
    """Two groups of four H = 16 nets and 300 recorded rows in segments with a
    gap (test_policy_adam_gpu.update_case's shape).  old_logp and old_value are
    evaluate_groups' outputs at the initial parameters -- noisy_old: old_logp
    plus noise, so that the first epoch's KL is positive already.  update() is
    one update of `epochs` epochs; group g stops once its KL passes targets[g]
    (two gate calls, one per target, joined by a select).  Returns (opt, stats
    [epochs, 2, 6], gate, update)."""
    import policy_adam_util as au
    rng = np.random.default_rng(seed)
    nets = [[au.make_net(mb, rng, 16, device) for _ in range(4)] for _ in range(2)]
    n = 300
    obs = t(np.abs(rng.normal(0.0, 3.0, (n, 69))).astype(np.float32), device)
    action = t(rng.integers(0, 6, n).astype(np.int32), device)
    adv, ret = (t(rng.standard_normal(n).astype(np.float32), device) for _ in range(2))
    end = t(rng.integers(0, 4, n).astype(np.int32), device)
    noise = t((rng.standard_normal(n) * 0.1).astype(np.float32), device)
    seg = torch.tensor([[[0, 70], [70, 71], [71, 71], [71, 140]],
                        [[150, 215], [215, 280], [280, 290], [290, 300]]], dtype=torch.int32, device=device)
    opt = mb.PolicyAdam(nets, lr=1e-2, max_grad_norm=0.5)
    rows = mb.policy_group_rows(seg, torch.zeros(2, dtype=torch.int64, device=device))
    first = [x.detach().clone() for x in mb.evaluate_groups(nets, obs, action, seg)]
    old_logp, old_value = (first[0] + noise if noisy_old else first[0]), first[1]
    moments = mb.advantage_moments_groups(adv, end, seg)
    stats = torch.zeros((epochs, 2, 6), dtype=torch.float64, device=device)
    gates = [torch.zeros(2, dtype=torch.int64, device=device) for _ in range(3)]
    pick = torch.tensor([True, False], device=device)

    def update():
        stats.zero_()
        gates[0].copy_(rows)
        gates[1].copy_(rows)
        for e in range(epochs):
            opt.zero_grad()
            outs = mb.evaluate_groups(nets, obs, action, seg)
            g = mb.ppo_loss_groups(*outs, old_logp, old_value, adv, ret, end, seg, rows, moments=moments, stats=stats[e],
                                   **HYPER)
            torch.autograd.backward(list(outs), list(g[:3]))
            mb.ppo_kl_gate(stats[e], rows, targets[0], gates[0])
            mb.ppo_kl_gate(stats[e], rows, targets[1], gates[1])
            torch.where(pick, gates[0], gates[1], out=gates[2])
            opt.step(gates[2])
    return opt, stats, gates[2], update
