"""CPU mode: policy groups (DESIGN.md "Policy groups"; SimManager
.set_policy_groups / set_policy(group=) / policy_segments) -- world ranges
acting through nets of their own in the one act(): the default, the bitwise
equality with an ungrouped manager when every group holds the same nets, the
float64 restatement with a different architecture per group, evaluate() per
segment, the segments against numpy, mixed memory heads, shards and refusals."""
import numpy as np
import pytest
import torch

import policy_ref as pr
import policy_groups_util as gu
import test_policy_cpu as tp
from simpair import compare


# ---- 1. default ----------------------------------------------------------------
def test_default_is_one_group():
    sim = gu.make_sim("B", starts=False)
    assert sim.policy_groups == [0]
    sc = sim.species_count_tensor().to_torch().numpy()
    seg = sim.policy_segments()
    assert seg.dtype == torch.int32 and tuple(seg.shape) == (1, 4, 2)
    ends = np.cumsum(sc.sum(axis=0))
    assert seg.numpy()[0].tolist() == [[int(e - n), int(e)] for e, n in zip(ends, sc.sum(axis=0))]
    sim.set_policy_groups([0])            # the starts in place: nothing changes
    sim.set_policy_groups(None)
    assert sim.policy_groups == [0]


# ---- 2. the same nets in every group: an ungrouped manager, bitwise -----------
def run_same_nets(exec_mode, shape, pattern):
    a, b = gu.make_sim(shape, exec_mode), gu.make_sim(shape, exec_mode, starts=False)
    nets = tp.make_nets(gu.CASES[3], pr.inputs(a, True))
    a.set_policy([pr.policy_net(n, a.device) for n in nets])      # no group: every group
    b.set_policy([pr.policy_net(n, b.device) for n in nets])
    W = gu.SHAPES[shape][0][0]
    reset = [1, 7] if W > 7 else [1, 2]
    for t in range(6):
        if pattern == "reset" and t == 2:
            a.reset_worlds(reset)
            b.reset_worlds(reset)
        gu.assert_same_outputs(a.act(), b.act(), f"{shape} {pattern} round {t}")
        for m in (a, b):
            m.step()
            if pattern == "shift":
                m.shift_observations()
        errs = compare(a, tp._AsOracle(b), f"{shape} {pattern} round {t}")
        assert not errs, errs[:4]


@pytest.mark.parametrize("pattern", ["plain", "shift", "reset"])
@pytest.mark.parametrize("shape", ["A", "B", "D"])
def test_same_nets_in_every_group_equal_an_ungrouped_manager(shape, pattern):
    run_same_nets("cpu", shape, pattern)


# ---- 3. different nets per group against float64 -------------------------------
DRAW = {"A": 11, "B": 11}   # draws at which the float64 restatement alone exempts <= 1 % of rows (asserted)


@pytest.mark.parametrize("shape", ["A", "B"])
def test_different_nets_per_group_against_float64(shape):
    """The scheme of test_forward_and_sampling_against_float64 over a grouped
    table: value, logp and the new HiddenState within tol = 8 x torch-f32's own
    largest error against float64; actions equal the restatement's except where
    u lies within 4 tol of a CDF edge, at most 1 % of rows."""
    sim = gu.make_sim(shape)
    starts = gu.SHAPES[shape][1]
    nets = gu.make_group_nets(sim, len(starts))
    gu.set_group_nets(sim, nets)
    sc = sim.species_count_tensor().to_torch().numpy()
    gw, sp, k = pr.row_keys(sc)
    (z64, v64, m64), (z32, v32, m32), has_mem = gu.reference(nets, sim, starts)
    assert has_mem.any() and not has_mem.all()
    hidden_before = sim.hidden_state_tensor().to_torch().numpy().copy()
    sim.policy_draw = DRAW[shape]
    o = sim.act()
    a, logp, value = (o[q].numpy()[:, 0] for q in ("action", "logp", "value"))
    lp64, lp32 = pr.logp64(z64), pr.logp64(z32)
    err32 = max(np.abs(v32 - v64).max(), np.abs(lp32 - lp64).max(), np.abs(m32 - m64)[has_mem].max())
    tol = 8.0 * err32
    a64, dist = pr.sample64(z64, pr.uniforms(tp.SEED, DRAW[shape], gw, sp, k))
    exempt = dist <= 4.0 * tol
    # (a condition on the restatement alone: nothing of the code under test is in it)
    assert exempt.mean() <= 0.01, (exempt.mean(), tol)
    rows = np.arange(len(a))
    e_v = np.abs(value - v64).max()
    e_lp = np.abs(logp - lp64[rows, a]).max()
    hid = sim.hidden_state_tensor().to_torch().numpy()
    e_m = np.abs(hid - m64)[has_mem].max()
    print(f"tol {tol:.3g} (torch f32 {err32:.3g}); value {e_v:.3g} logp {e_lp:.3g} memory {e_m:.3g}; "
          f"exempt {exempt.mean():.4f}")
    assert tol > 0 and e_v <= tol and e_lp <= tol and e_m <= tol
    assert np.array_equal(hid.view(np.uint32)[~has_mem], hidden_before.view(np.uint32)[~has_mem])
    assert np.array_equal(a[~exempt], a64[~exempt])
    onehot = sim.action_tensor().to_torch().numpy()
    assert np.array_equal(onehot, (np.arange(6)[None, :] == a[:, None]).astype(np.int32))


# ---- 4. act() equals evaluate per segment --------------------------------------
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_act_equals_evaluate_per_segment(shape):
    sim = gu.make_sim(shape)
    starts = gu.SHAPES[shape][1]
    W = gu.SHAPES[shape][0][0]
    needed = gu.needed_groups(starts, 0, W)
    nets = gu.make_group_nets(sim, len(starts))
    pnets = [[pr.policy_net(n) for n in four] for four in nets]
    for g in needed:                      # (a group without a world here needs no net)
        sim.set_policy(pnets[g], group=g)
    obs = sim.construct_obs().clone()
    hidden = sim.hidden_state_tensor().to_torch().clone()
    seg = sim.policy_segments().tolist()
    o = sim.act()
    covered = 0
    for g in range(len(starts)):
        for s in range(4):
            lo, hi = seg[g][s]
            if g not in needed:
                assert lo == hi
            if lo == hi:
                continue
            with torch.no_grad():
                logp, value, _ = pnets[g][s].evaluate(obs[lo:hi], o["action"][lo:hi], hidden[lo:hi])
            assert torch.equal(logp.view(torch.int32), o["logp"][lo:hi, 0].view(torch.int32)), (g, s)
            assert torch.equal(value.view(torch.int32), o["value"][lo:hi, 0].view(torch.int32)), (g, s)
            covered += hi - lo
    assert covered == sim.num_agents()


# ---- 5. segments -----------------------------------------------------------------
@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_segments_equal_numpy_after_births_and_deaths(shape):
    sim = gu.make_sim(shape)
    starts = gu.SHAPES[shape][1]
    counts = set()
    for t in range(5):
        sc = sim.species_count_tensor().to_torch().numpy()
        counts.add(int(sc.sum()))
        seg = sim.policy_segments().numpy()
        assert np.array_equal(seg, gu.segments_numpy(sc, starts)), t
        # species-major, group-minor, the segments tile [0, N)
        flat = seg.transpose(1, 0, 2).reshape(-1, 2)
        assert flat[0, 0] == 0 and flat[-1, 1] == sim.num_agents()
        assert np.array_equal(flat[1:, 0], flat[:-1, 1]) and (flat[:, 1] >= flat[:, 0]).all()
        if shape == "C":
            assert (seg[2, :, 0] == seg[2, :, 1]).all()
        sim.write_synthetic_actions(99, t, True)
        sim.step()
    assert len(counts) > 1 or shape == "A"   # the population moved (the 15 agents of A rarely do in five steps)
    out = torch.zeros((len(starts), 4, 2), dtype=torch.int32)
    assert sim.policy_segments(out=out) is out
    with pytest.raises(ValueError, match=r"int32 \[\d+, 4, 2\]"):
        sim.policy_segments(out=torch.zeros((1, 4, 2), dtype=torch.int32))


# ---- 6. mixed memory heads -------------------------------------------------------
def run_mixed_memory_heads(exec_mode):
    """Group 0's nets have memory heads, group 1's have none: after a step and
    a shift, act() leaves group 1's HiddenState rows as they are and writes
    group 0's with the heads' outputs (those of an ungrouped manager holding
    group 0's nets)."""
    import madrona_bots as mb
    W, A, cut = 40, 32, 17
    sims = [mb.SimManager(0, W, tp.SEED, A, exec_mode=exec_mode) for _ in range(2)]
    a, b = sims
    a.set_policy_groups([0, cut])
    mem = tp.make_nets(gu.CASES[3], np.abs(np.random.default_rng(0).normal(0, 30, (64, 85))).astype(np.float32))
    none = tp.make_nets(gu.CASES[2], np.abs(np.random.default_rng(1).normal(0, 30, (64, 69))).astype(np.float32))
    a.set_policy([pr.policy_net(n, a.device) for n in mem], group=0)
    a.set_policy([pr.policy_net(n, a.device) for n in none], group=1)
    b.set_policy([pr.policy_net(n, b.device) for n in mem])
    rng = np.random.default_rng(5)
    for t in range(3):
        # a HiddenState that is nobody's output, for the rows act() must keep
        h = torch.from_numpy(rng.standard_normal((a.num_agents(), 16)).astype(np.float32)).to(a.device)
        for m in sims:
            m.write_synthetic_actions(4321, t, True)
            m.write_actions(memory=h)
            m.step()
            m.shift_observations()
        # (from the twin, which holds the same table: nothing reads a's HiddenState before its act())
        before = b.hidden_state_tensor().to_torch().clone()
        seg = a.policy_segments().tolist()
        a.policy_draw = b.policy_draw = t
        a.act()
        b.act()
        ha, hb = a.hidden_state_tensor().to_torch(), b.hidden_state_tensor().to_torch()
        for s in range(4):
            (l0, h0), (l1, h1) = seg[0][s], seg[1][s]
            assert h0 > l0 and h1 > l1
            assert torch.equal(ha[l0:h0].view(torch.int32), hb[l0:h0].view(torch.int32)), (t, s)
            assert not torch.equal(ha[l0:h0], before[l0:h0])
            assert torch.equal(ha[l1:h1].view(torch.int32), before[l1:h1].view(torch.int32)), (t, s)


def test_mixed_memory_heads_keep_and_write_hidden_state():
    run_mixed_memory_heads("cpu")


# ---- 7. shards -------------------------------------------------------------------
@pytest.mark.parametrize("starts", [[0, 2, 6], [0, 2, 4]], ids=["cut-inside-a-group", "ghost-in-the-next-group"])
def test_two_shards_with_groups_equal_one_manager(starts):
    """Worlds 0..7 cut at 4.  [0, 2, 6]: the cut lies inside group 1, whose nets
    both shards hold.  [0, 2, 4]: shard 0's last local world belongs to group 1,
    its ghost (global world 4) to group 2."""
    import madrona_bots as mb
    W, A = 8, 16
    whole = mb.SimManager(0, W, tp.SEED, A, exec_mode="cpu")
    shards = [mb.SimManager(0, W // 2, tp.SEED, A, exec_mode="cpu", world_offset=0, shard_ghost=True),
              mb.SimManager(0, W // 2, tp.SEED, A, exec_mode="cpu", world_offset=W // 2)]
    nets = gu.make_group_nets(whole, len(starts), first=1)
    for m, (lo, hi) in zip([whole] + shards, ((0, W), (0, W // 2 + 1), (W // 2, W))):
        m.set_policy_groups(starts)
        assert m.policy_groups == starts
        gu.set_group_nets(m, nets, groups=gu.needed_groups(starts, lo, hi))   # no more than act() asks for
    taken = np.zeros(6)
    for t in range(6):
        # the ghost's rows follow row N of shard 0's outputs: they are the whole manager's
        # rows of global world W // 2, species by species, through that world's group's nets
        ow = whole.act()
        sc = whole.species_count_tensor().to_torch().numpy()
        n0, rows0 = shards[0].num_agents(), shards[0].num_rows()
        assert rows0 - n0 == sc[W // 2].sum() > 0
        out = {"action": torch.zeros((rows0, 1), dtype=torch.int32), "logp": torch.zeros((rows0, 1)),
               "value": torch.zeros((rows0, 1))}
        shards[0].act(out=out)
        o = shards[1].act()
        at = np.concatenate([np.arange(sc[:, :s].sum() + sc[:W // 2, s].sum(),
                                       sc[:, :s].sum() + sc[:W // 2 + 1, s].sum()) for s in range(4)]).astype(np.int64)
        gu.assert_same_outputs({k: v[n0:] for k, v in out.items()}, {k: v[at] for k, v in ow.items()},
                               f"the ghost's rows, round {t}")
        for m in [whole] + shards:
            m.step()
        taken += np.bincount(o["action"].numpy().ravel(), minlength=6)
    assert (taken > 0).sum() >= 3
    full, full_states = gu.by_world(whole, 0)
    for m, off in zip(shards, (0, W // 2)):
        sc = m.species_count_tensor().to_torch().numpy()
        assert np.array_equal(m.policy_segments().numpy(), gu.segments_numpy(sc, starts, off))
        part, states = gu.by_world(m, off)
        for key, cols in part.items():
            for k, v in cols.items():
                assert np.array_equal(v.view(np.uint32), full[key][k].view(np.uint32)), (key, k)
        for w, st in states.items():
            for k in st:
                assert np.array_equal(np.asarray(st[k]), np.asarray(full_states[w][k])), (w, k)


# ---- 8. refusals -----------------------------------------------------------------
def test_refusals_name_what_is_wrong():
    sim = gu.make_sim("B", starts=False)
    with pytest.raises(RuntimeError, match="ascending"):
        sim.set_policy_groups([0, 5, 5])
    with pytest.raises(RuntimeError, match="ascending"):
        sim.set_policy_groups([0, 9, 3])
    with pytest.raises(RuntimeError, match="begin at world 0, not 1"):
        sim.set_policy_groups([1, 2])
    with pytest.raises(RuntimeError, match="65 policy groups: at most 64"):
        sim.set_policy_groups(list(range(65)))
    assert sim.policy_groups == [0]
    sim.set_policy_groups(list(range(64)))
    sim.set_policy_groups([0, 1, 17, 39])
    nets = gu.make_group_nets(sim, 4)
    with pytest.raises(ValueError, match="policy group 4 out of range: the manager has 4"):
        sim.set_policy([pr.policy_net(n) for n in nets[0]], group=4)
    with pytest.raises(ValueError, match="out of range"):
        sim.clear_policy(group=7)
    gu.set_group_nets(sim, nets)
    first = sim.act(write=False)
    sim.clear_policy(species=3, group=2)
    with pytest.raises(RuntimeError, match="group 2 species 3 has no policy net"):
        sim.act()
    sim.set_policy(pr.policy_net(nets[2][2]), species=3, group=2)
    sim.policy_draw = 0
    gu.assert_same_outputs(first, sim.act(write=False), "the net is back")
    # the starts in place: the nets stay
    sim.set_policy_groups([0, 1, 17, 39])
    sim.policy_draw = 0
    gu.assert_same_outputs(first, sim.act(write=False), "the same starts")
    # new starts: every net is gone
    sim.set_policy_groups([0, 1, 17])
    assert sim.policy_groups == [0, 1, 17]
    with pytest.raises(RuntimeError, match="group 0 species 1 has no policy net"):
        sim.act()
    sim.set_policy_groups([])             # as None: back to one group
    assert sim.policy_groups == [0] and tuple(sim.policy_segments().shape) == (1, 4, 2)
    with pytest.raises(RuntimeError, match="species 1 has no policy net"):
        sim.act()
    sim.clear_policy()                    # (of nets that are not there: nothing happens)
    sim.set_policy([pr.policy_net(n) for n in nets[0]])
    assert sim.act(write=False)["action"].shape[0] == sim.num_agents()



# ---- 9. the harness, and the capacity hand-over ---------------------------------------
def test_a2c_groups_example_loop_runs_and_learns_something():
    """harness/a2c_groups.py: three updates of three universes of two widths on
    one manager; every universe's loss is finite and most of its parameters move."""
    import os
    import sys
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c
    import a2c_groups
    sim = mb.SimManager(0, 6, 69, 8, exec_mode="cpu")
    modules = [a2c.make_modules(h, "cpu", seed=1 + u) for u, h in enumerate((16, 32, 16))]
    before = [[p.detach().clone() for m in four for p in m.parameters()] for four in modules]
    optimizers = [[torch.optim.Adam(m.parameters(), lr=1e-3) for m in four] for four in modules]
    losses = a2c_groups.train(sim, [0, 2, 4], modules, optimizers, iters=3, horizon=4)
    assert sim.policy_groups == [0, 2, 4]
    assert len(losses) == 3 and all(len(row) == 3 and all(np.isfinite(row)) for row in losses)
    for four, old in zip(modules, before):
        after = [p.detach() for m in four for p in m.parameters()]
        assert all(torch.isfinite(q).all() for q in after)
        assert sum(not torch.equal(a, b) for a, b in zip(old, after)) >= len(old) // 2


@pytest.mark.parametrize("reward_fixed", [True, False])
def test_a2c_groups_learners_meet_only_in_the_faithful_reward(reward_fixed):
    """Two universes on one 8-world manager; the second one's nets change in
    width and weights between two runs.  With reward_fixed the first universe's
    losses and updated weights are the same bits in both runs.  With the
    reference's faithful reward (rewards[speciesID], include/mbots.h
    MBOTS_FLAG_REWARD_FIXED) species 4 of a world is paid from the next world's
    row, so the first universe's last world hears of its neighbour and its
    losses differ: the one place where groups meet, as shards meet in the ghost."""
    import os
    import sys
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c
    import a2c_groups
    W, A, iters, horizon = 8, 16, 2, 4

    def run(hidden):
        mods = [a2c.make_modules(h, "cpu", 5 + u) for u, h in enumerate(hidden)]
        opts = [[torch.optim.Adam(m.parameters(), lr=1e-3) for m in four] for four in mods]
        sim = mb.SimManager(0, W, tp.SEED, A, exec_mode="cpu", reward_fixed=reward_fixed)
        return a2c_groups.train(sim, [0, W // 2], mods, opts, iters, horizon), mods
    (la, ma), (lb, mb_) = run((32, 16)), run((32, 64))
    assert [row[1] for row in la] != [row[1] for row in lb]
    same_w = all(torch.equal(p.view(torch.int32), q.view(torch.int32))
                 for fa, fb in zip(ma[0], mb_[0]) for p, q in zip(fa.parameters(), fb.parameters()))
    assert ([row[0] for row in la] == [row[0] for row in lb]) == reward_fixed
    assert same_w == reward_fixed


def test_groups_follow_the_cpu_mode_capacity_hand_over():
    """auto_grow in CPU mode hands the manager over to a larger one: the groups,
    every group's nets and the draw counter go with it."""
    import madrona_bots as mb
    a = mb.SimManager(0, 6, tp.SEED, 12, exec_mode="cpu", agent_capacity=16, auto_grow=True)
    b = mb.SimManager(0, 6, tp.SEED, 12, exec_mode="cpu", agent_capacity=128)
    nets = gu.make_group_nets(b, 3)
    for m in (a, b):
        m.set_policy_groups([0, 2, 5])
        gu.set_group_nets(m, nets)
    for t in range(4):
        gu.assert_same_outputs(a.act(), b.act(), f"round {t}")
        a.step()
        b.step()
    assert a.agent_capacity > 16 and a.policy_groups == [0, 2, 5] and a.policy_draw == b.policy_draw == 4
