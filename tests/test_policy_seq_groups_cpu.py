"""CPU mode: madrona_bots.sequence_segments and evaluate_sequences_groups
(DESIGN.md "Grouped evaluate_sequences"; mbots_policy_seq_order /
mbots_policy_seq_eval_groups / mbots_policy_seq_grad_groups on the host path)
against the per-net evaluate_sequences loop over nonzero / index_select slices,
bit for bit, on the fixture of tests/policy_seq_groups_util.py: the sort, the
outputs, hidden and every gradient, the columns of no net, independence of the
host's thread count, the L = 1 case against evaluate_groups, padding, the
refusals, act()'s bits through a window, and the harness."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_seq_groups_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def loop():
    """The per-net loop's result on the fixture, computed once."""
    return u.run_loop(*u.fixture())


@pytest.fixture(scope="module")
def grouped():
    return u.cpu_grouped()


def test_fixture_covers_the_cases():
    nets, net_id, obs, action, length, hidden0, g = u.fixture()
    order, seg = u.segments_ref(net_id, u.G)
    order, seg = order.numpy(), seg.numpy()
    sizes = (seg[..., 1] - seg[..., 0]).ravel().tolist()
    assert set(sizes) == {0, 1, 63, 64, 65, 64 * 256 + 1} and obs.shape[0] == u.L == 5
    assert [a[0] for a in u.ARCH] == [16, 128, 64] and nets[2][3] is None
    assert (net_id < 0).any() and (net_id >= 4 * u.G).any() and (length == 0).any()
    # far from the identity: hardly any position holds its own column
    n = int(seg.max())
    assert (order[:n] == np.arange(n)).mean() < 0.01
    big = order[seg[0, 0, 0]:seg[0, 0, 1]]
    assert length[big].max() == 2 and length[big[:64]].min() >= 1 and length[big[-1]] == 2     # 257 tiles, the wrap
    lo = seg[u.SHORT_TILE][0]
    assert length[order[lo:lo + 64]].max() == u.L - 1
    lo = seg[u.EMPTY_TILE][0]
    assert length[order[lo:lo + 64]].max() == 0 and length[order[lo + 64]] == u.L


# ---- 1. the sort ----------------------------------------------------------------------
def test_sequence_segments_equals_the_nonzero_construction():
    import madrona_bots as mb
    net_id = u.fixture()[1]
    for ids, groups in ((net_id, u.G), (net_id, 64), (net_id[:1], 1), (net_id[:0], 2),
                        (np.full(1500, 7, np.int32), 2), (np.full(70, -1, np.int32), 1)):
        order, seg = mb.sequence_segments(torch.from_numpy(np.ascontiguousarray(ids)), groups)
        want_order, want_seg = u.segments_ref(ids, groups)
        assert order.dtype == torch.int32 and seg.dtype == torch.int32 and tuple(seg.shape) == (groups, 4, 2)
        assert torch.equal(order, want_order) and torch.equal(seg, want_seg)
        assert bool((order[int(seg.max()):] == -1).all())
    with pytest.raises(ValueError, match="groups must be 1..64"):
        mb.sequence_segments(torch.zeros(3, dtype=torch.int32), 65)
    with pytest.raises(ValueError, match="net_id must be int32"):
        mb.sequence_segments(torch.zeros(3, dtype=torch.int64), 2)


# ---- 2. outputs, hidden and every gradient ------------------------------------------------
def test_outputs_and_gradients_equal_the_per_net_loop(loop, grouped):
    u.assert_same(grouped, loop, "cpu")
    # (the comparison is not one of zeros)
    assert all(float(o.abs().max()) > 0 for o in grouped[0])
    for g_, s_ in ((0, 0), (1, 3), (2, 1)):
        assert all(float(q.abs().max()) > 0 for q in grouped[1][g_][s_]), (g_, s_)
    assert all(not q.any() for q in grouped[1][0][1])                         # the empty segment: zeros
    assert len(grouped[1][1][0]) == 2 * (3 + 5)                               # the memory head's two are among them


def test_columns_outside_are_zero_and_change_nothing(grouped):
    nets, net_id, obs, action, length, hidden0, g = u.fixture()
    outside = u.outside_columns(net_id, nets)
    assert outside.sum() == u.N_NONE + u.SIZES[2][3]
    for o in grouped[0]:
        assert not o.view(torch.int32)[:, torch.from_numpy(outside)].any()    # +0, bit for bit
    rng = np.random.default_rng(5)
    obs2, hidden2, action2, length2 = obs.copy(), hidden0.copy(), action.copy(), length.copy()
    obs2[:, outside] = rng.normal(0, 1e6, (u.L, int(outside.sum()), 69)).astype(np.float32)
    obs2[0, np.nonzero(outside)[0][0]] = np.nan
    hidden2[outside] = 3.0
    action2[:, outside] = 77                                                  # never looked at
    length2[outside] = 99
    g2 = [gi.copy() for gi in g]
    for gi in g2:
        gi[:, outside] = 1e30
    again = u.run_grouped(nets, net_id, obs2, action2, length2, hidden2, g2)
    u.assert_same(again, grouped, "outside columns changed")


# ---- 3. the host's thread count -----------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, {tests!r})
import conftest   # the suite's import paths
import policy_seq_groups_util as u
print(u.digest(u.cpu_grouped()))
"""


def test_bits_do_not_depend_on_host_threads(grouped):
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"))
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, text=True,
                              env=dict(os.environ, MBOTS_CPU_THREADS=t)) for t in ("1", "5", "16")]
    outs = [p.communicate()[0].split() for p in procs]
    assert all(p.returncode == 0 for p in procs)
    assert outs[0] == outs[1] == outs[2] == [u.digest(grouped)]


# ---- 4. L = 1: evaluate_groups' bits -------------------------------------------------------
def test_one_step_equals_evaluate_groups():
    import madrona_bots as mb
    nets, net_id, obs, action, length, hidden0, g = u.fixture()
    pn, params = u.policy_nets(nets)
    tid, to, ta, th, *tg = u.to("cpu", net_id, obs[:1], action[:1], hidden0, *[gi[:1] for gi in g])
    ones = torch.ones(len(net_id), dtype=torch.int32)
    order, seg = mb.sequence_segments(tid, u.G)
    out = mb.evaluate_sequences_groups(pn, to, ta, ones, th, order, seg)
    sum((gi * oi).sum() for gi, oi in zip(tg, out)).backward()
    got = u.grads_of(params)
    # the same rows, gathered in segment order, through evaluate_groups
    n = int(seg.max())
    rows = order[:n].long()
    pn2, params2 = u.policy_nets(nets)
    out2 = mb.evaluate_groups(pn2, to[0][rows].contiguous(), ta[0][rows].contiguous(), seg, th[rows].contiguous())
    sum((gi[0][rows] * oi).sum() for gi, oi in zip(tg, out2)).backward()
    want = u.grads_of(params2)
    for a, b in zip(out, out2):
        assert torch.equal(a.detach()[0][rows], b.detach())
    for g_ in range(u.G):
        for s_ in range(4):
            if nets[g_][s_] is None:
                continue
            for i, (a, b) in enumerate(zip(got[g_][s_][:-2], want[g_][s_][:-2])):      # all but the memory head
                assert torch.equal(a, b), (g_, s_, i)


# ---- 5. padding ---------------------------------------------------------------------------
def test_absent_steps_and_empty_columns_change_no_bit(grouped):
    nets, net_id, obs, action, length, hidden0, g = u.fixture()
    rng = np.random.default_rng(6)
    extra, steps = 70, 2
    B = len(net_id)
    obs2 = rng.normal(0, 100.0, (u.L + steps, B + extra, 69)).astype(np.float32)
    obs2[:u.L, :B] = obs
    action2 = np.full((u.L + steps, B + extra), 9, np.int32)
    action2[:u.L, :B] = action
    g2 = [np.full((u.L + steps, B + extra), 1e20, np.float32) for _ in g]
    for a, b in zip(g2, g):
        a[:u.L, :B] = b
    net_id2 = np.concatenate([net_id, np.full(extra, 4 * 1 + 0, np.int32)])               # two more tiles of (1, 0)
    length2 = np.concatenate([length, np.zeros(extra, np.int32)])
    hidden2 = np.concatenate([hidden0, np.ones((extra, 16), np.float32)])
    out, grads = u.run_grouped(nets, net_id2, obs2, action2, length2, hidden2, g2)
    for o in out:
        assert not o[u.L:].view(torch.int32).any() and not o[:, B:].view(torch.int32).any()
    u.assert_same(([o[:u.L, :B] for o in out], grads), grouped, "padding")


# ---- 6. refusals --------------------------------------------------------------------------
def test_refusals():
    import madrona_bots as mb
    nets, net_id, obs, action, length, hidden0, g = u.fixture()
    pn, params = u.policy_nets(nets)
    tid, to, ta, tl, th = u.to("cpu", net_id, obs, action, length, hidden0)
    order, seg = mb.sequence_segments(tid, u.G)
    call = lambda **kw: mb.evaluate_sequences_groups(
        kw.get("nets", pn), kw.get("obs", to), kw.get("action", ta), kw.get("length", tl), kw.get("hidden0", th),
        kw.get("order", order), kw.get("seg", seg))
    # a net without a memory head (or without memory_in): the pair is named, evaluate_groups pointed to
    import policy_ref as pr
    plain = dict(nets[1][2], memory=None)
    pn2 = [list(four) for four in pn]
    pn2[1][2] = pr.policy_net(plain)
    with pytest.raises(ValueError, match=r"group 1, species 3\): .* memory head .* evaluate_groups"):
        call(nets=pn2)
    pn2[1][2] = pr.policy_net(dict(nets[2][0], memory_in=False,
                                   trunk=[(nets[2][0]["trunk"][0][0][:, :69].copy(),) + nets[2][0]["trunk"][0][1:]]
                                   + nets[2][0]["trunk"][1:]))
    with pytest.raises(ValueError, match=r"group 1, species 3\): .* evaluate_groups"):
        call(nets=pn2)

    def bad_segments(g_, s_, lo, hi):
        s2 = seg.clone()
        s2[g_, s_, 0], s2[g_, s_, 1] = lo, hi
        return s2
    lo, hi = (int(v) for v in seg[1, 0])
    with pytest.raises(RuntimeError, match="group 0 species 4 and group 1 species 1 overlap"):
        call(seg=bad_segments(0, 3, lo - 1, lo + 1))
    with pytest.raises(RuntimeError, match=r"group 2 species 3 is not inside the \d+ positions of order"):
        call(seg=bad_segments(2, 2, len(net_id) - 3, len(net_id) + 1))
    with pytest.raises(RuntimeError, match="group 1 species 2 is not inside"):
        call(seg=bad_segments(1, 1, 9, 8))
    # an order entry out of range, and a column named twice
    for bad in (-1, len(net_id)):
        o2 = order.clone()
        o2[lo + 5] = bad
        with pytest.raises(RuntimeError, match=rf"group 1 species 1: order\[{lo + 5}\] = {bad} is outside"):
            call(order=o2)
    o2 = order.clone()
    o2[lo + 5] = o2[int(seg[0, 2, 0])]
    with pytest.raises(RuntimeError, match=rf"group 1 species 1: order\[{lo + 5}\] = \d+ names a sequence a second time"):
        call(order=o2)
    # a bad length and a bad present action inside a segment; outside a segment, or absent, neither is looked at
    col = int(order[int(seg[2, 1, 0]) + 3])
    l2 = tl.clone()
    l2[col] = u.L + 1
    with pytest.raises(RuntimeError, match=rf"group 2 species 2: length {u.L + 1} of sequence {col} is outside \[0, 5\]"):
        call(length=l2)
    l2[col] = 2
    a2 = ta.clone()
    a2[1, col] = 6
    with pytest.raises(RuntimeError, match=rf"group 2 species 2: action 6 of step 1 of sequence {col} is outside 0..5"):
        call(length=l2, action=a2)
    l2[col] = 1
    call(length=l2, action=a2)
    # shapes, dtypes and devices name the argument
    with pytest.raises(ValueError, match="obs must be float32"):
        call(obs=to.double())
    with pytest.raises(ValueError, match="action must be int32"):
        call(action=ta.long())
    with pytest.raises(ValueError, match="length must be int32"):
        call(length=tl[:-1])
    with pytest.raises(ValueError, match="hidden0 must be float32"):
        call(hidden0=th[:, :8])
    with pytest.raises(ValueError, match=r"order must be int32 \[B\]"):
        call(order=order[:-1])
    with pytest.raises(ValueError, match=r"segments must be int32 \[3, 4, 2\]"):
        call(seg=seg[:2])
    with pytest.raises(ValueError, match="segments must be int32 .* on cpu"):
        call(seg=seg.to("meta"))
    with pytest.raises(ValueError, match="nets must hold 1..64 groups"):
        call(nets=[])
    w, b, c = pn[1][2].memory
    pn[1][2].memory = (w.detach().double(), b, c)
    with pytest.raises(ValueError, match=r"group 1, species 3\): memory Linear weight must be float32 on cpu"):
        call()
    pn[1][2].memory = (w, b, c)
    # gradients only where asked
    params[0][0][0].requires_grad_(False)
    out = call()
    out[1].sum().backward()
    assert params[0][0][0].grad is None and params[0][0][2].grad is not None
    assert params[2][0][-1].grad is not None                                   # the memory head's bias, through h


# ---- 7. act()'s bits through a window, per group ------------------------------------------------
def test_same_bits_as_act_through_the_window():
    u.check_window_bits_groups("cpu")


# ---- 8. the harness -----------------------------------------------------------------------------
def test_harness_grouped_evaluate_leaves_the_loop_s_parameters():
    """harness/a2c_recurrent_groups.py in CPU mode, three groups of recurrent
    nets that own their parameters, two updates: --grouped-evaluate leaves every
    parameter bit for bit where the default path leaves it."""
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c_recurrent
    import a2c_recurrent_groups
    after = []
    for flag in (False, True):
        sim = mb.SimManager(0, 6, 69, 8, exec_mode="cpu")
        modules = [a2c_recurrent.make_modules(H, "cpu", seed=10 + i) for i, H in enumerate((16, 32, 16))]
        optimizers = [[torch.optim.Adam(m.parameters(), lr=1e-3) for m in four] for four in modules]
        before = [p.detach().clone() for four in modules for m in four for p in m.parameters()]
        losses = a2c_recurrent_groups.train(sim, [0, 2, 4], modules, optimizers, iters=2, horizon=4,
                                            grouped_evaluate=flag)
        assert len(losses) == 2 and len(losses[0]) == 3 and np.isfinite(losses).all()
        after.append([p.detach().clone() for four in modules for m in four for p in m.parameters()])
        assert sum(not torch.equal(a, b) for a, b in zip(before, after[-1])) >= len(before) // 2
    assert all(torch.equal(a, b) for a, b in zip(*after))
