"""CPU mode: madrona_bots.evaluate_groups and its backward pass (DESIGN.md
"Grouped evaluate"; mbots_policy_eval_groups / mbots_policy_grad_groups on the
host path) against the per-net evaluate() loop over .tolist() slices, bit for
bit, on the fixture of tests/policy_eval_groups_util.py: outputs and every
gradient, the rows of no net, one net for four species, independence of the
host's thread count, the refusals, and the harness's --grouped-evaluate."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_eval_groups_util as u
import policy_grad_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def loop():
    """The per-net loop's result on the fixture, computed once."""
    nets, seg, n, obs, hidden, action, g = u.fixture()
    return u.run_loop(nets, seg, obs, hidden, action, g)


@pytest.fixture(scope="module")
def grouped():
    nets, seg, n, obs, hidden, action, g = u.fixture()
    return u.run_grouped(nets, seg, obs, hidden, action, g)


def test_fixture_covers_the_lengths():
    nets, seg, n, *_ = u.fixture()
    lens = (seg[..., 1] - seg[..., 0]).ravel().tolist()
    assert set(lens) == {0, 1, 63, 64, 65, 64 * 256 + 1} and u.LENGTHS[0][0] == 64 * 256 + 1
    assert seg[seg[..., 1] > seg[..., 0]].min() == 1 and seg.max() < n        # a gap before and a gap after
    assert [a[0] for a in u.ARCH] == [16, 128, 64] and nets[2][3] is None


# ---- 1. outputs and every gradient ----------------------------------------------
def test_outputs_and_gradients_equal_the_per_net_loop(loop, grouped):
    u.assert_same(grouped, loop, "cpu")
    # (the comparison is not one of zeros)
    assert all(float(o.abs().max()) > 0 for o in grouped[0])
    assert all(float(q.abs().max()) > 0 for q in grouped[1][0][0] + grouped[1][1][3] + grouped[1][2][1])
    assert all(not q.any() for q in grouped[1][0][1])                         # the empty segment: zeros


# ---- 2. rows of no segment, or of a pair without a net ----------------------------
def test_rows_outside_are_zero_and_change_nothing(grouped):
    nets, seg, n, obs, hidden, action, g = u.fixture()
    outside = u.outside_rows(seg, n, nets)
    assert outside.sum() == u.GAP_BEFORE + u.GAP_AFTER + u.LENGTHS[2][3]
    for o in grouped[0]:
        assert not o.view(torch.int32)[torch.from_numpy(outside)].any()       # +0, bit for bit
    rng = np.random.default_rng(5)
    obs2, hidden2, action2 = obs.copy(), hidden.copy(), action.copy()
    k = int(outside.sum())
    obs2[outside] = rng.normal(0, 1e6, (k, 69)).astype(np.float32)
    obs2[np.nonzero(outside)[0][0]] = np.nan
    hidden2[outside] = 3.0
    action2[outside] = 77                                                     # never looked at
    g2 = [gi.copy() for gi in g]
    for gi in g2:
        gi[outside] = 1e30
    again = u.run_grouped(nets, seg, obs2, hidden2, action2, g2)
    u.assert_same(again, grouped, "outside rows changed")


# ---- 3. one group, one net for all four species -----------------------------------
def test_one_net_for_four_species_equals_four_evaluate_calls():
    """Outputs bit for bit.  The net's parameters are shared by the four
    segments, so each gradient is autograd's sum of four per-segment gradients
    in torch's order: against the four evaluate() calls' gradients g_i (bitwise
    those of nets that own their parameters, test 1) it may differ by the
    three roundings of a four-term f32 sum, each at most 2^-24 of a partial
    sum that sum |g_i| bounds."""
    import madrona_bots as mb
    nets, _, _, obs, hidden, action, g = u.fixture()
    d = nets[0][0]
    lengths = [[65, 1, 64, 63]]
    seg, n = u.segments_of(lengths, [(0, 2), (0, 0), (0, 3), (0, 1)])
    obs, action, g = obs[:n], action[:n], [gi[:n] for gi in g]
    ref = u.run_loop([[d, d, d, d]], seg, obs, None, action, g)               # four nets that own their copies
    net, ps = gr.policy_net(d)
    to, ta, ts, *tg = u.to("cpu", obs, action, seg, *g)
    for form in (net, [net] * 4):
        for q in ps:
            q.grad = None
        out = mb.evaluate_groups([form], to, ta, ts)
        sum((gi * oi).sum() for gi, oi in zip(tg, out)).backward()
        for a, b in zip(out, ref[0]):
            assert torch.equal(a.detach(), b)
        for i, q in enumerate(ps):
            parts = torch.stack([ref[1][0][s][i] for s in range(4)]).double()
            bound = 3 * 2.0 ** -24 * parts.abs().sum(0)
            assert bool(((q.grad.double() - parts.sum(0)).abs() <= bound).all()), i


# ---- 4. the host's thread count -----------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, {tests!r})
import conftest   # the suite's import paths
import policy_eval_groups_util as u
nets, seg, n, obs, hidden, action, g = u.fixture()
print(u.digest(u.run_grouped(nets, seg, obs, hidden, action, g)))
"""


def test_bits_do_not_depend_on_host_threads(grouped):
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"))
    procs = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, text=True,
                              env=dict(os.environ, MBOTS_CPU_THREADS=t)) for t in ("1", "5", "16")]
    outs = [p.communicate()[0].split() for p in procs]
    assert all(p.returncode == 0 for p in procs)
    assert outs[0] == outs[1] == outs[2] == [u.digest(grouped)]


# ---- 5. refusals ------------------------------------------------------------------------
def test_refusals():
    import madrona_bots as mb
    nets, seg, n, obs, hidden, action, g = u.fixture()
    pn, params = u.policy_nets(nets)
    to, th, ta, ts = u.to("cpu", obs, hidden, action, seg)

    def bad_segments(g_, s_, lo, hi):
        s2 = ts.clone()
        s2[g_, s_, 0], s2[g_, s_, 1] = lo, hi
        return s2
    lo, hi = seg[1, 0]
    with pytest.raises(RuntimeError, match="group 1 species 1 and group 0 species 2 overlap"):
        mb.evaluate_groups(pn, to, ta, bad_segments(0, 1, hi - 1, hi + 0), th)
    with pytest.raises(RuntimeError, match=r"group 2 species 3 is not inside the \d+ rows"):
        mb.evaluate_groups(pn, to, ta, bad_segments(2, 2, n - 3, n + 1), th)
    with pytest.raises(RuntimeError, match="group 0 species 4 is not inside"):
        mb.evaluate_groups(pn, to, ta, bad_segments(0, 3, -1, 0), th)
    with pytest.raises(RuntimeError, match="group 1 species 2 is not inside"):
        mb.evaluate_groups(pn, to, ta, bad_segments(1, 1, 9, 8), th)
    with pytest.raises(ValueError, match="segments must be int32"):
        mb.evaluate_groups(pn, to, ta, ts.long(), th)
    with pytest.raises(ValueError, match=r"segments must be int32 \[3, 4, 2\]"):
        mb.evaluate_groups(pn, to, ta, ts[:2], th)
    with pytest.raises(ValueError, match="segments must be int32 .* on cpu"):
        mb.evaluate_groups(pn, to, ta, ts.to("meta"), th)
    with pytest.raises(ValueError, match="obs must be float32"):
        mb.evaluate_groups(pn, to.double(), ta, ts, th)
    with pytest.raises(ValueError, match="action must be int32"):
        mb.evaluate_groups(pn, to, ta.long(), ts, th)
    with pytest.raises(ValueError, match="hidden .* is needed"):
        mb.evaluate_groups(pn, to, ta, ts)
    with pytest.raises(ValueError, match="hidden must be float32"):
        mb.evaluate_groups(pn, to, ta, ts, th.double())
    with pytest.raises(ValueError, match="nets must hold 1..64 groups"):
        mb.evaluate_groups([], to, ta, ts, th)
    with pytest.raises(ValueError, match=r"nets\[1\] must be four PolicyNet"):
        mb.evaluate_groups([pn[0], pn[1][:3], pn[2]], to, ta, ts, th)
    # an action outside 0..5 inside a segment, and a parameter of another dtype: the pair is named
    a2 = ta.clone()
    a2[int(seg[2, 1, 0])] = 6
    with pytest.raises(RuntimeError, match="group 2 species 2: action 6 of row 0 is outside 0..5"):
        mb.evaluate_groups(pn, to, a2, ts, th)
    w, b, c = pn[1][2].actor[0]
    pn[1][2].actor[0] = (w.detach().double(), b, c)
    with pytest.raises(ValueError, match=r"group 1, species 3\): actor Linear 0 weight must be float32 on cpu"):
        mb.evaluate_groups(pn, to, ta, ts, th)
    pn[1][2].actor[0] = (w, b, c)
    # gradients only where asked
    params[0][0][0].requires_grad_(False)
    out = mb.evaluate_groups(pn, to, ta, ts, th)
    out[1].sum().backward()
    assert params[0][0][0].grad is None and params[0][0][2].grad is not None
    assert params[2][0][-1].grad is not None and not params[2][0][-5].grad.any()      # the actor: never g_value


# ---- 6. the harness ------------------------------------------------------------------------
def test_harness_grouped_evaluate_leaves_the_loop_s_parameters():
    """harness/a2c_groups.py in CPU mode, three groups of nets that own their
    parameters, two updates: --grouped-evaluate leaves every parameter bit for
    bit where the default path leaves it."""
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import a2c
    import a2c_groups
    after = []
    for flag in (False, True):
        sim = mb.SimManager(0, 6, 69, 8, exec_mode="cpu")
        modules = [a2c.make_modules(H, "cpu", seed=10 + i) for i, H in enumerate((16, 32, 16))]
        optimizers = [[torch.optim.Adam(m.parameters(), lr=1e-3) for m in four] for four in modules]
        before = [p.detach().clone() for four in modules for m in four for p in m.parameters()]
        losses = a2c_groups.train(sim, [0, 2, 4], modules, optimizers, iters=2, horizon=4, grouped_evaluate=flag)
        assert len(losses) == 2 and len(losses[0]) == 3 and np.isfinite(losses).all()
        after.append([p.detach().clone() for four in modules for m in four for p in m.parameters()])
        assert sum(not torch.equal(a, b) for a, b in zip(before, after[-1])) >= len(before) // 2
    assert all(torch.equal(a, b) for a, b in zip(*after))
