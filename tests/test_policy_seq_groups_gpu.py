"""GPU: madrona_bots.sequence_segments and evaluate_sequences_groups on the
device (DESIGN.md "Grouped evaluate_sequences": the counting sort,
policy_seq_eval_groups_kernel, the backward's waves and their reduce) on the
fixture of tests/policy_seq_groups_util.py -- against the CPU path, bit for
bit; twice in a row; against act() on a grouped manager through a window;
recorded into a graph that is replayed on other rows, another order and other
segments; and the clamp of an order entry outside the batch."""
import numpy as np
import pytest
import torch

import policy_seq_groups_util as u

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def grouped():
    return u.run_grouped(*u.fixture(), device=DEV)


def test_sequence_segments_equals_the_cpu_path():
    import madrona_bots as mb
    net_id = u.fixture()[1]
    for ids, groups in ((net_id, u.G), (net_id, 64), (net_id[:1], 1), (net_id[:1024], 2), (net_id[:1025], 3),
                        (np.full(1500, 7, np.int32), 2), (np.full(70, -1, np.int32), 1)):
        t = torch.from_numpy(np.ascontiguousarray(ids))
        order, seg = mb.sequence_segments(t.to(DEV), groups)
        want_order, want_seg = mb.sequence_segments(t, groups)
        assert order.device.type == "cuda" and seg.device.type == "cuda"
        assert torch.equal(order.cpu(), want_order) and torch.equal(seg.cpu(), want_seg), (len(ids), groups)


def test_device_equals_cpu_path(grouped):
    u.assert_same(grouped, u.cpu_grouped(), "device against the CPU path")
    assert all(float(o.abs().max()) > 0 for o in grouped[0])


def test_two_calls_in_a_row_agree(grouped):
    u.assert_same(u.run_grouped(*u.fixture(), device=DEV), grouped, "second device call")


def test_same_bits_as_act_through_the_window():
    u.check_window_bits_groups("hip")


def variant():
    """The fixture with other rows, another order and other segments: the
    columns reversed (so every net's columns lie elsewhere) and species 1 and 2
    of group 1 exchanged (so the segments' bounds move)."""
    nets, net_id, obs, action, length, hidden0, g = u.fixture()
    rev = lambda a, axis: np.ascontiguousarray(np.flip(a, axis=axis))
    net_id2 = rev(net_id, 0).copy()
    a, b = net_id2 == 4, net_id2 == 5
    net_id2[a], net_id2[b] = 5, 4
    return nets, net_id2, rev(obs, 1), rev(action, 1), rev(length, 0), rev(hidden0, 0), [rev(gi, 1) for gi in g]


def test_graph_capture_and_replay_on_other_contents(grouped):
    """sequence_segments, forward and backward recorded once after one warm
    call (one stream, nothing forked, no queue setting touched), replayed on
    other rows with another order and other segments, then on the fixture's
    own: each replay equals the CPU path of those contents."""
    import madrona_bots as mb
    fx = u.fixture()
    nets = fx[0]
    pn, params = u.policy_nets(nets, DEV)
    tid, to, ta, tl, th, *tg = u.to(DEV, *fx[1:6], *fx[6])
    live = [q for four in params for ps in four for q in ps or [] if q is not None]

    def call():
        order, seg = mb.sequence_segments(tid, u.G)          # recorded too: a replay sorts the net ids of then
        out = mb.evaluate_sequences_groups(pn, to, ta, tl, th, order, seg, return_hidden=True)
        return list(out), torch.autograd.grad(sum((gi * oi).sum() for gi, oi in zip(tg, out)), live)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                               # the warm call: the workspace exists from here on
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = call()
    other = variant()
    assert not np.array_equal(other[1], fx[1])
    for contents, want in ((other, u.run_grouped(*other)), (fx, u.cpu_grouped())):
        new = u.to(DEV, *contents[1:6], *contents[6])
        for dst, src in zip([tid, to, ta, tl, th] + tg, new):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for k, a, b in zip(("logp", "value", "entropy", "hidden"), out, want[0]):
            assert torch.equal(a.detach().cpu(), b), k
        flat = [q for four in want[1] for ps in four for q in ps or [] if q is not None]
        assert len(flat) == len(grads) and all(torch.equal(a.cpu(), b) for a, b in zip(grads, flat))


def test_order_entry_outside_the_batch_is_a_column_of_length_zero(grouped):
    """An order entry outside [0, B) inside a segment is read as a column of
    length 0 that is neither read nor written: the run equals, in every output
    bit and every gradient bit, the run in which that position's column has
    length 0 (whose outputs are the zero launch's +0 either way)."""
    import madrona_bots as mb
    nets, net_id, obs, action, length, hidden0, g = u.fixture()
    B = len(net_id)
    order, seg = mb.sequence_segments(torch.from_numpy(net_id), u.G)
    for bad in (B + 5, -3):
        want_len = length.copy()
        bad_order = order.clone()
        for pair, at in (((1, 0), 5), ((0, 0), 64 * 256), ((2, 2), 62)):       # mid tile, the wrapped tile, a last row
            lo, hi = (int(v) for v in seg[pair])
            p = min((q for q in range(lo, hi) if length[int(order[q])] > 0), key=lambda q: abs(q - lo - at))
            want_len[int(order[p])] = 0
            bad_order[p] = bad
        want = u.run_grouped(nets, net_id, obs, action, want_len, hidden0, g, DEV)
        got = u.run_grouped(nets, net_id, obs, action, length, hidden0, g, DEV,
                            order_seg=(bad_order.to(DEV), seg.to(DEV)))
        u.assert_same(got, want, f"order entry {bad}")
