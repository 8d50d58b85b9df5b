"""The sequence loss on host tensors (DESIGN.md "Device learner step"):
mbots_policy_seq_group_rows and mbots_policy_seq_a2c_loss against the harness's
own keep mask and torch autograd of its per_element composition, against the
float32 restatement bit for bit and against math.fsum within the bound of the
summation order, and the wrappers' refusals.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import policy_seq_loss_ref as sr
import policy_seq_loss_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd", "harness"))

END_RESET = 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def case():
    return u.seq_case()


@pytest.fixture(scope="module", params=[u.LAST_TABLE, -1], ids=["last_table_4", "no_bound"])
def run(request, case):
    """(last_table, the library's outputs, the restatement's) -- computed once."""
    import madrona_bots as mb
    last = request.param
    got = u.seq_run(mb, case, "cpu", last)
    order, seg, rows = got[:3]
    ref = sr.seq_loss_f32(case["logp"], case["value"], case["entropy"], case["adv"], case["ret"], case["length"],
                          case["t0"], case["end"], order, seg, rows, last)
    return last, got, ref


def harness_keep(case, last_table):
    """keep [L, B] float32 as harness/a2c_recurrent_groups.window_batch builds
    it (rows >= 0 there is k < len, as batch() documents)."""
    c = u.seq_tensors(case, "cpu")
    k = torch.arange(u.SEQ_L, dtype=torch.int32)[:, None]
    keep = k < c["length"][None, :]
    if last_table >= 0:
        keep = keep & (c["t0"][None, :] + k < last_table)
    keep &= ~((c["end"] == END_RESET)[None, :] & (k == c["length"][None, :] - 1))
    return keep.to(torch.float32)


def group_of(case):
    """The group of every column, -1 where its net_id names no net."""
    ids = case["net_id"].astype(np.int64)
    return np.where((ids >= 0) & (ids < 4 * u.SEQ_G), ids // 4, -1)


def test_case_covers_what_it_claims(case, run):
    last, (order, seg, rows, *_), _ = run
    sizes = (seg[:, :, 1] - seg[:, :, 0]).tolist()
    assert sizes == u.PAIRS and sizes[0][0] > 4 * 256 and 0 in sizes[0]
    assert set(case["length"].tolist()) == set(range(u.SEQ_L + 1)) and set(case["end"].tolist()) == {0, 1, 2, 3}
    assert (group_of(case) < 0).sum() == u.SEQ_B - sum(map(sum, u.PAIRS)) > 0
    keep = sr.keep_mask(u.SEQ_L, case["length"], case["t0"], case["end"], last)
    inside = np.arange(u.SEQ_L)[:, None] < case["length"][None, :]
    if last >= 0:
        cut = (inside & ~keep).sum(axis=0) * keep.sum(axis=0)       # columns both kept and cut
        assert (cut > 0).sum() > 100 and rows[u.DEAD_GROUP] == 0 and seg[u.DEAD_GROUP, :, 1].max() > 0
    else:
        assert rows[u.DEAD_GROUP] > 0


def test_rows_equal_the_harness_keep_sum(case, run):
    last, (order, seg, rows, *_), _ = run
    keep = harness_keep(case, last)
    group = torch.from_numpy(group_of(case))
    want = [int(keep[:, group == g].sum()) for g in range(u.SEQ_G)]
    assert rows.tolist() == want
    assert rows.tolist() == sr.group_rows(u.SEQ_L, case["length"], case["t0"], case["end"], order, seg, last).tolist()
    assert np.array_equal(keep.numpy() != 0, sr.keep_mask(u.SEQ_L, case["length"], case["t0"], case["end"], last))


def test_gradients_equal_torch_autograd_of_the_harness_composition(case, run):
    """Element by element, no sum involved: the bits on every counted element,
    and +0 on every other one (where torch's product with a zero weight leaves
    a zero of either sign)."""
    import a2c_recurrent_groups as h
    last, (order, seg, rows, g_logp, g_value, g_entropy, _), _ = run
    c = u.seq_tensors(case, "cpu")
    keep = harness_keep(case, last)
    group = torch.from_numpy(group_of(case))
    total = torch.from_numpy(rows).to(torch.float32).clamp_(min=1.0)
    weight = torch.where(group >= 0, (1.0 / total)[group.clamp(min=0)], torch.zeros(()))
    outs = [c[k].clone().requires_grad_() for k in ("logp", "value", "entropy")]
    per = h.per_element(*outs, c["adv"], c["ret"], 0.5, 0.01) * (keep * weight[None, :])
    per.sum().backward()
    counted = (keep * weight[None, :]).numpy() != 0
    assert counted.sum() == rows.sum()
    for got, x in zip((g_logp, g_value, g_entropy), outs):
        want = x.grad.numpy()
        assert np.array_equal(bits(got)[counted], bits(want)[counted])
        assert not bits(got)[~counted].any() and not want[~counted].any()


def test_outputs_equal_the_float32_restatement(run):
    _, got, ref = run
    for a, b in zip(got[3:6], ref[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(got[6].view(np.uint64), ref[3].view(np.uint64))


def test_loss_against_fsum(case, run):
    """|loss - fsum| <= n 2^-53 sum |per_row|, n the additions on the longest
    chain: ceil(columns / 256) * L into an accumulator, 256 across them, 4 across
    the species and the one onto loss."""
    last, (order, seg, rows, *_, loss), ref = run
    per = ref[4]
    for g in range(u.SEQ_G):
        cols = np.concatenate([order[lo:hi] for lo, hi in seg[g]])
        vals = per[:, cols].astype(np.float64).reshape(-1).tolist()
        exact = math.fsum(vals)
        n = max(-(-int(hi - lo) // 256) for lo, hi in seg[g]) * u.SEQ_L + 256 + 4 + 1
        bound = n * 2.0 ** -53 * math.fsum(abs(x) for x in vals)
        print(f"group {g}: loss {loss[g]!r}, |error| {abs(loss[g] - exact):.3e}, bound {bound:.3e}")
        assert abs(loss[g] - exact) <= bound
        assert (rows[g] == 0) == (loss[g] == 0.0)


def test_loss_accumulates_and_a_dead_group_is_not_touched(case):
    import madrona_bots as mb
    start = np.array([1.5, -2.25, -0.0], np.float64)
    got = u.seq_run(mb, case, "cpu", u.LAST_TABLE, loss=start)
    order, seg, rows = got[:3]
    ref = sr.seq_loss_f32(case["logp"], case["value"], case["entropy"], case["adv"], case["ret"], case["length"],
                          case["t0"], case["end"], order, seg, rows, u.LAST_TABLE, loss=start)
    assert np.array_equal(got[6].view(np.uint64), ref[3].view(np.uint64))
    assert got[6].view(np.uint64)[u.DEAD_GROUP] == start.view(np.uint64)[u.DEAD_GROUP]      # -0.0 stays -0.0
    dead = np.concatenate([order[lo:hi] for lo, hi in seg[u.DEAD_GROUP]])
    assert len(dead) and not any(bits(g)[:, dead].any() for g in got[3:6])


def test_refusals_name_the_argument_or_the_pair(case):
    import madrona_bots as mb
    c = u.seq_tensors(case, "cpu")
    order, seg = mb.sequence_segments(c["net_id"], u.SEQ_G)
    rows = torch.ones(u.SEQ_G, dtype=torch.int64)
    cols = [c[k] for k in ("logp", "value", "entropy", "adv", "ret")]
    meta = [c["length"], c["t0"], c["end"], order, seg, rows]

    def loss(cols=cols, meta=meta, **kw):
        return mb.a2c_loss_sequences(*cols, *meta, u.LAST_TABLE, **kw)

    with pytest.raises(ValueError, match=r"value must be float32 \[3, 2400\]"):
        loss(cols=[cols[0], cols[1][:, :-1], *cols[2:]])
    with pytest.raises(ValueError, match="adv must be float32"):
        loss(cols=[*cols[:3], cols[3].double(), cols[4]])
    with pytest.raises(ValueError, match="ret must be float32.*on cpu"):
        loss(cols=[*cols[:4], cols[4].to("meta")])
    with pytest.raises(ValueError, match="logp must be float32 \\[L, B\\]"):
        loss(cols=[cols[0][0], *cols[1:]])
    with pytest.raises(ValueError, match=r"t0 must be int32 \[2400\]"):
        loss(meta=[meta[0], meta[1].long(), *meta[2:]])
    with pytest.raises(ValueError, match="length must be int32"):
        loss(meta=[meta[0][:-1], *meta[1:]])
    with pytest.raises(ValueError, match="segments must be int32"):
        loss(meta=[*meta[:4], seg.reshape(-1, 2), rows])
    with pytest.raises(ValueError, match="rows must be a contiguous int64"):
        loss(meta=[*meta[:5], rows.to(torch.int32)])
    with pytest.raises(ValueError, match="loss must be a contiguous float64"):
        loss(loss=torch.zeros(u.SEQ_G))
    with pytest.raises(ValueError, match="order must be int32"):
        mb.sequence_group_rows(meta[0], meta[1], meta[2], order.long(), seg, rows.clone())
    with pytest.raises(ValueError, match="rows must be a contiguous int64"):
        mb.sequence_group_rows(meta[0], meta[1], meta[2], order, seg, torch.zeros(u.SEQ_G + 1, dtype=torch.int64))

    # the host path reads the segments and every column they name
    outside = seg.clone()
    outside[1, 3, 1] = u.SEQ_B + 1
    for call in (lambda s, o: loss(meta=[*meta[:3], o, s, rows]),
                 lambda s, o: mb.sequence_group_rows(meta[0], meta[1], meta[2], o, s, rows.clone(), u.LAST_TABLE)):
        with pytest.raises(RuntimeError, match=r"segment \[\d+, 2401\) of group 1 species 4 is not inside the 2400"):
            call(outside, order)
        twice = order.clone()
        lo = int(seg[0, 2, 0])
        twice[lo + 5] = twice[lo + 1]
        with pytest.raises(RuntimeError, match=rf"group 0 species 3: order\[{lo + 5}\] = \d+ names a sequence a second time"):
            call(seg, twice)
        beyond = order.clone()
        beyond[int(seg[1, 0, 0])] = u.SEQ_B
        with pytest.raises(RuntimeError, match=r"group 1 species 1: order\[\d+\] = 2400 is outside the 2400 sequences"):
            call(seg, beyond)
    long = c["length"].clone()
    long[int(order[0])] = u.SEQ_L + 1
    with pytest.raises(RuntimeError, match=r"group 0 species 1: length 4 of sequence \d+ is outside \[0, 3\]"):
        loss(meta=[long, *meta[1:]])
