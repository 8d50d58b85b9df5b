"""PPO on the device for the padded [L, B] sequence batches, host tensors
(DESIGN.md "PPO on the device"): mbots_policy_seq_adv_moments and
mbots_policy_seq_ppo_loss against their float32 restatement bit for bit, the
options, the refusals, and harness/ppo_recurrent_groups.py in CPU mode.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import policy_ppo_ref as pr
import policy_ppo_util as u

t = u.t


@pytest.fixture(scope="module")
def seqs():
    return u.seq_case()


def same(got, want):
    for name, a, b in zip(("g_logp", "g_value", "g_entropy"), got, want):
        assert np.array_equal(pr.bits32(a), pr.bits32(b)), name
    assert np.array_equal(pr.bits64(got[3]), pr.bits64(want[3])), "stats"
    if want[4] is not None:
        assert np.array_equal(pr.bits64(got[4]), pr.bits64(want[4])), "moments"


def test_case_covers_the_chunks_and_every_branch_of_the_kept_count(seqs):
    SK, L, last = pr.SEQ_CHUNK, u.SEQ_L, u.SEQ_LAST_TABLE
    lengths = {int(b - a) for a, b in seqs["segments"].reshape(-1, 2)}
    assert lengths >= {0, 1, 255, 256, 257, SK - 1, SK, SK + 1, 2 * SK + 3}
    ln, t0, end, kept = seqs["len"], seqs["t0"], seqs["end"], seqs["kept"]
    reset = end == pr.END_RESET
    branches = {"empty": ln == 0, "whole": (ln > 0) & (kept == ln), "cut by the bound": (t0 + ln > last) & (t0 < last),
                "dropped by the bound": (ln > 0) & (t0 >= last),
                "reset, last row dropped": reset & (ln > 0) & (t0 + ln <= last) & (kept == ln - 1),
                "reset, bound already dropped it": reset & (t0 + ln > last) & (t0 < last) & (kept == last - t0),
                "reset of one row": reset & (ln == 1) & (kept == 0) & (t0 < last)}
    for name, m in branches.items():
        assert m.sum() >= 20, name
    assert seqs["rows"][0] > 0 and seqs["rows"][1] > 0 and seqs["rows"][2] == 0
    assert sorted(seqs["order"].tolist()) == list(range(seqs["B"]))


@pytest.mark.parametrize("opt", [dict(), dict(moments=False), dict(value_clip=False), dict(last_table=-1)],
                         ids=("all", "no-moments", "no-value-clip", "no-bound"))
def test_loss_and_moments_equal_the_float32_restatement(seqs, opt):
    import madrona_bots as mb
    got, want = u.run_seq(mb, seqs, "cpu", **opt), u.ref_seq(seqs, **opt)
    same(got, want)
    assert (got[3][:2, :4] != 0).all() and not got[3][2].any()
    L, B = seqs["cols"][0].shape
    last = opt.get("last_table", u.SEQ_LAST_TABLE)
    kept = pr.seq_kept(seqs["len"], seqs["t0"], seqs["end"], last, L)
    named = np.zeros(B, bool)
    for lo, hi in seqs["segments"][:2].reshape(-1, 2):                         # (group 2 has rows == 0: passed over)
        named[seqs["order"][lo:hi]] = True
    off = ~((np.arange(L)[:, None] < kept[None, :]) & named[None, :])
    assert off.sum() > B and all(not pr.bits32(x)[off].any() for x in got[:3])  # +0, not -0
    if got[4] is not None:
        assert got[4][2, 0] > 0                                                # the moments do not look at rows


def test_stats_accumulate_and_old_value_may_be_absent(seqs):
    import madrona_bots as mb
    once = u.ref_seq(seqs)[3]
    got = u.run_seq(mb, seqs, "cpu", stats=once.copy())
    same(got, u.ref_seq(seqs, stats=once))
    assert not np.array_equal(got[3][:2], once[:2]) and not got[3][2].any()
    none = dict(seqs, cols=seqs["cols"][:4] + [None] + seqs["cols"][5:])
    same(u.run_seq(mb, none, "cpu"), u.ref_seq(seqs, value_clip=False))


def test_refusals(seqs):
    import madrona_bots as mb
    bad = u.seq_case(bad_order=True)
    with pytest.raises(RuntimeError, match=r"order\[\d+\] = -1 is outside the \d+ sequences"):
        u.run_seq(mb, bad, "cpu")
    cols = [t(c) for c in seqs["cols"]]
    meta = [t(seqs[k]) for k in ("len", "t0", "end", "order", "segments")]
    rows = t(seqs["rows"])
    with pytest.raises(ValueError, match="clip must lie"):
        mb.ppo_loss_sequences(*cols, *meta, rows, clip=1.5)
    with pytest.raises(ValueError, match="old_logp must be float32"):
        mb.ppo_loss_sequences(*cols[:3], cols[3][:, :9], *cols[4:], *meta, rows)
    with pytest.raises(ValueError, match="length must be int32"):
        mb.ppo_loss_sequences(*cols, meta[0][:5], *meta[1:], rows)
    with pytest.raises(ValueError, match="t0 must be int32"):
        mb.ppo_loss_sequences(*cols, meta[0], meta[1].long(), *meta[2:], rows)
    with pytest.raises(ValueError, match="stats must be"):
        mb.ppo_loss_sequences(*cols, *meta, rows, stats=torch.zeros(3, 6))
    with pytest.raises(ValueError, match="adv must be float32"):
        mb.advantage_moments_sequences(cols[5].double(), *meta)
    with pytest.raises(ValueError, match="moments must be"):
        mb.advantage_moments_sequences(cols[5], *meta, moments=torch.zeros(3, 3))
    long = seqs["len"].copy()
    long[seqs["order"][int(seqs["segments"][0, 2, 0])]] = u.SEQ_L + 1
    with pytest.raises(RuntimeError, match="is outside"):
        mb.ppo_loss_sequences(*cols, t(long), *meta[1:], rows)


def harness_run(exec_mode, device):
    """harness/ppo_recurrent_groups.py: 64 worlds, four groups of recurrent
    nets -- the last one's range starts past the manager's worlds -- two
    updates of three epochs; the parameters before and after, and the log."""
    import madrona_bots as mb
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(mb.__file__)), "..", "harness"))
    import ppo_recurrent_groups as prg
    sim = mb.SimManager(0, 64, 69, 8, exec_mode=exec_mode)
    modules = prg.make_groups((16, 32, 16, 32), device, seed=20)
    before = [[p.detach().cpu().clone() for m in four for p in m.parameters()] for four in modules]
    log = prg.train(sim, [0, 21, 42, 64], modules, iters=2, horizon=4, epochs=3, lr=1e-3, max_grad_norm=0.5)
    after = [[p.detach().cpu().clone() for m in four for p in m.parameters()] for four in modules]
    return before, after, log


def test_harness_ppo_recurrent_groups_in_cpu_mode():
    before, after, log = harness_run("cpu", "cpu")
    assert len(log) == 2
    for rec in log:
        st = np.array(rec["stats"])
        assert st.shape == (3, 4, 6) and np.isfinite(st).all()
        assert rec["rows"][3] == 0 and not st[:, 3].any() and all(r > 0 for r in rec["rows"][:3])
        assert (st[1:, :3, 4] > 0).all() and (st[:, :3, 0] != 0).all()          # KL > 0 from the second epoch on
    same_bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert all(same_bits(a, b) for a, b in zip(before[3], after[3]))
    for g in range(3):
        assert sum(not same_bits(a, b) for a, b in zip(before[g], after[g])) >= len(before[g]) // 2
