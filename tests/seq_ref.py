"""Helpers of the sequence tests (test_seq_*.py): the numpy restatement of
include/mbots.h "Sequences for a recurrent learner" -- it works from a window's
pushed columns and compute()'s next / end alone --, a recorder of what the
learner would keep per table, the scenarios, and the bodies both execution
modes run (make: a manager factory).  Every comparison is bitwise; floats go
through a uint32 view (health's int32 bits are not comparable as floats)."""
import numpy as np
import pytest
import torch

import traj_util as tu

PARAMS = tu.PARAMS[1]
W20, A20, MAX_ROWS = 20, 32, 8192
SPLITS = ((0, 1), (1, 130), (130, None))
BATCH_KEYS = ("rows", "t0", "len", "end", "obs", "reward", "value", "adv", "ret", "action_in", "hidden0")
PER_SEQ = ("t0", "len", "end", "hidden0")     # [B, ...]; every other key is [L, B, ...]


def cpu(W=W20, A=A20, **kw):
    import madrona_bots as mb
    kw.setdefault("agent_capacity", 128)
    return mb.SimManager(0, W, tu.SEED, A, exec_mode="cpu", **kw)


def hip(W=W20, A=A20, **kw):
    import madrona_bots as mb
    kw.setdefault("agent_capacity", 128)
    return mb.SimManager(0, W, tu.SEED, A, **kw)


def flagged(make, **flags):
    """`make` whose managers open their trajectory window with `flags`, for
    the traj_util scenarios that open the window themselves."""
    def f(*a, **kw):
        m = make(*a, **kw)
        plain = m.trajectory_window
        m.trajectory_window = lambda horizon, max_rows, **k: plain(horizon, max_rows, **{**flags, **k})
        return m
    return f


def small(make):
    """`make` at traj_util's own size (4 worlds x 8 agents)."""
    return lambda *a, **kw: make(tu.W, tu.A, *a, **kw)


ALL = dict(record_obs=True, record_state=True)


def np_(x):
    return x.detach().cpu().numpy().copy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b, where=""):
    assert a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(bits(a), bits(b)), where


def same_dict(a, b, where=""):
    assert sorted(a) == sorted(b), (where, sorted(a), sorted(b))
    for k in a:
        same(a[k], b[k], (where, k))


# ---- the restatement --------------------------------------------------------
def sequences_ref(res):
    """res: to_numpy(compute()).  Sequences in (t0, q0) order: a start is a row
    of table 0 or a row whose link names no row of the table before; it follows
    next to the first row with end != 0.  Returns S, seq_id / seq_pos per
    table, and rows [n, S], t0, len, end [S]."""
    link, nxt, end, rows = res["link"], res["next"], res["end"], res["rows"]
    n = len(rows)
    starts = []
    for t in range(n):
        if t == 0:
            q0 = np.arange(rows[0])
        else:
            q0 = np.nonzero(~((link[t] >= 0) & (link[t] < rows[t - 1])))[0]
        starts += [(t, int(q)) for q in q0]
    S = len(starts)
    sid = [np.full(r, -1, np.int32) for r in rows]
    pos = [np.full(r, -1, np.int32) for r in rows]
    out = {"rows": np.full((n, S), -1, np.int32), "t0": np.zeros(S, np.int32), "len": np.zeros(S, np.int32),
           "end": np.zeros(S, np.int32)}
    for s, (t, q) in enumerate(starts):
        out["t0"][s] = t
        k = 0
        while True:
            assert sid[t][q] == -1
            sid[t][q], pos[t][q] = s, k
            out["rows"][k, s] = q
            if end[t][q] != 0:
                out["len"][s], out["end"][s] = k + 1, end[t][q]
                break
            q = int(nxt[t][q])
            t, k = t + 1, k + 1
    return S, sid, pos, out


class Recorder:
    """after_push hook: what the learner keeps per table today -- clones of
    construct_obs(), action_tensor and hidden_state_tensor."""

    def __init__(self, obs_of=None):
        self.obs, self.action, self.hidden = [], [], []
        self.obs_of = obs_of

    def __call__(self, mgr, t):
        self.obs.append(np_(mgr.construct_obs()) if self.obs_of is None else self.obs_of())
        self.action.append(np_(mgr.action_tensor().to_torch()))
        self.hidden.append(np_(mgr.hidden_state_tensor().to_torch()))


def gather_ref(tables, idx):
    """tables[t]: [N_t, C]; element (k, b) is tables[t0[b] + k][rows[k, b]],
    zeros where rows is -1."""
    n, S = idx["rows"].shape
    C = tables[0].shape[1]
    out = np.zeros((n, S, C), tables[0].dtype)
    for b in range(S):
        for k in range(idx["len"][b]):
            out[k, b] = tables[idx["t0"][b] + k][idx["rows"][k, b]]
    return out


def batch_ref(res, idx, rec):
    """The whole batch [0, S) from compute()'s columns and a Recorder."""
    out = dict(idx)
    for key in ("reward", "value", "adv", "ret"):
        out[key] = gather_ref([x.reshape(-1, 1) for x in res[key]], idx)[:, :, 0]
    out["obs"] = gather_ref(rec.obs, idx)
    masks = [(a != 0).astype(np.uint8) @ (1 << np.arange(6)).astype(np.uint8) for a in rec.action]
    out["action_in"] = gather_ref([m.astype(np.uint8).reshape(-1, 1) for m in masks], idx)[:, :, 0]
    out["hidden0"] = np.stack([rec.hidden[t][idx["rows"][0, b]] for b, t in enumerate(idx["t0"])]) \
        if len(idx["t0"]) else np.zeros((0, 16), np.float32)
    return out


def cut(batch, lo, hi):
    return {k: np.ascontiguousarray(v[lo:hi] if k in PER_SEQ else v[:, lo:hi]) for k, v in batch.items()}


# ---- running a window -------------------------------------------------------
def memory_for(n, t):
    g = torch.Generator().manual_seed(tu.SEED * 104729 + t)
    return torch.randn((n, 16), generator=g, dtype=torch.float32)


def write_memory(mgr, t):
    """before_step hook: the learner's recurrent state of step t."""
    mgr.write_actions(memory=memory_for(mgr.num_agents(), t).to(mgr.device))


def run20(make, *, fixd=False, episode_length=0, rec=None, flags=ALL, before_step=write_memory, **kw):
    """P20 (R20 with episode_length 4): 20 worlds x 32 agents, the breed- and
    shoot-heavy stream, 9 steps, 10 tables."""
    mgr = make(W20, A20, fix_depth_alias=fixd)
    if episode_length:
        mgr.set_episode_length(episode_length)
    win = mgr.trajectory_window(tu.STEPS + 1, MAX_ROWS, **flags)
    if before_step is write_memory:
        write_memory(mgr, 98)          # (table 0 holds a recurrent state too: hidden0 is not all zeros)
    tu.run_window(mgr, with_values=True, win=win, before_step=before_step, after_push=rec, **kw)
    return mgr, win


def numbered(win):
    """compute + sequences: (res, S, seq_id per table, seq_pos per table)."""
    res = tu.to_numpy(win.compute(*PARAMS))
    S = win.sequences()
    n = len(res["rows"])
    return res, S, [np_(win.view(win.SEQ_ID, t)).reshape(-1) for t in range(n)], \
        [np_(win.view(win.SEQ_POS, t)).reshape(-1) for t in range(n)]


def to_np(batch):
    return {k: np_(v) for k, v in batch.items()}


def facts(idx, n):
    """Counts the scenarios are chosen for."""
    ln, t0, end = idx["len"], idx["t0"], idx["end"]
    return {"S": len(ln), "span": int(((t0 == 0) & (ln == n)).sum()), "late": int(((t0 > 0) & (ln >= 2)).sum()),
            "died": int((end == 1).sum()), "reset": int((end == 2).sum()),
            "last": int((t0 == n - 1).sum())}


# ---- bodies both execution modes run ---------------------------------------
def check_numbering(win, where):
    """Test 1 on a pushed window; returns what the device run is compared by."""
    res, S, sid, pos = numbered(win)
    S_ref, sid_ref, pos_ref, idx = sequences_ref(res)
    assert S == S_ref, (where, S, S_ref)
    for t in range(len(res["rows"])):
        same(sid[t], sid_ref[t], (where, "seq_id", t))
        same(pos[t], pos_ref[t], (where, "seq_pos", t))
    allid = np.concatenate(sid)
    assert np.array_equal(np.unique(allid), np.arange(S)), where           # every id occurs
    assert int(idx["len"].sum()) == sum(res["rows"]) == len(allid), where  # sum len = sum N_t
    for s in range(0, S, max(S // 50, 1)):                                  # positions contiguous from 0
        p = np.sort(np.concatenate([pos[t][sid[t] == s] for t in range(len(sid))]))
        assert np.array_equal(p, np.arange(idx["len"][s])), (where, s)
    return {"S": np.array([S]), "sid": np.concatenate(sid), "pos": np.concatenate(pos)}, idx, res


def numbering_scenarios(make):
    out = {}
    mgr, win = tu.scenario_plain(flagged(small(make), sequences=True), True)
    out["P4"], idx, res = check_numbering(win, "P4")
    assert facts(idx, 10)["S"] >= 40
    mgr, win, marks = tu.scenario_reset(flagged(small(make), sequences=True), "flag")
    out["R4"], idx, res = check_numbering(win, "R4")
    f = facts(idx, 10)
    assert f["S"] >= 45 and f["reset"] >= 11, f
    mgr, win = run20(make, flags=dict(sequences=True), before_step=None)
    out["P20"], idx, res = check_numbering(win, "P20")
    f = facts(idx, 10)
    assert min(res["rows"]) >= 640 and max(res["rows"]) > 2 * 256 and max(res["rows"]) % 64, res["rows"]
    assert f["S"] >= 843 and f["span"] >= 499 and f["late"] >= 183 and f["died"] >= 184 and f["last"] >= 20, f
    mgr, win = run20(make, episode_length=4, flags=dict(sequences=True), before_step=None)
    out["R20"], idx, res = check_numbering(win, "R20")
    f = facts(idx, 10)
    assert f["S"] >= 2079 and f["reset"] >= 1319 and f["died"] >= 120 and f["span"] == 0 and f["last"] >= 640, f
    return out


def check_batches(win, rec, where, splits=SPLITS):
    """Test 2 on a pushed, recorded window: batch(0, S) and its pieces against
    the restatement; returns the whole batch."""
    res, S, sid, pos = numbered(win)
    S_ref, _, _, idx = sequences_ref(res)
    assert S == S_ref
    ref = batch_ref(res, idx, rec)
    whole = to_np(win.batch())
    assert tuple(whole) == BATCH_KEYS
    same_dict(whole, ref, where)
    n = len(res["rows"])
    assert ((whole["len"] >= 1) & (whole["len"] <= n)).all() and np.isin(whole["end"], (1, 2, 3)).all()
    pieces = []
    for lo, hi in splits:
        hi = S if hi is None else hi
        part = to_np(win.batch(lo, hi))
        same_dict(part, cut(ref, lo, hi), (where, lo, hi))
        pieces.append(part)
    glued = {k: np.concatenate([p[k] for p in pieces], axis=0 if k in PER_SEQ else 1) for k in BATCH_KEYS}
    same_dict(glued, whole, (where, "glued"))
    # obs with a strict subset of the index keys: the index the decode lacks is
    # the window's own, the caller's arrays are written all the same
    dev = win.view(win.LINK, 0).device
    for keys in (("rows", "obs"), ("t0", "obs"), ("obs",), ("len", "obs", "rows")):
        out = {k: torch.full(whole[k].shape, 77, dtype=torch.from_numpy(whole[k]).dtype, device=dev) for k in keys}
        assert win.batch(out=out) is out
        same_dict(to_np(out), {k: whole[k] for k in keys}, (where, keys))
    lo, hi = 1, min(130, S)
    same_dict(to_np(win.batch(lo, hi, keys=["t0", "obs"])), {k: cut(ref, lo, hi)[k] for k in ("t0", "obs")},
              (where, "t0 + obs, part"))
    return whole, idx, res


def batches_scenario(make, reset, fixd):
    rec = Recorder()
    mgr, win = run20(make, fixd=fixd, episode_length=4 if reset else 0, rec=rec)
    whole, idx, res = check_batches(win, rec, ("R20" if reset else "P20", fixd))
    S, n = len(idx["len"]), len(res["rows"])
    assert S % 64 and (n * S) % 64 and (n * (S - 130)) % 64 and n * S > 64      # partial tiles, and full ones
    assert whole["obs"].any() and whole["action_in"].any() and (whole["rows"] == -1).any()
    assert whole["hidden0"][idx["t0"] == 0].all(axis=1).all() and not whole["hidden0"][idx["t0"] > 0].any()
    if fixd:   # the depth bytes are the record's own 32, not the semantic ones
        assert not np.array_equal(whole["obs"][..., :32], np.abs(whole["obs"][..., 35:67]))
    return whole


def oracle_obs_scenario(make, fixd):
    """Test 3: obs held to the oracle's columns, not to construct_obs."""
    import pyoracle
    from test_parity_gpu import _obs_rows_oracle
    orc = pyoracle.OracleSim(W20, tu.SEED, A20, cap=128)
    rec = Recorder(obs_of=lambda: _obs_rows_oracle(orc, False, fixd).astype(np.float32).copy())

    def before(mgr, t):
        orc.column(pyoracle.COL_ACTION)[:] = tu.breed_shoot(orc.num_agents(), t).numpy()
        orc.step()
    mgr, win = run20(make, fixd=fixd, rec=rec, before_step=before)
    res, S, _, _ = numbered(win)
    _, _, _, idx = sequences_ref(res)
    assert [len(o) for o in rec.obs] == res["rows"]
    got = np_(win.batch(keys=["obs"])["obs"])
    same(got, gather_ref(rec.obs, idx), ("oracle", fixd))
    return got


def gather_scenario(make):
    """Test 4: the learner's own [N_t, 1] f32 and [N_t, 6] int32 tensors."""
    mgr, win = run20(make, flags=dict(sequences=True), before_step=None)
    res, S, _, _ = numbered(win)
    _, _, _, idx = sequences_ref(res)
    g = torch.Generator().manual_seed(7)
    logp = [torch.randn((r, 1), generator=g) for r in res["rows"]]
    act = [torch.randint(-5, 2 ** 31 - 1, (r, 6), generator=g, dtype=torch.int32) for r in res["rows"]]
    out = {}
    for name, tabs in (("logp", logp), ("act", act)):
        ref = gather_ref([x.numpy() for x in tabs], idx)
        dev = [x.to(mgr.device) for x in tabs]
        out[name] = np_(win.gather(dev))
        same(out[name], ref, name)
        assert (out[name][idx["rows"] < 0] == 0).all() and (idx["rows"] < 0).any()
        same(np_(win.gather(dev, 1, 130)), ref[:, 1:130], (name, "part"))
    flat = [x.reshape(-1) for x in logp]                                   # [N_t] is [N_t, 1]
    same(np_(win.gather([x.to(mgr.device) for x in flat])), out["logp"], "flat")
    with pytest.raises(ValueError):
        win.gather([x.to(mgr.device) for x in logp[:-1]])                   # one tensor per table
    with pytest.raises(ValueError):
        win.gather([x.double().to(mgr.device) for x in logp])              # a 4-byte dtype
    return out


def ring_scenario(make):
    """Test 5: horizon 6 chained twice with clear(keep_last): base != 0, the
    kept table's records survive the clear."""
    mgr = make(W20, A20)
    win = mgr.trajectory_window(6, MAX_ROWS, **ALL)
    rec = Recorder()
    tu.run_window(mgr, steps=5, with_values=True, win=win, before_step=write_memory, after_push=rec)
    first, _, _ = check_batches(win, rec, "ring 1", splits=((0, 70), (70, None)))
    win.clear(keep_last=True)
    with pytest.raises(RuntimeError, match=r"status -1"):
        win.batch()                                                         # a clear invalidates
    rec2 = Recorder()
    rec2.obs, rec2.action, rec2.hidden = rec.obs[-1:], rec.action[-1:], rec.hidden[-1:]
    tu.run_window(mgr, steps=5, with_values=True, win=win, first_table=False, t0=5, before_step=write_memory,
                  after_push=rec2)
    second, idx, _ = check_batches(win, rec2, "ring 2", splits=((0, 70), (70, None)))
    assert second["hidden0"][idx["t0"] == 0].any()                          # the kept table's state
    return {"first": first, "second": second}


def growth_scenario(make):
    """Test 6: the capacity grows in-window under the new flags."""
    rec = Recorder()
    mk = flagged(make, **ALL)
    mgr = mk(tu.W, tu.A, agent_capacity="auto")
    for t in range(tu.GROW_PRE):
        mgr.write_actions(tu.breed_turning(mgr.num_agents(), t).to(mgr.device))
        mgr.step()
    cap0 = mgr.agent_capacity
    win = tu.run_window(mgr, steps=tu.GROW_STEPS, with_values=True, t0=tu.GROW_PRE, before_step=write_memory,
                        after_push=rec,
                        actions=lambda n, t: (tu.breed_turning if t < tu.GROW_PRE + 4 else tu.breed_shoot)(n, t))
    assert cap0 == 128 and mgr.agent_capacity == 256
    whole, idx, res = check_batches(win, rec, "growth", splits=((0, 70), (70, None)))
    return whole


def errors_scenario(make):
    """Test 8."""
    import madrona_bots as mb
    mgr = make(tu.W, tu.A)
    blob = mgr.save_checkpoint()
    with pytest.raises(RuntimeError, match=r"status -1"):
        mb._check(mb._lib.mbots_traj_open_ex(mgr._h, 4, 64, 8))             # an unknown flag
    win = mgr.trajectory_window(4, 33, sequences=True)
    assert win.flags == win.FLAG_SEQ
    win.push()
    with pytest.raises(RuntimeError, match=r"status -1"):
        win.sequences()                                                     # no compute yet
    win.compute(0.9)
    with pytest.raises(RuntimeError, match=r"status -1"):
        win.view(win.SEQ_ID, 0)                                             # no sequences yet
    with pytest.raises(RuntimeError, match=r"status -1"):
        win.batch()
    S = win.sequences()
    assert S == tu.W * tu.A and win.view(win.SEQ_POS, 0).shape == (S, 1)
    win.compute(0.5, 0.5, 1.0)                                              # another compute leaves them valid
    b = win.batch()
    assert tuple(b) == ("rows", "t0", "len", "end", "reward", "value", "adv", "ret")
    assert tuple(b["rows"].shape) == (1, S) and (np_(b["end"]) == 3).all()
    for key in ("obs", "action_in", "hidden0"):                             # fields whose flag is off
        with pytest.raises(RuntimeError, match=r"status -1"):
            win.batch(keys=[key])
    with pytest.raises(ValueError):
        win.batch(keys=["nope"])
    with pytest.raises(ValueError):
        win.batch(out={"rows": torch.zeros((1, S), dtype=torch.int64, device=mgr.device)})
    for lo, hi in ((0, S + 1), (3, 2)):
        with pytest.raises(RuntimeError, match=r"status -4"):
            win.batch(lo, hi)
        with pytest.raises(RuntimeError, match=r"status -4"):
            win.gather([torch.zeros((S, 1), device=mgr.device)], lo, hi)
    assert tuple(win.batch(2, 2)["rows"].shape) == (1, 0)                   # an empty range is fine
    out = {"len": torch.zeros(S, dtype=torch.int32, device=mgr.device)}
    assert win.batch(out=out) is out and (np_(out["len"]) == 1).all()
    # a push invalidates the sequences
    mgr.write_actions(tu.breed_shoot(mgr.num_agents(), 0).to(mgr.device))
    mgr.step()
    win.push()
    for call in (win.batch, win.sequences, lambda: win.view(win.SEQ_ID, 0)):
        with pytest.raises(RuntimeError, match=r"status -1"):
            call()
    # a truncated table: recorded truncated, refused from compute on
    for t in (1, 2):
        mgr.write_actions(tu.breed_shoot(mgr.num_agents(), t).to(mgr.device))
        mgr.step()
        win.push()
    assert mgr.num_agents() > 33
    with pytest.raises(RuntimeError, match=r"status -4"):
        win.compute(0.9)
    for call in (win.sequences, win.batch):
        with pytest.raises(RuntimeError, match=r"status -1"):
            call()
    win.close()
    # the same with the records on: three tables of 34 rows and more into slots
    # of 33, the last in the ring's last slot (a row too many would leave the
    # record, state and mask arrays); refused from compute on, and once they
    # have left, the window records and batches as ever
    win = mgr.trajectory_window(3, 33, **ALL)
    for _ in range(3):
        win.push()
    with pytest.raises(RuntimeError, match=r"status -4"):
        win.compute(0.9)
    for call in (win.sequences, win.batch):
        with pytest.raises(RuntimeError, match=r"status -1"):
            call()
    mgr.load_checkpoint(blob)                                               # (32 rows again; empties the window)
    assert win.num_tables == 0
    rec = Recorder()
    write_memory(mgr, 98)
    tu.run_window(mgr, steps=2, with_values=True, win=win, before_step=write_memory, after_push=rec)
    after, idx, res = check_batches(win, rec, "after truncation", splits=((0, 7), (7, None)))
    assert max(res["rows"]) == 33 and after["hidden0"].any()
    win.close()
    # a flagless window refuses, and computes the bits of a second manager's
    m1, m2 = make(tu.W, tu.A), make(tu.W, tu.A)
    w1 = tu.run_window(m1, with_values=True)
    w2 = m2.trajectory_window(tu.STEPS + 1, 4096, **ALL)
    tu.run_window(m2, with_values=True, win=w2)
    r1, r2 = tu.to_numpy(w1.compute(*PARAMS)), tu.to_numpy(w2.compute(*PARAMS))
    tu.assert_same(r1, r2, where="flagless")
    tu.check_against_restatement(r1, [np.zeros(tu.W, np.int32)] * len(r1["rows"]), *PARAMS)
    assert w1.flags == 0
    with pytest.raises(RuntimeError, match=r"status -1"):
        w1.sequences()
    with pytest.raises(RuntimeError, match=r"status -1"):
        w1.view(w1.SEQ_ID, 0)
    with pytest.raises(RuntimeError, match=r"status -1"):
        w1.batch()
    return {"flagless": r1, "after truncation": after}


def shards_scenario(make):
    """Test 9: worlds 0-1 with the shard ghost and worlds 2-3 without against
    one manager, on the identity-keyed synthetic stream."""
    pre = 10
    mgrs = [make(tu.W, tu.A), make(2, tu.A, shard_ghost=True), make(2, tu.A, world_offset=2)]
    outs = []
    for m in mgrs:
        for t in range(pre):
            m.write_synthetic_actions(1234, t, False)
            m.step()
        win = m.trajectory_window(10, 4096, **ALL)
        rec = Recorder()
        tu.run_window(m, with_values=False, win=win, actions=None, t0=pre, after_push=rec)
        whole, idx, res = check_batches(win, rec, "shard", splits=((0, 7), (7, None)))
        world = np.array([res["world"][t][q] for t, q in zip(idx["t0"], idx["rows"][0])])
        outs.append((whole, res, world))
    assert mgrs[1].num_rows() > mgrs[1].num_agents()                       # the ghost has rows of its own
    (one, r1, w1), (a, ra, wa), (b, rb, wb) = outs
    for t in range(10):                                                     # ... which lie in no sequence
        assert r1["rows"][t] == ra["rows"][t] + rb["rows"][t]
    assert int(a["len"].sum()) == sum(ra["rows"]) and set(wa) == {0, 1} and set(wb) == {2, 3}
    for w in range(tu.W):
        part, pw = (a, wa) if w < 2 else (b, wb)
        got = sorted(zip(part["t0"][pw == w], part["len"][pw == w], part["end"][pw == w]))
        exp = sorted(zip(one["t0"][w1 == w], one["len"][w1 == w], one["end"][w1 == w]))
        assert got == exp and len(got) >= tu.A, w
    return one


def same_tree(a, b, where=""):
    """Two bodies' outcomes (nested dicts / lists of arrays) bitwise equal."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), where
        for k in a:
            same_tree(a[k], b[k], (where, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_tree(x, y, (where, i))
    elif isinstance(a, np.ndarray):
        same(a, b, where)
    else:
        assert a == b, where
