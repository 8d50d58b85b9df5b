"""Helpers of the trajectory-window tests (test_traj_*.py): the action stream,
a recorder that runs a manager through a window, and the numpy restatement of
include/mbots.h "Trajectory window" the sweeps are held against."""
import ctypes

import numpy as np
import pytest
import torch

W, A = 4, 8          # worlds, init_num_agents_per_world
SEED = 15            # rand_seed and action-stream seed of the shared scenario
STEPS = 9            # 10 tables: the initial one and one per step
KEYS = ("link", "world", "reward", "value", "next", "end", "adv", "ret")


def cpu(num_worlds=W, **kw):
    import madrona_bots as mb
    kw.setdefault("agent_capacity", 128)
    return mb.SimManager(0, num_worlds, SEED, A, exec_mode="cpu", **kw)


def hip(num_worlds=W, **kw):
    import madrona_bots as mb
    kw.setdefault("agent_capacity", 128)
    return mb.SimManager(0, num_worlds, SEED, A, **kw)


def breed_shoot(n, t, seed=SEED):
    """Breed- and shoot-heavy: shoot 3/8, breed 3/8, forward 1/8, rotate 1/8,
    by a draw seeded per step (a function of the row index and the step)."""
    g = torch.Generator().manual_seed(seed * 1000 + t)
    r = torch.randint(0, 8, (n,), generator=g)
    a = torch.zeros((n, 6), dtype=torch.int32)
    a[r < 3, 4] = 1
    a[(r >= 3) & (r < 6), 5] = 1
    a[r == 6, 0] = 1
    a[r == 7, 2] = 1
    return a


def breed_turning(n, t):
    """tests/test_grow_capacity.py::_breed_turning as an action array: every
    agent breeds, and walks or turns by a seeded draw."""
    r = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(500 + t))
    a = torch.zeros((n, 6), dtype=torch.int32)
    a[:, 5] = 1
    a[r == 0, 0] = 1
    a[r == 1, 2] = 1
    a[r == 2, 3] = 1
    return a


def values_for(n, t, seed=SEED):
    """The caller's critic estimates of table t: seeded random f32."""
    g = torch.Generator().manual_seed(seed * 7919 + 31 * t + 5)
    return torch.randn((n,), generator=g, dtype=torch.float32)


def run_window(mgr, steps=STEPS, horizon=None, with_values=False, before_step=None, after_push=None,
               win=None, first_table=True, t0=0, actions=breed_shoot, max_rows=4096):
    """Open a window on `mgr` (or go on with `win`), push the current table
    (first_table; after_push(mgr, t) follows every push) and then `steps` steps'
    tables: actions written (actions None: the identity-keyed synthetic
    stream), before_step(mgr, t) called, step, push.  Returns the window."""
    if win is None:
        win = mgr.trajectory_window(horizon or steps + 1, max_rows)

    def push(t):
        n = mgr.num_agents()
        win.push(values_for(n, t).to(mgr.device) if with_values else None)
        if after_push:
            after_push(mgr, t)

    if first_table:
        push(t0)
    for k in range(steps):
        t = t0 + k
        n = mgr.num_agents()
        if actions is not None:
            mgr.write_actions(actions(n, t).to(mgr.device))
        else:
            mgr.write_synthetic_actions(1234, t, False)
        if before_step:
            before_step(mgr, t)
        mgr.step()
        push(t + 1)
    return win


def to_numpy(res):
    """compute()'s dict as numpy arrays (copies), rows flattened."""
    out = {"rows": list(res["rows"])}
    for k in KEYS:
        out[k] = [x.detach().cpu().numpy().reshape(-1).copy() for x in res[k]]
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(a, b, keys=KEYS, where=""):
    """Two results (to_numpy) bitwise equal."""
    assert a["rows"] == b["rows"], (where, a["rows"], b["rows"])
    for k in keys:
        assert len(a[k]) == len(b[k]), (where, k)
        for t, (x, y) in enumerate(zip(a[k], b[k])):
            assert x.dtype == y.dtype and x.shape == y.shape, (where, k, t)
            assert np.array_equal(bits(x), bits(y)), (where, k, t)


def restate(link, reward, value, world, marks, gamma, lam, death_reward, world_offset=0):
    """The header's formulas in numpy float32, t from the back; every product
    and every sum its own np.float32 operation.  marks[t][w] != 0: the step that
    produced table t re-initialised local world w.  Returns next, end, adv, ret."""
    n = len(link)
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    dr = np.float32(death_reward)
    nxt = []
    for t in range(n - 1):
        m = np.full(len(link[t]), -1, np.int32)
        src = link[t + 1]
        ok = (src >= 0) & (src < len(link[t]))
        m[src[ok]] = np.nonzero(ok)[0].astype(np.int32)
        nxt.append(m)
    end = [None] * n
    adv = [None] * n
    ret = [None] * n
    for t in range(n - 1, -1, -1):
        v = value[t].astype(np.float32)
        if t == n - 1:
            end[t] = np.full(len(v), 3, np.int32)
            adv[t] = np.zeros(len(v), np.float32)
            ret[t] = v.copy()
            continue
        r = nxt[t]
        has = r >= 0
        wl = world[t] - world_offset
        reset = np.asarray(marks[t + 1])[wl] != 0
        end[t] = np.where(has, 0, np.where(reset, 2, 1)).astype(np.int32)
        a = np.zeros(len(v), np.float32)
        rs = r[has]
        prod = (g * value[t + 1][rs]).astype(np.float32)
        tot = (reward[t + 1][rs] + prod).astype(np.float32)
        delta = (tot - v[has]).astype(np.float32)
        if t + 1 <= n - 2:
            delta = (delta + (gl * adv[t + 1][rs]).astype(np.float32)).astype(np.float32)
        a[has] = delta
        died = end[t] == 1
        a[died] = (dr - v[died]).astype(np.float32)
        adv[t] = a
        ret[t] = (a + v).astype(np.float32)
    return nxt, end, adv, ret


def lifelines_ref(nxt, rows, t0=0):
    n = len(rows)
    cur = np.arange(rows[t0], dtype=np.int64)
    out = [cur]
    for t in range(t0, n - 1):
        step = np.full_like(cur, -1)
        alive = cur >= 0
        step[alive] = nxt[t][cur[alive]]
        cur = step
        out.append(cur)
    return np.stack(out)


def scenario_facts(res, marks=None, world_offset=0):
    """(births, deaths, survivors) of a window: births counts the rows of tables
    >= 1 without a predecessor (outside the worlds `marks` says their step
    re-initialised), deaths the end == 1 rows, survivors the lifelines of table 0
    that reach the last table."""
    births = 0
    for t in range(1, len(res["link"])):
        new = res["link"][t] < 0
        if marks is not None:
            new &= np.asarray(marks[t])[res["world"][t] - world_offset] == 0
        births += int(new.sum())
    deaths = sum(int((x == 1).sum()) for x in res["end"])
    life = lifelines_ref(res["next"], res["rows"])
    survivors = int((life[-1] >= 0).sum())
    return births, deaths, survivors


class Episodes:
    """after_push hook: each table's per-world episodes, from which the tests
    derive the reset marks without asking the window (marks[t][w]: the episode
    of world w changed in the step that produced table t)."""

    def __init__(self):
        self.tables = []

    def __call__(self, mgr, t):
        self.tables.append(mgr.episode_tensor().to_torch().cpu().numpy().reshape(-1).copy())

    def marks(self):
        e = self.tables
        return [np.zeros_like(e[0])] + [(e[t] != e[t - 1]).astype(np.int32) for t in range(1, len(e))]


def check_against_restatement(res, marks, gamma, lam, death_reward, world_offset=0, where=""):
    """next, end, adv, ret of a result (to_numpy) bitwise equal to restate()."""
    nxt, end, adv, ret = restate(res["link"], res["reward"], res["value"], res["world"], marks, gamma, lam,
                                 death_reward, world_offset)
    ref = dict(res, next=nxt, end=end, adv=adv, ret=ret)
    assert_same(res, ref, ("next", "end", "adv", "ret"), where)


def assert_scenario(res, marks=None, world_offset=0):
    """At least one birth, one death and one agent alive from the first table
    to the last: the window cannot pass vacuously."""
    births, deaths, survivors = scenario_facts(res, marks, world_offset)
    assert births >= 1 and deaths >= 1 and survivors >= 1, (births, deaths, survivors)


# ---- the scenarios both execution modes run (factory: cpu or hip) ----------
PARAMS = ((1.0, 1.0, 0.0), (0.99, 0.95, -1.0))
RESET_STEP, RESET_WORLD, OTHER_WORLD = 5, 1, 3   # in the plain run, step 5 kills an agent of
                                                 # world 1 and one of world 3
EPISODE_LENGTH = 4


def scenario_plain(make, with_values, **kw):
    mgr = make()
    return mgr, run_window(mgr, with_values=with_values, **kw)


def scenario_reset(make, mode, with_values=True):
    """mode "flag": reset_worlds([RESET_WORLD]) before step RESET_STEP; "length":
    set_episode_length(EPISODE_LENGTH) from the start.  Returns mgr, win, marks."""
    mgr = make()
    ep = Episodes()
    if mode == "length":
        mgr.set_episode_length(EPISODE_LENGTH)

    def before(m, t):
        if mode == "flag" and t == RESET_STEP:
            m.reset_worlds([RESET_WORLD])
    win = run_window(mgr, with_values=with_values, before_step=before, after_push=ep)
    return mgr, win, ep.marks()


GROW_PRE, GROW_STEPS = 20, 8   # the all-breeding stream's largest world holds 56 agents after 20
                               # steps; 2 n + A passes 128 before step 23


def scenario_growth(make, capacity):
    """GROW_PRE steps of the all-breeding stream, then a window over GROW_STEPS
    steps -- four more of that stream, during which an agent_capacity="auto"
    manager grows 128 -> 256, then the breed- and shoot-heavy one."""
    mgr = make(agent_capacity=capacity)
    for t in range(GROW_PRE):
        mgr.write_actions(breed_turning(mgr.num_agents(), t).to(mgr.device))
        mgr.step()
    cap0 = mgr.agent_capacity
    win = run_window(mgr, steps=GROW_STEPS, with_values=True, t0=GROW_PRE,
                     actions=lambda n, t: (breed_turning if t < GROW_PRE + 4 else breed_shoot)(n, t))
    return mgr, win, cap0


# ---- bodies both execution modes run (make: cpu or hip) --------------------
def chained_windows_keep_every_transition(make):
    """Two windows of 6 tables chained by clear(keep_last=True) hold the
    transitions of one window of 11; with lambda 0 the advantages of those
    transitions are the same bits too (no bootstrapping across the cut)."""
    params = (0.99, 0.0, -1.0)
    mgr, big = scenario_plain(make, True, steps=10)
    whole = to_numpy(big.compute(*params))
    assert_scenario(whole)
    m2 = make()
    win = run_window(m2, steps=5, horizon=6, with_values=True)
    first = to_numpy(win.compute(*params))
    with pytest.raises(RuntimeError, match=r"status -1"):
        win.push()                                            # full
    win.clear(keep_last=True)
    assert win.num_tables == 1
    run_window(m2, steps=5, with_values=True, win=win, first_table=False, t0=5)
    second = to_numpy(win.compute(*params))
    for part, off in ((first, 0), (second, 5)):
        assert part["rows"] == whole["rows"][off:off + 6]
        for t in range(6):
            for k in ("world", "reward", "value"):
                assert np.array_equal(bits(part[k][t]), bits(whole[k][off + t])), (k, off, t)
        for t in range(1, 6):
            assert np.array_equal(part["link"][t], whole["link"][off + t])
        for t in range(5):
            for k in ("next", "end", "adv", "ret"):
                assert np.array_equal(bits(part[k][t]), bits(whole[k][off + t])), (k, off, t)


def compute_twice_gives_the_same_bits(win, expected):
    """A compute with the first parameter set, then one with the second on the
    same pushed tables: `expected`, that window's result at the second set."""
    win.compute(*PARAMS[0])
    again = to_numpy(win.compute(*PARAMS[1]))
    assert_same(again, expected)
    return again


def _gather(parts, counts):
    """harness/gather.py's reassembly: species-major, per species rank-major.
    parts[k]: rank k's rows, counts[k]: its rows per species."""
    out = []
    for s in range(4):
        for x, c in zip(parts, counts):
            lo = int(sum(c[:s]))
            out.append(x[lo:lo + int(c[s])])
    return np.concatenate(out)


def two_shards_equal_one_manager(make):
    """Worlds 0-1 with the shard ghost and worlds 2-3 without, in one process,
    on the identity-keyed synthetic stream (10 steps in, where the stream's
    window holds births and deaths); value: each row's x position, an
    identity-carried quantity every manager can hand over."""
    pre = 10
    mgrs = [make(), make(2, shard_ghost=True), make(2, world_offset=2)]
    wins, counts = [], [[], [], []]
    for i, m in enumerate(mgrs):
        for t in range(pre):
            m.write_synthetic_actions(1234, t, False)
            m.step()
        win = m.trajectory_window(10, 4096)

        def push(m=m, win=win, i=i):
            win.push(m.position_tensor(False).to_torch()[:, 0].contiguous())
            counts[i].append(m.species_count_tensor().to_torch().cpu().numpy().sum(0))
        push()
        for t in range(pre, pre + 9):
            m.write_synthetic_actions(1234, t, False)
            m.step()
            push()
        wins.append(win)
    one, a, b = (to_numpy(w.compute(*PARAMS[1])) for w in wins)
    assert_scenario(one)
    for t in range(10):
        assert one["rows"][t] == a["rows"][t] + b["rows"][t]
        assert a["rows"][t] == mgrs[1].num_agents() or t < 9      # the ghost's rows are not recorded
        for k in ("world", "end", "adv", "ret"):
            got = _gather([a[k][t], b[k][t]], [counts[1][t], counts[2][t]])
            assert np.array_equal(bits(got), bits(one[k][t])), (k, t)
        if t:
            for part in (a, b):
                assert (part["link"][t] < part["rows"][t - 1]).all(), t
    assert mgrs[1].num_rows() > mgrs[1].num_agents()              # the ghost has rows of its own
    # world is global: the second shard's rows name worlds 2 and 3 only
    assert all(set(np.unique(x)) <= {0, 1} for x in a["world"])
    assert all(set(np.unique(x)) == {2, 3} for x in b["world"])


def errors_and_emptying(make):
    import madrona_bots as mb
    mgr = make()
    with pytest.raises(RuntimeError, match=r"status -1"):
        mgr.trajectory_window(1, 64)
    win = mgr.trajectory_window(4, 33)
    with pytest.raises(RuntimeError):
        mgr.trajectory_window(4, 64)                               # one per manager
    with pytest.raises(RuntimeError, match=r"status -1"):
        win.compute(0.9)                                           # empty
    with pytest.raises(ValueError):
        win.push(torch.zeros(3))                                   # fewer values than rows
    win.push()
    blob = mgr.save_checkpoint()
    rows = [mgr.num_agents()]
    for t in range(3):
        mgr.write_actions(breed_shoot(mgr.num_agents(), t).to(mgr.device))
        mgr.step()
        win.push()
        rows.append(mgr.num_agents())
    assert rows[-1] == 34 and max(rows[:3]) == 33                  # the last table is one row too many
    with pytest.raises(RuntimeError, match=r"status -1"):
        win.push()                                                 # full
    for _ in range(2):                                             # ... and stays unusable
        with pytest.raises(RuntimeError, match=r"status -4"):
            win.compute(0.9)
    with pytest.raises(RuntimeError):
        win.view(win.END, 0)
    win.clear()
    assert win.num_tables == 0
    mgr.load_checkpoint(blob)                                      # back to 32 rows
    win.push()
    mgr.write_actions(breed_shoot(mgr.num_agents(), 0).to(mgr.device))
    mgr.step()
    win.push()
    res = to_numpy(win.compute(0.9))
    assert res["rows"] == rows[:2]
    check_against_restatement(res, [np.zeros(W, np.int32)] * 2, 0.9, 1.0, 0.0)
    # a load and a set_world_state empty the window
    mgr.load_checkpoint(blob)
    assert win.num_tables == 0
    win.push()
    ws = mgr.world_state(0)
    mgr.set_world_state(0, ws["position"], ws["rotation_wz"], ws["food"])
    assert win.num_tables == 0
    win.push()
    win.compute(0.9)
    with pytest.raises(RuntimeError, match=r"status -4"):
        win.view(win.LINK, 1)                                      # table 1 is outside the window
    # views after close are refused, by the object and by the library
    h = mgr._h
    win.close()
    with pytest.raises(RuntimeError, match="closed"):
        win.view(win.LINK, 0)
    ct = mb._CTensor()
    assert mb._lib.mbots_traj_view(h, 0, 0, ctypes.byref(ct)) == -1
    assert mb._lib.mbots_traj_push(h, None, None) == -1
    mgr.trajectory_window(4, 64).close()                           # and a new one can be opened
    truncated_table_leaves_its_neighbour(mgr, blob, rows)


def truncated_table_leaves_its_neighbour(mgr, blob, rows):
    """The same run (blob: its first table; rows: 32, .., 33, 34) through a
    ring of 3 slots of 33 rows.  Tables 0 to 2 fill slots 0 to 2; after
    clear(keep_last) the 34-row table goes into slot 0, whose row 33 would be
    row 0 of slot 1.  Slot 1's pushed columns (still table 1's) must hold what
    they held, compute must refuse with status -4 until the table has left the
    window, and the window works again afterwards."""
    mgr.load_checkpoint(blob)
    win = mgr.trajectory_window(3, 33)
    win.push(values_for(rows[0], 0).to(mgr.device))
    for t in range(2):
        mgr.write_actions(breed_shoot(mgr.num_agents(), t).to(mgr.device))
        mgr.step()
        win.push(values_for(rows[t + 1], t + 1).to(mgr.device))
    win.compute(0.9)
    keys = (("link", win.LINK), ("world", win.WORLD), ("reward", win.REWARD), ("value", win.VALUE))
    slot1 = {k: win.view(what, 1) for k, what in keys}             # views of slot 1's storage
    held = {k: v.detach().cpu().numpy().copy() for k, v in slot1.items()}
    assert all(len(v) == rows[1] for v in held.values())
    assert held["value"].any() and held["reward"].any() and (held["link"] != 0).any()
    win.clear(keep_last=True)
    mgr.write_actions(breed_shoot(mgr.num_agents(), 2).to(mgr.device))
    mgr.step()
    assert mgr.num_agents() == rows[3] == 34
    v = torch.full((34,), 7.5)                                     # (no stored value or reward is 7.5)
    win.push(v.to(mgr.device))
    assert win.num_tables == 2
    for _ in range(2):
        with pytest.raises(RuntimeError, match=r"status -4"):
            win.compute(0.9)
    if mgr.device.type != "cpu":
        torch.cuda.synchronize()
    for k, v in slot1.items():
        assert np.array_equal(bits(v.detach().cpu().numpy()), bits(held[k])), k
    win.clear(keep_last=True)                                      # the truncated table is table 0 now
    with pytest.raises(RuntimeError, match=r"status -4"):
        win.compute(0.9)
    win.clear()                                                    # ... and now it has left
    mgr.load_checkpoint(blob)
    win.push()
    res = to_numpy(win.compute(0.9))
    assert res["rows"] == [rows[0]] and (res["end"][0] == 3).all()
    win.close()
