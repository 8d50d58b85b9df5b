"""The oracle-side reference of the window sequences
(tests/test_window_sequences.py): what a trajectory window and the rasteriser
must hold, recorded from the oracle (oracle/pyoracle.py) alone.  Nothing here
reads the product: link comes from stamps the test writes into HiddenState on
both sides, world from the oracle's species counts, reward from its Reward
column, the reset marks from its flags and episodes, the sweeps from
traj_util.restate on those arrays, the images from render_ref.render_ref on
the oracle's world_state()."""
import numpy as np
import torch

import pyoracle
import render_ref
import traj_util as tu


def stamp(mgr, orc):
    """row + 1 into column 0 of the current HiddenState of both sides: the step
    carries HiddenState with its agent through the species sort and gives a
    newborn, a respawn and every agent of a re-initialised world zeros, so after
    the step the oracle's column 0, minus 1, is each row's previous row or -1.
    (float32 holds every row index below 2^24 exactly.)"""
    o = orc.column(pyoracle.COL_HIDDEN)
    n = len(o)
    assert n < 1 << 24
    o[:, 0] = np.arange(1, n + 1, dtype=np.float32)
    h = mgr.hidden_state_tensor(False).to_torch()
    assert h.shape[0] == n, (h.shape, n)
    h[:, 0] = torch.arange(1, n + 1, dtype=torch.float32, device=h.device)


def oracle_worlds(orc, world_offset=0):
    """Each row's global world from the oracle's species counts: the table is
    species-major, world-major within a species."""
    c = orc.species_count()
    return (np.repeat(np.tile(np.arange(c.shape[0], dtype=np.int32), 4), c.T.reshape(-1)) +
            np.int32(world_offset)).astype(np.int32)


def oracle_images(orc, worlds, scale, pal):
    """render_ref of the oracle's worlds as they stand now, stacked like
    render_worlds' outputs."""
    outs = []
    for w in worlds:
        st = orc.world_state(int(w))
        outs.append(render_ref.render_ref(dict(st, position=st["xy"], rotation_wz=st["rot"]), scale, pal))
    return {"cls": np.stack([o[0] for o in outs]), "slot": np.stack([o[1] for o in outs]),
            "rgb": np.stack([o[2] for o in outs])}


class WindowRecorder:
    """The tables a window holds, from the oracle.  restart() when the window
    was emptied or opened, before_step() right before the oracle steps (after
    the stamps), table(t) at every push; keep_last() follows
    clear(keep_last=True).  The caller hands values(t) to the product's push."""

    def __init__(self, orc, seed, world_offset=0):
        self.orc, self.seed, self.world_offset = orc, seed, world_offset
        self.tables = []
        self._flags = self._episode = None

    def restart(self):
        self.tables = []
        self._flags = self._episode = None

    def keep_last(self):
        self.tables = self.tables[-1:]

    def __len__(self):
        return len(self.tables)

    def before_step(self):
        self._flags = self.orc.reset_flags().copy()
        self._episode = self.orc.episode().copy()

    def values(self, t):
        """The critic's estimates of the table now on the oracle."""
        return tu.values_for(self.orc.num_agents(), t, self.seed)

    def table(self, t, stepped):
        """Record the oracle's current table.  stepped: it is the product of a
        step taken since before_step() (else the first table of a window, whose
        link and marks nobody follows)."""
        orc = self.orc
        n = orc.num_agents()
        W = orc.num_worlds
        if stepped:
            link = orc.column(pyoracle.COL_HIDDEN)[:, 0].astype(np.int32) - 1
            # the step re-initialised a world iff its episode changed or it held
            # a flag (a flag may name the episode the world is already in)
            mark = ((orc.episode() != self._episode) | (self._flags != 0)).astype(np.int32)
        else:
            link = np.full(n, -1, np.int32)
            mark = np.zeros(W, np.int32)
        self.tables.append({"rows": n, "link": link, "mark": mark,
                            "world": oracle_worlds(orc, self.world_offset),
                            "reward": orc.column(pyoracle.COL_REWARD).reshape(-1).copy(),
                            "value": self.values(t).numpy().copy()})

    def reference(self, gamma, lam, death_reward):
        """What compute() must return (tu.to_numpy's layout; link[0] is not to
        be compared), plus "marks"."""
        tb = self.tables
        ref = {"rows": [x["rows"] for x in tb], "marks": [x["mark"] for x in tb]}
        for k in ("link", "world", "reward", "value"):
            ref[k] = [x[k] for x in tb]
        ref["next"], ref["end"], ref["adv"], ref["ret"] = tu.restate(
            ref["link"], ref["reward"], ref["value"], ref["world"], ref["marks"], gamma, lam, death_reward,
            self.world_offset)
        return ref


def facts(ref, world_offset=0):
    """Of a reference: rows with end 0 / 1 / 2 and the links of -1 outside the
    worlds their step re-initialised (births and respawns)."""
    end = np.concatenate(ref["end"])
    births = 0
    for t in range(1, len(ref["rows"])):
        births += int(((ref["link"][t] < 0) & (ref["marks"][t][ref["world"][t] - world_offset] == 0)).sum())
    return {"alive": int((end == 0).sum()), "deaths": int((end == 1).sum()),
            "reset_cuts": int((end == 2).sum()), "births": births}


def check_window(win, out, ref, where):
    """A compute() result against the reference, bitwise: rows, the pushed
    columns (link from table 1 on), the derived ones, and lifelines(0) / (2)."""
    res = tu.to_numpy(out)
    n = len(ref["rows"])
    assert res["rows"] == ref["rows"], (where, res["rows"], ref["rows"])
    for k in tu.KEYS:
        lo = 1 if k == "link" else 0
        assert len(res[k]) == len(ref[k]) == (n - 1 if k == "next" else n), (where, k)
        for t in range(lo, len(ref[k])):
            x, y = res[k][t], np.asarray(ref[k][t])
            assert x.dtype == y.dtype and x.shape == y.shape, (where, k, t, x.dtype, y.dtype, x.shape, y.shape)
            if not np.array_equal(tu.bits(x), tu.bits(y)):
                bad = np.nonzero(tu.bits(x) != tu.bits(y))[0]
                raise AssertionError(f"{where}: {k}[{t}] differs in {len(bad)} of {len(x)} rows; first row "
                                     f"{bad[0]}: window {x[bad[0]]!r} reference {y[bad[0]]!r}")
    for t0 in (0, 2):
        if t0 < n:
            life = win.lifelines(t0).cpu().numpy()
            assert np.array_equal(life, tu.lifelines_ref(ref["next"], ref["rows"], t0)), (where, "lifelines", t0)
