"""Lock-step of the CPU oracle (oracle/mbots_oracle.c) with the reference's own
simulation code on the stand-in engine (oracle/refbuild/, oracle/pyref.py).

The stand-in's render system traces nothing, so before each step the oracle's
finder slots go into it, and after each step the oracle's new sensor rows: the
sensor stays out of scope here (tests/test_sensor_scenes.py holds it to float64
geometry).  Everything else is compared bitwise after every step and shift:
every exported column, current and Prev -- the Prev sensor bytes are the
reference's own updateSensorOutputIdx copy -- the species counts, the world
offsets and counts, the sensor index, each world's agents in slot order and its
food list.

The reference writes SpeciesCount before it respawns (quirk B.5); the oracle
exports the count after.  speciesInfoSync respawns species i up to
initNumAgentsPerWorld / 4, so the oracle's count must be max(raw, A // 4), and
that is what is asserted -- it pins the respawn count itself.
"""
import numpy as np

import pyoracle as po
from golden_util import STREAMS, breed_heavy, shoot_heavy  # noqa: F401  (the cases' action streams)

NAMES = ["species", "pos", "health", "surround", "reward", "action", "stats", "hidden",
         "semantic", "depth"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint8)


class Mismatch(AssertionError):
    pass


class LockStep:
    def __init__(self, W, seed, A, cap=512, orc=None):
        import pyref
        self.W, self.A = W, A
        self.orc = orc if orc is not None else po.OracleSim(W, seed, A, cap=cap)
        self.ref = pyref.RefSim(W, seed, A)
        self.t = 0
        self.stepped = False
        # what the run went through (for the cases' own assertions)
        self.deaths = self.respawns = self.births = self.friendly = self.enemy = self.ate = 0
        self.peak_food = 0
        self.peak_world = 0
        self.compare("init")

    # -- inputs ---------------------------------------------------------------
    def write_actions(self, actions=None, hidden=None):
        """The same current Action (and HiddenState) rows on both sides; None
        copies what the oracle's table holds (write_synthetic_actions)."""
        if actions is not None:
            self.orc.column(po.COL_ACTION)[:] = np.asarray(actions, np.int32).reshape(-1, 6)
        if hidden is not None:
            self.orc.column(po.COL_HIDDEN)[:] = np.asarray(hidden, np.float32).reshape(-1, po.HIDDEN)
        self.ref.write_column(po.COL_ACTION, self.orc.column(po.COL_ACTION))
        self.ref.write_column(po.COL_HIDDEN, self.orc.column(po.COL_HIDDEN))

    def synthetic(self, seed, write_hidden=True):
        self.orc.write_synthetic_actions(seed, self.t, write_hidden)
        self.write_actions()

    def set_world_state(self, w, pos, rot, food):
        self.orc.set_world_state(w, pos, rot, food)
        self.ref.set_world_state(w, pos, rot, food)

    # -- the two calls --------------------------------------------------------
    def step(self, check=True):
        orc, ref = self.orc, self.ref
        for w in range(self.W):
            ref.set_finder(w, orc.world_state(w)["finder"])
        n0 = orc.num_agents()
        self.stepped = True
        orc.step()
        ref.step()
        ref.sensor()
        if ref.num_agents() == orc.num_agents():
            ref.write_column(po.COL_SEMANTIC, orc.column(po.COL_SEMANTIC))
            ref.write_column(po.COL_DEPTH, orc.column(po.COL_DEPTH))
        if check:
            self.compare(f"step {self.t}")
        assert orc.overflow() == 0, "the oracle's cap binds: the reference has none"
        st = orc.column(po.COL_STATS)
        raw = ref.species_count()
        resp = int(np.maximum(self.A // 4 - raw, 0).sum())
        births = int(st[:, 3].sum())
        self.births += births
        self.respawns += resp
        self.deaths += n0 + births + resp - orc.num_agents()
        self.friendly += int(st[:, 0].sum())
        self.enemy += int(st[:, 1].sum())
        self.ate += int(st[:, 2].sum())
        self.peak_world = max(self.peak_world, int(orc.world_counts()[0].max()))
        self.peak_food = max(self.peak_food, max(len(orc.world_state(w)["food"]) for w in range(self.W)))
        self.t += 1

    def shift(self, check=True):
        self.orc.shift_observations()
        self.ref.shift_observations()
        if check:
            self.compare(f"shift {self.t - 1}")

    # -- comparison -----------------------------------------------------------
    def _world_of_row(self):
        c, o = self.orc.world_counts()
        si = self.orc.sensor_index()
        m = np.full(self.orc.num_agents(), -1, np.int64)
        for w in range(self.W):
            m[si[o[w]:o[w] + c[w]]] = w
        return m

    def compare(self, where, counts=True):
        orc, ref = self.orc, self.ref
        if ref.num_agents() != orc.num_agents():
            raise Mismatch(f"{where}: {ref.num_agents()} reference rows, {orc.num_agents()} oracle rows")
        for is_prev in (False, True):
            for i, nm in enumerate(NAMES):
                r, o = ref.column(i, is_prev), orc.column(i, is_prev)
                bad = np.nonzero((bits(r) != bits(o)).reshape(len(r), -1).any(axis=1))[0]
                if len(bad):
                    k = int(bad[0])
                    raise Mismatch(f"{where}: column {'prev_' if is_prev else ''}{nm} row {k} world "
                                   f"{int(self._world_of_row()[k])}: reference {r[k]} oracle {o[k]} "
                                   f"({len(bad)} rows differ)")
        if counts and self.stepped:   # (SpeciesCount is first written by a step)
            raw = ref.species_count()
            want = np.maximum(raw, self.A // 4)
            if not np.array_equal(want, orc.species_count()):
                raise Mismatch(f"{where}: species_count: reference before respawns {raw.tolist()}, so "
                               f"{want.tolist()} after; oracle {orc.species_count().tolist()}")
        if counts:
            if ref.bridge_total() != orc.num_agents():
                raise Mismatch(f"{where}: SimBridge.totalNumAgents {ref.bridge_total()} oracle {orc.num_agents()}")
        rc, ro = ref.world_counts()
        oc, oo = orc.world_counts()
        if not (np.array_equal(rc, oc) and np.array_equal(ro, oo)):
            raise Mismatch(f"{where}: world counts / offsets: reference {rc.tolist()} {ro.tolist()} "
                           f"oracle {oc.tolist()} {oo.tolist()}")
        if counts and not np.array_equal(ref.sensor_index(), orc.sensor_index()):
            bad = int(np.nonzero(ref.sensor_index() != orc.sensor_index())[0][0])
            raise Mismatch(f"{where}: sensor_index differs first at agent {bad}")
        for w in range(self.W):
            a, b = ref.world_state(w), orc.world_state(w)
            for k in ("xy", "rot", "species", "health", "food"):
                if a[k].shape != b[k].shape or not np.array_equal(bits(a[k]), bits(b[k])):
                    raise Mismatch(f"{where}: world {w} {k}: reference {a[k].tolist()} oracle {b[k].tolist()}")
            if a["cur_food"] != len(b["food"]):
                raise Mismatch(f"{where}: world {w}: currentNumFood {a['cur_food']} but {len(b['food'])} packages")
