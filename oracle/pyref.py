"""TEST INFRASTRUCTURE ONLY: ctypes view of oracle/_ref/libmbots_ref.so.

That library is the reference's own simulation translation unit compiled
against the stand-in engine of oracle/refbuild/ (`make -C oracle ref`); it is
built only where the reference's source lies on the machine and is never
committed.  RefSim mirrors pyoracle.OracleSim's method names where the two
overlap, so that tests/ref_lockstep.py can run both in lock-step.  The product
package never imports this module, and nothing that runs on a device does.
"""
import ctypes
import os

import numpy as np

from pyoracle import _COL_SPEC, COL_ACTION, COL_DEPTH, COL_HIDDEN, COL_SEMANTIC  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libmbots_ref.so")
_LIB = None


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _LIB
    if _LIB is None:
        L = ctypes.CDLL(LIB_PATH)
        vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int32
        L.ref_create.restype = vp
        L.ref_create.argtypes = [u32, u32, u32, u32]
        L.ref_destroy.argtypes = [vp]
        for fn in (L.ref_step, L.ref_sensor, L.ref_shift_observations):
            fn.argtypes = [vp]
            fn.restype = None
        for fn in (L.ref_num_agents, L.ref_bridge_total):
            fn.restype = u32
            fn.argtypes = [vp]
        L.ref_read_column.restype = ctypes.c_int
        L.ref_read_column.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        L.ref_write_column.restype = ctypes.c_int
        L.ref_write_column.argtypes = [vp, ctypes.c_int, vp, u32]
        L.ref_species_count.argtypes = [vp, vp]
        L.ref_world_counts.argtypes = [vp, vp, vp]
        L.ref_sensor_index.argtypes = [vp, vp]
        L.ref_world_state.restype = i32
        L.ref_world_state.argtypes = [vp, u32, vp, vp, vp, vp]
        L.ref_current_food.restype = i32
        L.ref_current_food.argtypes = [vp, u32]
        L.ref_world_food.restype = i32
        L.ref_world_food.argtypes = [vp, u32, vp]
        L.ref_set_finder.restype = ctypes.c_int
        L.ref_set_finder.argtypes = [vp, u32, vp, u32]
        L.ref_set_world_state.restype = ctypes.c_int
        L.ref_set_world_state.argtypes = [vp, u32, vp, u32, vp, u32]
        _LIB = L
    return _LIB


class RefSim:
    """The reference's simulation on the stand-in engine (numpy arrays)."""

    def __init__(self, num_worlds, rand_seed, init_num_agents_per_world, max_rows=0):
        self.num_worlds = int(num_worlds)
        self.init_agents = int(init_num_agents_per_world)
        self._destroy = lib().ref_destroy
        self._h = lib().ref_create(num_worlds, rand_seed, init_num_agents_per_world,
                                   max_rows or max(4096, 1024 * self.num_worlds))
        if not self._h:
            raise MemoryError("ref_create failed")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._destroy(h)
            self._h = None

    def step(self):
        """The reference's Step task graph (no sensor: the render system is a stub)."""
        lib().ref_step(self._h)

    def sensor(self):
        lib().ref_sensor(self._h)

    def shift_observations(self):
        lib().ref_shift_observations(self._h)

    def num_agents(self):
        return int(lib().ref_num_agents(self._h))

    def bridge_total(self):
        return int(lib().ref_bridge_total(self._h))

    def column(self, col, is_prev=False):
        dt, k = _COL_SPEC[col]
        out = np.zeros((self.num_agents(), k), dt)
        if lib().ref_read_column(self._h, col, 1 if is_prev else 0, out.ctypes.data):
            raise ValueError(f"no column {col}")
        return out

    def write_column(self, col, values):
        """Current Action / HiddenState, or the current sensor rows, per export row."""
        dt, k = _COL_SPEC[col]
        v = np.ascontiguousarray(np.asarray(values, dt).reshape(-1, k))
        if lib().ref_write_column(self._h, col, v.ctypes.data, len(v)):
            raise ValueError(f"column {col}: {len(v)} rows for {self.num_agents()} agents, or not writable")

    def species_count(self):
        """SpeciesCount as speciesInfoSync wrote it: [W, 4], before the respawns."""
        out = np.zeros((self.num_worlds, 4), np.int32)
        lib().ref_species_count(self._h, out.ctypes.data)
        return out

    def world_counts(self):
        c = np.zeros(self.num_worlds, np.int32)
        o = np.zeros(self.num_worlds, np.int32)
        lib().ref_world_counts(self._h, c.ctypes.data, o.ctypes.data)
        return c, o

    def sensor_index(self):
        c, _ = self.world_counts()
        out = np.zeros(int(c.sum()), np.int32)
        lib().ref_sensor_index(self._h, out.ctypes.data)
        return out

    def world_state(self, w):
        n = int(self.world_counts()[0][w])
        xy = np.zeros((n, 2), np.float32)
        rot = np.zeros((n, 2), np.float32)
        sp = np.zeros(n, np.int32)
        hp = np.zeros(n, np.int32)
        k = int(lib().ref_world_state(self._h, w, xy.ctypes.data, rot.ctypes.data, sp.ctypes.data, hp.ctypes.data))
        assert k == n, (k, n)
        food = np.zeros((240, 4), np.int32)
        nf = int(lib().ref_world_food(self._h, w, food.ctypes.data))
        if nf < 0:
            raise AssertionError(f"world {w}: a food entity does not stand where, or turned as, its package's draws say")
        return dict(xy=xy, rot=rot, species=sp, health=hp, food=food[:nf].copy(),
                    cur_food=int(lib().ref_current_food(self._h, w)))

    def set_finder(self, w, slots):
        s = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        if lib().ref_set_finder(self._h, int(w), s.ctypes.data, len(s)):
            raise ValueError("ref_set_finder: another population, or a slot outside it")

    def set_world_state(self, w, position, rotation_wz, food):
        xyr = np.ascontiguousarray(np.concatenate(
            [np.asarray(position, np.float32).reshape(-1, 2),
             np.asarray(rotation_wz, np.float32).reshape(-1, 2)], axis=1))
        fd = np.ascontiguousarray(np.asarray(food, np.int32).reshape(-1, 4))
        if lib().ref_set_world_state(self._h, int(w), xyr.ctypes.data, len(xyr), fd.ctypes.data, len(fd)):
            raise ValueError("ref_set_world_state: another population or an impossible food list")

    def snapshot(self, include_prev=True):
        names = ["species", "pos", "health", "surround", "reward", "action", "stats",
                 "hidden", "semantic", "depth"]
        out = {}
        for i, nm in enumerate(names):
            out[nm] = self.column(i)
            if include_prev:
                out["prev_" + nm] = self.column(i, True)
        return out
