"""madrona_bots -- MI355X-native drop-in for the reference's Python module.

Mirrors the nanobind surface of src/entry/entry.cpp:16-45:

    SimManager(gpu_id, num_worlds, rand_seed, init_num_agents_per_world)
        .step()  .shift_observations()
        .depth_tensor(is_prev)  .semantic_tensor(is_prev)  .reward_tensor(is_prev)
        .species_count_tensor() .position_tensor(is_prev)  .health_tensor(is_prev)
        .surrounding_tensor(is_prev)  .action_tensor(is_prev)
        .stats_tensor(is_prev)  .hidden_state_tensor(is_prev)

Each accessor returns a ``Tensor`` whose ``to_torch()`` is a zero-copy torch
view of memory owned by the manager (madrona::py::Tensor, mgr.cpp:70-76).
The simulation runs in libmbots.so: hand-written gfx950 kernels
(``exec_mode="hip"``, the default) or, for ``exec_mode="cpu"``
(madrona::ExecMode::CPU; learn/env.py:12-15 picks it without a GPU), the same
world step on host threads with bit-identical results and host tensor views.
Importing without the built library raises ImportError; a HIP-mode manager
without a GPU raises RuntimeError (no silent fallback).
"""
import ctypes
import os
import types
import warnings
import weakref

import torch  # loads the HIP runtime libmbots.so links against (same soname)

__all__ = ["SimManager", "ScriptBotsViewer", "Tensor", "madrona", "ExportID", "ExecMode", "unpack_rollout",
           "unpack_learner", "rebuild_learner", "CapacityWarning", "CapacityError", "MAX_CAPACITY",
           "CAPACITY_CLASSES", "TrajectoryWindow", "RENDER_PALETTE", "RENDER_SCALES", "CLS_FLOOR", "CLS_WALL",
           "CLS_FOOD", "CLS_BODY", "CLS_MARK", "PolicyNet", "policy_activation", "ACTIVATIONS", "evaluate_groups",
           "sequence_segments", "evaluate_sequences_groups", "policy_group_rows", "a2c_loss_groups", "PolicyAdam",
           "sequence_group_rows", "a2c_loss_sequences", "advantage_moments_groups", "advantage_moments_sequences",
           "ppo_loss_groups", "ppo_loss_sequences", "ppo_kl_gate"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libmbots.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        f"madrona_bots: {_LIB_PATH} is missing; build it with "
        "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950)")


class _Config(ctypes.Structure):
    _fields_ = [("gpu_id", ctypes.c_int32), ("num_worlds", ctypes.c_uint32),
                ("rand_seed", ctypes.c_uint32), ("init_num_agents_per_world", ctypes.c_uint32),
                ("sensor_size", ctypes.c_uint32), ("world_offset", ctypes.c_uint32),
                ("agent_capacity", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("exec_mode", ctypes.c_int32)]


class _LearnerOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in
                ("obs", "prev_obs", "reward", "stats", "action", "hidden", "prev_hidden")]


class _RenderOut(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in ("cls", "slot", "rgb")]


class _TrajBatch(ctypes.Structure):   # struct mbots_traj_batch
    _fields_ = [(k, ctypes.c_void_p) for k in ("rows", "t0", "len", "end", "obs", "reward", "value", "adv", "ret",
                                               "action_in", "hidden0")]


class _PolicyLayer(ctypes.Structure):   # struct mbots_policy_layer
    _fields_ = [("in_", ctypes.c_uint32), ("out", ctypes.c_uint32), ("act", ctypes.c_int32),
                ("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p)]


class _PolicyNet(ctypes.Structure):     # struct mbots_policy_net
    _fields_ = [("n_trunk", ctypes.c_uint32), ("trunk", _PolicyLayer * 4), ("actor", _PolicyLayer * 2),
                ("critic", _PolicyLayer * 2), ("memory", _PolicyLayer), ("flags", ctypes.c_uint32),
                ("gate", _PolicyLayer)]


class _PolicyGradLayer(ctypes.Structure):   # struct mbots_policy_grad_layer
    _fields_ = [("weight", ctypes.c_void_p), ("bias", ctypes.c_void_p)]


class _PolicyGrads(ctypes.Structure):   # struct mbots_policy_grads
    _fields_ = [("trunk", _PolicyGradLayer * 4), ("actor", _PolicyGradLayer * 2), ("critic", _PolicyGradLayer * 2),
                ("memory", _PolicyGradLayer), ("gate", _PolicyGradLayer)]


class _AdamTensor(ctypes.Structure):   # struct mbots_policy_adam_tensor
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("n", ctypes.c_uint64), ("group", ctypes.c_uint32)]


class _CTensor(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("device", ctypes.c_int32),
                ("dims", ctypes.c_int64 * 2)]


def _load():
    L = ctypes.CDLL(_LIB_PATH)
    vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
    P = ctypes.POINTER
    sig = {
        "mbots_create": [P(_Config), P(vp)],
        "mbots_destroy": [vp],
        "mbots_step": [vp, vp],
        "mbots_shift_observations": [vp, vp],
        "mbots_num_agents": [vp, P(u32)],
        "mbots_construct_obs": [vp, i32, vp, ctypes.c_uint64, vp],
        "mbots_checkpoint_size": [vp, P(ctypes.c_uint64)],
        "mbots_save_checkpoint": [vp, vp, ctypes.c_uint64],
        "mbots_load_checkpoint": [vp, vp, ctypes.c_uint64],
        "mbots_world_state": [vp, u32, vp, vp, vp, vp, P(i32)],
        "mbots_set_world_state": [vp, u32, vp, u32, vp, u32],
        "mbots_export": [vp, i32, P(_CTensor)],
        "mbots_export_on": [vp, i32, vp, P(_CTensor)],
        "mbots_set_action": [vp, u32, P(i32)],
        "mbots_agent_offset_for_world": [vp, u32, P(u32)],
        "mbots_write_synthetic_actions": [vp, u32, u32, i32, vp],
        "mbots_join": [vp, vp],
        "mbots_record_sensor_done": [vp, vp],
        "mbots_rollout_record_bytes": [vp, P(u32)],
        "mbots_pack_rollout": [vp, vp, ctypes.c_uint64, vp],
        "mbots_unpack_rollout": [vp, ctypes.c_uint64, i32, i32, vp, vp, vp, vp],
        "mbots_learner_record_bytes": [vp, P(u32)],
        "mbots_pack_learner": [vp, vp, ctypes.c_uint64, vp],
        "mbots_unpack_learner": [vp, ctypes.c_uint64, i32, i32, P(_LearnerOut), vp],
        "mbots_pack_learner_slim": [vp, vp, ctypes.c_uint64, vp],
        "mbots_unpack_learner_slim": [vp, ctypes.c_uint64, i32, i32, P(_LearnerOut), vp, vp],
        "mbots_rebuild_learner": [vp, ctypes.c_uint64, vp, vp, u32, vp, vp, vp, ctypes.c_uint64, vp, vp, vp,
                                  i32, vp],
        "mbots_write_actions": [vp, vp, vp, ctypes.c_uint64, vp],
        "mbots_num_rows": [vp, P(u32)],
        "mbots_agent_steps": [vp, P(ctypes.c_uint64)],
        "mbots_overflow": [vp, P(ctypes.c_uint64)],
        "mbots_enable_kernel_timing": [vp, i32],
        "mbots_kernel_times": [vp, P(ctypes.c_double), P(ctypes.c_uint64)],
        "mbots_schedule_info": [vp, P(u32)],
        "mbots_max_population": [vp, P(u32)],
        "mbots_capacity": [vp, P(u32)],
        "mbots_grow_capacity": [vp, u32],
        "mbots_set_auto_capacity": [vp, i32],
        "mbots_release_retired": [vp],
        "mbots_reset_worlds": [vp, vp, u32, vp, vp],
        "mbots_set_episode_length": [vp, u32],
        "mbots_traj_open": [vp, u32, ctypes.c_uint64],
        "mbots_traj_close": [vp],
        "mbots_traj_push": [vp, vp, vp],
        "mbots_traj_compute": [vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, P(ctypes.c_int64), P(u32), vp],
        "mbots_traj_clear": [vp, i32],
        "mbots_traj_num_tables": [vp, P(u32)],
        "mbots_traj_view": [vp, i32, u32, P(_CTensor)],
        "mbots_traj_open_ex": [vp, u32, ctypes.c_uint64, u32],
        "mbots_traj_sequences": [vp, P(ctypes.c_uint64), vp],
        "mbots_traj_batch": [vp, ctypes.c_uint64, ctypes.c_uint64, P(_TrajBatch), vp],
        "mbots_traj_gather": [vp, ctypes.c_uint64, ctypes.c_uint64, P(vp), u32, u32, vp, vp],
        "mbots_render_worlds": [vp, vp, u32, u32, P(_RenderOut), vp],
        "mbots_render_palette": [P(ctypes.c_uint8)],
        "mbots_policy_set": [vp, u32, P(_PolicyNet), vp],
        "mbots_policy_clear": [vp, u32],
        "mbots_policy_groups": [vp, P(u32), u32],
        "mbots_policy_num_groups": [vp, P(u32), P(u32)],
        "mbots_policy_set_group": [vp, u32, u32, P(_PolicyNet), vp],
        "mbots_policy_clear_group": [vp, u32, u32],
        "mbots_policy_segments": [vp, vp, vp],
        "mbots_policy_act": [vp, u32, vp, vp, vp, ctypes.c_uint64, vp],
        "mbots_policy_draw": [vp, i32, P(u32)],
        "mbots_policy_activation": [i32, vp, vp, ctypes.c_uint64, i32, vp],
        "mbots_policy_grad_workspace": [P(_PolicyNet), ctypes.c_uint64, P(ctypes.c_uint64)],
        "mbots_policy_eval": [P(_PolicyNet), vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, ctypes.c_uint64, i32, vp],
        "mbots_policy_grad": [P(_PolicyNet), vp, vp, vp, ctypes.c_uint64, vp, vp, vp, P(_PolicyGrads), vp,
                              ctypes.c_uint64, i32, vp],
        "mbots_policy_groups_workspace": [P(_PolicyNet), u32, ctypes.c_uint64, P(ctypes.c_uint64)],
        "mbots_policy_eval_groups": [P(_PolicyNet), u32, vp, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, vp,
                                     ctypes.c_uint64, i32, vp],
        "mbots_policy_grad_groups": [P(_PolicyNet), u32, vp, vp, vp, vp, ctypes.c_uint64, vp, vp, vp, P(_PolicyGrads), vp,
                                     ctypes.c_uint64, i32, vp],
        "mbots_policy_seq_workspace": [P(_PolicyNet), u32, ctypes.c_uint64, P(ctypes.c_uint64)],
        "mbots_policy_seq_eval": [P(_PolicyNet), vp, vp, vp, vp, u32, ctypes.c_uint64, vp, vp, vp, vp, vp,
                                  ctypes.c_uint64, i32, vp],
        "mbots_policy_seq_grad": [P(_PolicyNet), vp, vp, vp, vp, u32, ctypes.c_uint64, vp, vp, vp, P(_PolicyGrads), vp,
                                  ctypes.c_uint64, i32, vp],
        "mbots_policy_seq_order": [vp, ctypes.c_uint64, u32, vp, vp, vp, ctypes.c_uint64, i32, vp],
        "mbots_policy_seq_groups_workspace": [P(_PolicyNet), u32, u32, ctypes.c_uint64, P(ctypes.c_uint64)],
        "mbots_policy_seq_eval_groups": [P(_PolicyNet), u32, vp, vp, vp, vp, vp, vp, u32, ctypes.c_uint64, vp, vp, vp,
                                         vp, vp, ctypes.c_uint64, i32, vp],
        "mbots_policy_seq_grad_groups": [P(_PolicyNet), u32, vp, vp, vp, vp, vp, vp, u32, ctypes.c_uint64, vp, vp, vp,
                                         P(_PolicyGrads), vp, ctypes.c_uint64, i32, vp],
        "mbots_policy_group_rows": [vp, u32, vp, i32, vp],
        "mbots_policy_a2c_loss": [vp, vp, vp, vp, vp, vp, ctypes.c_uint64, vp, u32, vp, ctypes.c_float, ctypes.c_float,
                                  vp, vp, vp, vp, i32, vp],
        "mbots_policy_adam": [P(_AdamTensor), ctypes.c_uint64, vp, u32, vp, ctypes.c_float, ctypes.c_float,
                              ctypes.c_float, ctypes.c_float, i32, vp],
        "mbots_policy_seq_group_rows": [vp, vp, vp, ctypes.c_uint64, vp, vp, u32, i32, vp, i32, vp],
        "mbots_policy_seq_a2c_loss": [vp, vp, vp, vp, vp, vp, vp, vp, u32, ctypes.c_uint64, vp, vp, u32, i32, vp,
                                      ctypes.c_float, ctypes.c_float, vp, vp, vp, vp, i32, vp],
        "mbots_policy_adam_clip_workspace": [P(_AdamTensor), ctypes.c_uint64, u32, P(ctypes.c_uint64)],
        "mbots_policy_adam_clip": [P(_AdamTensor), ctypes.c_uint64, vp, u32, vp, ctypes.c_float, ctypes.c_float,
                                   ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp, vp,
                                   ctypes.c_uint64, i32, vp],
        "mbots_policy_ppo_workspace": [ctypes.c_uint64, u32, P(ctypes.c_uint64)],
        "mbots_policy_adv_moments": [vp, vp, ctypes.c_uint64, vp, u32, vp, vp, ctypes.c_uint64, i32, vp],
        "mbots_policy_ppo_loss": [vp] * 8 + [ctypes.c_uint64, vp, u32, vp, vp] + [ctypes.c_float] * 4 + [vp] * 5 +
                                 [ctypes.c_uint64, i32, vp],
        "mbots_policy_seq_adv_moments": [vp, vp, vp, vp, u32, ctypes.c_uint64, vp, vp, u32, i32, vp, vp,
                                         ctypes.c_uint64, i32, vp],
        "mbots_policy_seq_ppo_loss": [vp] * 10 + [u32, ctypes.c_uint64, vp, vp, u32, i32, vp, vp] +
                                     [ctypes.c_float] * 4 + [vp] * 5 + [ctypes.c_uint64, i32, vp],
        "mbots_policy_ppo_gate": [vp, vp, u32, ctypes.c_double, vp, i32, vp],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    L.mbots_last_error.restype = ctypes.c_char_p
    L.mbots_last_error.argtypes = []
    return L


_lib = _load()


def _check(rc):
    if rc != 0:
        msg = _lib.mbots_last_error().decode(errors="replace")
        raise (CapacityError if rc == _E_CAPACITY else RuntimeError)(f"madrona_bots: {msg} (status {rc})")


_W_CAPACITY, _E_CAPACITY = 1, -5   # include/mbots.h MBOTS_W_CAPACITY / MBOTS_E_CAPACITY
MAX_CAPACITY = 4096                # MBOTS_MAX_CAPACITY
CAPACITY_CLASSES = (128, 256, 512, 1024, 2048, 4096)   # the kernels' slot classes


# the rasteriser's class codes (include/mbots.h MBOTS_RENDER_*): a body is
# CLS_BODY + species - 1 (4..7), a heading mark CLS_MARK + species - 1 (8..11)
CLS_FLOOR, CLS_WALL, CLS_FOOD, CLS_BODY, CLS_MARK = 0, 1, 2, 4, 8
RENDER_SCALES = (1, 2, 4, 8)
RENDER_H, RENDER_W = 96, 128       # image rows / columns at scale 1


def _render_palette():
    import numpy as np
    buf = (ctypes.c_uint8 * 36)()
    _check(_lib.mbots_render_palette(buf))
    pal = np.frombuffer(bytes(buf), dtype=np.uint8).reshape(12, 3).copy()
    pal.setflags(write=False)
    return pal


def _capacity_class(need):
    """The smallest kernel capacity class holding `need` agents (the largest
    class when none does)."""
    for c in CAPACITY_CLASSES:
        if need <= c:
            return c
    return MAX_CAPACITY


class CapacityWarning(RuntimeWarning):
    """Births or respawns were dropped because a world reached agent_capacity:
    the reference's worlds have no cap (sim.cpp:561-564, :830-834), so the run
    now differs from the reference's (MBOTS_W_CAPACITY)."""


class CapacityError(RuntimeError):
    """CapacityWarning under strict_capacity=True (MBOTS_E_CAPACITY); the step ran."""


class ExportID:
    """enum class ExportID (src/sim/sim.hpp:18-55) + build extensions."""
    Reset, Action, PrevAction, HiddenState, PrevHiddenState, Reward, PrevReward, Done, \
        Position, PrevPosition, Health, PrevHealth, Surrounding, PrevSurrounding, \
        SensorSemantic, SensorDepth, PrevSensorSemantic, PrevSensorDepth, Stats, PrevStats, \
        SensorIndex, SpeciesCount = range(22)
    Species, PrevSpecies, Episode, EpisodeStep = 32, 33, 34, 35


_DTYPES = {0: (torch.uint8, "|u1"), 1: (torch.int8, "|i1"), 2: (torch.int32, "<i4"),
           3: (torch.float32, "<f4")}
_DTYPE_CODE = {v[0]: k for k, v in _DTYPES.items()}


def _raw_stream(device):
    """hipStream_t of torch's current stream on `device` (no Stream object)."""
    return torch._C._cuda_getCurrentRawStream(device)

FLAG_REWARD_FIXED = 0x1
FLAG_FIX_DEPTH_ALIAS = 0x2
FLAG_SHARD_GHOST = 0x4
FLAG_STRICT_CAPACITY = 0x8


class ExecMode:
    """madrona::ExecMode (MBOTS_EXEC_*)."""
    CUDA = HIP = 0
    CPU = 1


def _exec_mode(v):
    if isinstance(v, str):
        v = {"hip": ExecMode.HIP, "cuda": ExecMode.HIP, "gpu": ExecMode.HIP,
             "cpu": ExecMode.CPU}.get(v.lower())
        if v is None:
            raise ValueError("exec_mode must be 'hip' or 'cpu'")
    v = int(v)
    if v not in (ExecMode.HIP, ExecMode.CPU):
        raise ValueError(f"unknown exec_mode {v}")
    return v


RENDER_PALETTE = _render_palette()   # uint8 [12, 3]: RGB per class code (mbots_render_palette)

OBS_DIM = 69   # learn/env.py:19
# TK_* indices of mbots_kernel_times
KERNELS = ("world_step", "scan", "export", "sensor", "shift", "actions", "move", "obs")


# per-world exports (not table columns)
_WORLD_EXPORTS = (ExportID.SpeciesCount, ExportID.Reset, ExportID.Episode, ExportID.EpisodeStep)


class _Handle:
    """One manager's library handle (mbots_create / mbots_destroy).  Every
    exported view holds it -- a torch view's storage holds the Tensor whose
    array interface it was built from, and that Tensor holds this -- so a view
    outlives the SimManager that produced it.  The manager's view
    cache holds views, which hold this handle and never the manager, so there
    is no reference cycle: the device memory is freed by reference counting
    once the manager and every view of it are gone."""
    __slots__ = ("h",)

    def __init__(self, h):
        self.h = h

    def __del__(self):
        h = self.h
        if h and _lib is not None:   # module globals may be gone at interpreter exit
            _lib.mbots_destroy(h)
            self.h = None


class Tensor:
    """Non-owning device tensor view (madrona::py::Tensor)."""

    def __init__(self, keep, ct, column=False, mgr=None):
        self._keep = keep            # the manager's _Handle: keeps its memory alive
        self._mgr = mgr              # the manager (its view cache), for table columns
        self._column = column        # a table column: W x cap row slots behind it
        self._gen = mgr._gen if mgr is not None else 0   # the manager's storage it points into
        self._ptr = int(ct.data or 0)
        self._torch_dtype, self._typestr = _DTYPES[ct.dtype]
        self._device = int(ct.device)
        self.shape = (int(ct.dims[0]), int(ct.dims[1]))

    def devicePtr(self):
        return self._ptr

    @property
    def dtype(self):
        return self._torch_dtype

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self._typestr, "data": (self._ptr, False),
                "version": 3, "strides": None, "stream": None}

    def to_torch(self):
        """Zero-copy torch view on cuda:<gpu_id> (host memory in CPU mode)."""
        if self._device < 0:
            return self._host_view()
        dev = torch.device("cuda", self._device)
        if self.shape[0] == 0:
            return torch.empty(self.shape, dtype=self._torch_dtype, device=dev)
        # one torch view per column allocation, sliced to the current row count:
        # the learner reads ~10 views per step and is host-bound at small world
        # counts (scripts/refhost.py); building a view from the array interface
        # every time is most of an accessor's host cost
        # (a view taken before a capacity growth belongs to the manager's
        # previous storage: no cached view of the current one)
        base = self._mgr._view_cache(self) if (self._column and self._mgr is not None
                                                and self._keep is self._mgr._hd
                                                and self._gen == self._mgr._gen) else None
        if base is not None:
            return base[:self.shape[0]]
        t = torch.as_tensor(self, device=dev)
        if t.data_ptr() != self._ptr:
            raise RuntimeError("madrona_bots: to_torch() produced a copy, expected a view")
        return t

    def _host_view(self):
        import numpy as np
        npdt = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int32: np.int32,
                torch.float32: np.float32}[self._torch_dtype]
        n = self.shape[0] * self.shape[1]
        if n == 0:
            return torch.empty(self.shape, dtype=self._torch_dtype)
        buf = (ctypes.c_char * (n * np.dtype(npdt).itemsize)).from_address(self._ptr)
        buf._keep = self._keep       # the view (numpy base -> buffer) keeps the manager's memory
        t = torch.from_numpy(np.frombuffer(buf, dtype=npdt, count=n).reshape(self.shape))
        if t.data_ptr() != self._ptr:
            raise RuntimeError("madrona_bots: to_torch() produced a copy, expected a view")
        return t


def unpack_rollout(records, with_depth=None):
    """Learner side of the config-5 gather: uint8 [N, 64 | 96] rollout records
    (SimManager.pack_rollout, gathered from every rank) -> {"obs": float32
    [N, 69] (construct_obs, bit-identical), "reward": float32 [N, 1],
    "stats": int32 [N, 4]} on the records' device (mbots_unpack_rollout)."""
    if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] not in (64, 96):
        raise ValueError("records must be uint8 [N, 64] or [N, 96]")
    depth = records.shape[1] == 96 if with_depth is None else bool(with_depth)
    if depth != (records.shape[1] == 96):
        raise ValueError("with_depth does not match the record width")
    rec = records.contiguous()
    n = rec.shape[0]
    dev = rec.device
    obs = torch.empty((n, OBS_DIM), dtype=torch.float32, device=dev)
    rew = torch.empty((n, 1), dtype=torch.float32, device=dev)
    st = torch.empty((n, 4), dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None)
    _check(_lib.mbots_unpack_rollout(ctypes.c_void_p(rec.data_ptr()), n, 1 if depth else 0,
                                     dev.index if dev.type == "cuda" else -1,
                                     ctypes.c_void_p(obs.data_ptr()), ctypes.c_void_p(rew.data_ptr()),
                                     ctypes.c_void_p(st.data_ptr()), stream))
    return {"obs": obs, "reward": rew, "stats": st}


LEARNER_BYTES, LEARNER_BYTES_DEPTH = 272, 336
LEARNER_SLIM_BYTES, LEARNER_SLIM_BYTES_DEPTH = 128, 192
_LEARNER_KEYS = ("obs", "prev_obs", "reward", "stats", "action", "hidden", "prev_hidden")
_SLIM_KEYS = ("obs", "prev_obs", "reward", "stats", "src")


def unpack_learner(records, with_depth=None, keys=None):
    """Learner side of the config-5 round trip: uint8 [N, 272 | 336] learner
    records (SimManager.pack_learner, gathered from every rank) -> the columns
    learn/training_loop.py reads after step(): "obs" / "prev_obs" float32
    [N, 69] (construct_obs of the current / previous columns, bit-identical),
    "reward" [N, 1], "stats" int32 [N, 4], "action" int32 [N, 6], "hidden" /
    "prev_hidden" float32 [N, 16] (mbots_unpack_learner), on the records'
    device; `keys` selects the outputs.  Slim records (uint8 [N, 128 | 192],
    SimManager.pack_learner(slim=True)) give "obs", "prev_obs", "reward",
    "stats" and "src" int32 [N] -- each row's index in the table before the
    step, -1 for a newborn (mbots_unpack_learner_slim; harness/gather.py
    rebuilds action / hidden / prev_hidden from it)."""
    widths = (LEARNER_BYTES, LEARNER_BYTES_DEPTH, LEARNER_SLIM_BYTES, LEARNER_SLIM_BYTES_DEPTH)
    if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] not in widths:
        raise ValueError(f"records must be uint8 [N, w], w in {widths}")
    slim = records.shape[1] in (LEARNER_SLIM_BYTES, LEARNER_SLIM_BYTES_DEPTH)
    wide = LEARNER_SLIM_BYTES_DEPTH if slim else LEARNER_BYTES_DEPTH
    depth = records.shape[1] == wide if with_depth is None else bool(with_depth)
    if depth != (records.shape[1] == wide):
        raise ValueError("with_depth does not match the record width")
    keys = (_SLIM_KEYS if slim else _LEARNER_KEYS) if keys is None else tuple(keys)
    allowed = _SLIM_KEYS if slim else _LEARNER_KEYS
    if any(k not in allowed for k in keys):
        raise ValueError(f"keys must be among {allowed}")
    rec = records.contiguous()
    n, dev = rec.shape[0], rec.device
    shapes = {"obs": ((n, OBS_DIM), torch.float32), "prev_obs": ((n, OBS_DIM), torch.float32),
              "reward": ((n, 1), torch.float32), "stats": ((n, 4), torch.int32),
              "action": ((n, 6), torch.int32), "hidden": ((n, 16), torch.float32),
              "prev_hidden": ((n, 16), torch.float32), "src": ((n,), torch.int32)}
    out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in keys}
    lo = _LearnerOut(**{k: (out[k].data_ptr() if k in out else None) for k in _LEARNER_KEYS})
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None)
    devi = dev.index if dev.type == "cuda" else -1
    if slim:
        src = ctypes.c_void_p(out["src"].data_ptr() if "src" in out else None)
        _check(_lib.mbots_unpack_learner_slim(ctypes.c_void_p(rec.data_ptr()), n, 1 if depth else 0, devi,
                                              ctypes.byref(lo), src, stream))
    else:
        _check(_lib.mbots_unpack_learner(ctypes.c_void_p(rec.data_ptr()), n, 1 if depth else 0, devi,
                                         ctypes.byref(lo), stream))
    return out


def rebuild_learner(src, cur_counts, last_counts, last_action, last_memory, last_hidden):
    """The learner rank's rebuild from slim records (mbots_rebuild_learner):
    src int32 [N] (unpack_learner of slim records, in the reassembled global
    order), cur_counts / last_counts int64 [ranks, 4] species rows per rank of
    the gathered and of the last table, last_action int32 [M, 6] /
    last_memory f32 [M, 16] (the learner's writes after the last step) and
    last_hidden f32 [M, 16] (that step's HiddenState), all on one device (or
    the host) -> {"action" [N, 6], "hidden" [N, 16], "prev_hidden" [N, 16]}:
    the manager's Action, HiddenState and PrevHiddenState, bit-identical."""
    dev = src.device
    n = src.shape[0]
    cc = torch.as_tensor(cur_counts, dtype=torch.int64).cpu().contiguous()
    lc = torch.as_tensor(last_counts, dtype=torch.int64).cpu().contiguous()
    if cc.dim() != 2 or cc.shape[1] != 4 or lc.shape != cc.shape:
        raise ValueError("cur_counts / last_counts must be int64 [ranks, 4] of the same ranks")
    la = last_action.to(device=dev, dtype=torch.int32).contiguous()
    lm = last_memory.to(device=dev, dtype=torch.float32).contiguous()
    lh = last_hidden.to(device=dev, dtype=torch.float32).contiguous()
    s = src.to(torch.int32).contiguous()
    out = {"action": torch.empty((n, 6), dtype=torch.int32, device=dev),
           "hidden": torch.empty((n, 16), dtype=torch.float32, device=dev),
           "prev_hidden": torch.empty((n, 16), dtype=torch.float32, device=dev)}
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    _check(_lib.mbots_rebuild_learner(ptr(s), n, ptr(cc), ptr(lc), cc.shape[0], ptr(la), ptr(lm), ptr(lh),
                                      la.shape[0], ptr(out["action"]), ptr(out["hidden"]), ptr(out["prev_hidden"]),
                                      dev.index if dev.type == "cuda" else -1, stream))
    return out


madrona = types.ModuleType("madrona_bots.madrona")
madrona.ExecMode = ExecMode
madrona.Tensor = Tensor


class SimManager:
    """Manager (src/entry/mgr.hpp:10-68) with the nanobind constructor
    signature (entry.cpp:17-28).  Keyword-only extensions: exec_mode ("hip" /
    "cpu" or ExecMode.*: the Manager's ExecMode), agent_capacity
    (per-world slot cap), world_offset (global index of this shard's first
    world), reward_fixed (rewards[speciesID-1] instead of the reference's
    off-by-one), fix_depth_alias (depth_tensor returns real depth,
    SURVEY B.1), shard_ghost (also step world world_offset + num_worlds, never
    exported, so a shard's faithful B.3 rewards equal one device's; its agents
    act on the write_synthetic_actions stream), strict_capacity (a world that
    reaches agent_capacity -- at most MAX_CAPACITY = 4096 slots -- and drops a
    birth or respawn makes step() raise CapacityError instead of warning with
    CapacityWarning: the reference has no cap).

    auto_grow=True grows the worlds' capacity instead of dropping agents:
    before each step() the manager reads the largest world population n
    (mbots_max_population: a wait for the last step's row counts, not for its
    sensor) and, when the step could overflow -- a step adds at most n births
    (one per agent, sim.cpp:561-564) and A respawns (:830-834) -- moves its
    state into the smallest capacity class (128, 256, 512, 1024, 2048, 4096)
    that holds 2 n + A, so the run stays the reference's (bitwise equal to a
    manager that never drops) up to 4096 agents per world.  The run starts at
    agent_capacity; agent_capacity="auto" is the class of 3 A with growth on.
    In HIP mode the growth is the library's (mbots_set_auto_capacity: a
    device-side move inside the same handle), in CPU mode a hand-over to a
    new native manager through a checkpoint.  A sharded run grows each
    rank on its own worlds (shard_ghost counted): results do not depend on
    the class a world runs in.  grow_capacity(cap) grows by hand.  Views
    fetched before a growth keep reading the storage they were taken from
    (kept until release_retired() or the manager's end) but no longer follow
    the manager: take them after step(), as learn/training_loop.py:43-50 does.
    A step captured into a HIP graph pins the capacity.

    Episodes: reset_worlds(worlds, episodes=None) flags worlds (global
    indices) to start over at the next step() -- reset, then step: the world is
    re-initialised from its episode's key (episode e of global world gw:
    threefry2x32(seed, 0, e, gw), the reference's split_i(initKey, episode,
    world); episode 0 is the world the constructor builds) and then stepped
    like the others, its agents' rows new (Action, HiddenState and every Prev
    column zero).  reset_tensor() is the live flag array (0 none, 1 next
    episode, v >= 2 episode v - 2; the step clears what it consumes),
    episode_tensor() / episode_step_tensor() each world's episode and its
    steps since the last reset or creation.  episode_length=k (or
    set_episode_length(k)) resets every world whose episode_step has reached k.
    A manager that uses none of these steps exactly as before.

    Multi-step returns: trajectory_window(horizon, max_rows) opens the
    manager's TrajectoryWindow, which follows every agent through the species
    sort over up to `horizon` tables and computes lifelines, discounted returns
    and GAE(lambda) advantages on the device (INTEGRATION.md "Multi-step
    returns").  While one is open, a CPU-mode manager with growth on grows in
    place (grow_capacity) rather than through a checkpoint hand-over, which
    would leave the window behind."""

    def __init__(self, gpu_id, num_worlds, rand_seed, init_num_agents_per_world, *,
                 exec_mode="hip", agent_capacity=128, world_offset=0, reward_fixed=False,
                 fix_depth_alias=False, shard_ghost=False, strict_capacity=False, auto_grow=False,
                 episode_length=0):
        self.exec_mode = _exec_mode(exec_mode)
        self.gpu_id = int(gpu_id)
        self.num_worlds = int(num_worlds)
        self._auto_cap = isinstance(agent_capacity, str) or bool(auto_grow)
        if isinstance(agent_capacity, str):
            if agent_capacity != "auto":
                raise ValueError('agent_capacity must be an int or "auto"')
            agent_capacity = _capacity_class(3 * int(init_num_agents_per_world))
        self.agent_capacity = int(agent_capacity)
        flags = (FLAG_REWARD_FIXED if reward_fixed else 0) | \
                (FLAG_FIX_DEPTH_ALIAS if fix_depth_alias else 0) | \
                (FLAG_SHARD_GHOST if shard_ghost else 0) | \
                (FLAG_STRICT_CAPACITY if strict_capacity else 0)
        self._cfg = (self.gpu_id, self.num_worlds, int(rand_seed) & 0xFFFFFFFF,
                     int(init_num_agents_per_world), 32, int(world_offset), flags, self.exec_mode)
        self._ghost = bool(shard_ghost)
        self._fix_depth = bool(fix_depth_alias)
        self._ktiming = False
        self._gen = 0                # bumped when the columns' storage moves (a growth)
        self._traj = None            # the open TrajectoryWindow, if any
        self._policy = [[None] * 4]  # the PolicyNet set per (group, species) (set_policy)
        self._episode_length = int(episode_length)
        if not 0 <= self._episode_length < 2 ** 32:
            raise ValueError("episode_length must be in [0, 2^32)")
        self._open(self.agent_capacity)
        if self._episode_length:
            _check(_lib.mbots_set_episode_length(self._h, self._episode_length))

    def _open(self, cap):
        """Create the native manager at capacity `cap` (and reset the caches
        that belong to one)."""
        g, W, seed, A, sensor, off, flags, mode = self._cfg
        cfg = _Config(g, W, seed, A, sensor, off, int(cap), flags, mode)
        h = ctypes.c_void_p()
        _check(_lib.mbots_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._hd = _Handle(h)        # destroyed when the manager and all its views are gone
        self._h = h
        if self._auto_cap and self.exec_mode == ExecMode.HIP:
            _check(_lib.mbots_set_auto_capacity(h, 1))   # mbots_step grows in place
        self._set_capacity(cap)

    def _set_capacity(self, cap):
        self.agent_capacity = int(cap)
        # row slots of every table column (the shard ghost is one more world)
        self._cap_rows = (self.num_worlds + (1 if self._ghost else 0)) * self.agent_capacity
        self._views = {}
        self._gen += 1

    def _refresh_capacity(self):
        """Follow a growth the library did (mbots_capacity: host state, no
        synchronisation)."""
        v = ctypes.c_uint32()
        _check(_lib.mbots_capacity(self._h, ctypes.byref(v)))
        if v.value != self.agent_capacity:
            self._set_capacity(v.value)

    def grow_capacity(self, cap):
        """Move the manager into `cap` slots per world in place
        (mbots_grow_capacity: same handle, device-side in HIP mode); `cap`
        equal to agent_capacity does nothing, a smaller one or one above
        MAX_CAPACITY raises.  Views taken before read the retired storage."""
        _check(_lib.mbots_grow_capacity(self._h, int(cap)))
        self._refresh_capacity()

    def release_retired(self):
        """Free the storage earlier growths retired (mbots_release_retired);
        views taken before those growths must not be used afterwards."""
        _check(_lib.mbots_release_retired(self._h))

    def _grow_if_needed(self):
        """CPU mode with growth on: the next capacity class before a step that
        could overflow this one (at most 2 n + A agents after it), handed
        over to a new native manager through a checkpoint."""
        if self.agent_capacity >= MAX_CAPACITY:
            return
        # (waits for the last step's row counts only, not for its sensor or the
        # caller's chain: the device stays fed while the host runs one step ahead)
        v = ctypes.c_uint32()
        _check(_lib.mbots_max_population(self._h, ctypes.byref(v)))
        need = 2 * int(v.value) + self._cfg[3]
        if need <= self.agent_capacity:
            return
        if self._traj is not None:
            # an open trajectory window lives in the native manager: grow that
            # one in place (mbots_grow_capacity), which leaves the window intact
            self.grow_capacity(_capacity_class(need))
            return
        blob = self.save_checkpoint()
        old = (self._hd, self._h, self.agent_capacity, self._cap_rows, self._views, self._gen)
        self._open(_capacity_class(need))   # (raises with the manager unchanged)
        try:
            _check(_lib.mbots_load_checkpoint(self._h, ctypes.c_void_p(blob.ctypes.data), blob.size))
        except BaseException:
            # keep running in the old class rather than on a fresh world
            self._hd, self._h, self.agent_capacity, self._cap_rows, self._views, self._gen = old
            raise
        if self._ktiming:
            self.enable_kernel_timing(True)
        # the groups, the nets and the draw counter follow the hand-over
        if len(self._policy) > 1 or any(n is not None for n in self._policy[0]):
            draw = ctypes.c_uint32()
            _check(_lib.mbots_policy_draw(old[1], 0, ctypes.byref(draw)))
            nets, self._policy = self._policy, [[None] * 4]
            starts = (ctypes.c_uint32 * 64)()
            n = ctypes.c_uint32()
            _check(_lib.mbots_policy_num_groups(old[1], ctypes.byref(n), starts))
            self.set_policy_groups(list(starts[:n.value]))
            for g, four in enumerate(nets):
                for sp, net in enumerate(four):
                    if net is not None:
                        self._set_policy_one(sp + 1, net, g)
            _check(_lib.mbots_policy_draw(self._h, 1, ctypes.byref(draw)))
        del old                      # (freed now unless a view still holds it)

    def _stream(self):
        if self.exec_mode == ExecMode.CPU:
            return ctypes.c_void_p(None)
        return ctypes.c_void_p(_raw_stream(self.gpu_id))

    def _view_cache(self, tensor):
        """Torch view of the whole allocation behind `tensor` (every row slot
        the manager reserved for that column), created once; None for exports
        that are not table columns."""
        rows, cols = tensor.shape
        cap_rows = self._cap_rows
        if rows > cap_rows:
            return None
        key = (tensor._ptr, tensor._torch_dtype, cols)
        base = self._views.get(key)
        if base is None:
            # (owned by the handle, not the manager: no cycle through the cache)
            full = Tensor(self._hd, _CTensor(tensor._ptr, _DTYPE_CODE[tensor._torch_dtype], tensor._device,
                                             (ctypes.c_int64 * 2)(cap_rows, cols)))
            base = torch.as_tensor(full, device=torch.device("cuda", tensor._device))
            if base.data_ptr() != tensor._ptr:
                raise RuntimeError("madrona_bots: to_torch() produced a copy, expected a view")
            self._views[key] = base
        return base

    @property
    def device(self):
        """torch device of the exported views."""
        if self.exec_mode == ExecMode.CPU:
            return torch.device("cpu")
        return torch.device("cuda", self.gpu_id)

    # -- graphs -------------------------------------------------------------
    def step(self):
        native = self._auto_cap and self.exec_mode == ExecMode.HIP
        if self._auto_cap and not native:
            self._grow_if_needed()
        rc = _lib.mbots_step(self._h, self._stream())
        if native:
            self._refresh_capacity()
        if rc == _W_CAPACITY:   # the step ran; agents were dropped at the cap (reported late by a few steps)
            warnings.warn(f"madrona_bots: {_lib.mbots_last_error().decode(errors='replace')}",
                          CapacityWarning, stacklevel=2)
        elif rc:
            _check(rc)

    def shift_observations(self):
        _check(_lib.mbots_shift_observations(self._h, self._stream()))

    # -- exports ------------------------------------------------------------
    def _export(self, eid):
        # stream-ordered on torch's current stream: the view's deferred copies
        # and joins are enqueued there, after everything the manager enqueued
        # on whatever stream its previous call used (mbots_export_on)
        ct = _CTensor()
        _check(_lib.mbots_export_on(self._h, eid, self._stream(), ctypes.byref(ct)))
        return Tensor(self._hd, ct, column=eid not in _WORLD_EXPORTS, mgr=self)

    def depth_tensor(self, is_prev=False):
        return self._export(ExportID.PrevSensorDepth if is_prev else ExportID.SensorDepth)

    def semantic_tensor(self, is_prev=False):
        return self._export(ExportID.PrevSensorSemantic if is_prev else ExportID.SensorSemantic)

    def reward_tensor(self, is_prev=False):
        return self._export(ExportID.PrevReward if is_prev else ExportID.Reward)

    def species_count_tensor(self):
        return self._export(ExportID.SpeciesCount)

    def position_tensor(self, is_prev=False):
        return self._export(ExportID.PrevPosition if is_prev else ExportID.Position)

    def health_tensor(self, is_prev=False):
        return self._export(ExportID.PrevHealth if is_prev else ExportID.Health)

    def surrounding_tensor(self, is_prev=False):
        return self._export(ExportID.PrevSurrounding if is_prev else ExportID.Surrounding)

    def action_tensor(self, is_prev=False):
        return self._export(ExportID.PrevAction if is_prev else ExportID.Action)

    def stats_tensor(self, is_prev=False):
        return self._export(ExportID.PrevStats if is_prev else ExportID.Stats)

    def hidden_state_tensor(self, is_prev=False):
        return self._export(ExportID.PrevHiddenState if is_prev else ExportID.HiddenState)

    # C++-only accessors of the reference (mgr.hpp:38, :54-62) + extensions
    def sensor_index_tensor(self):
        return self._export(ExportID.SensorIndex)

    def done_tensor(self):
        return self._export(ExportID.Done)

    def species_tensor(self, is_prev=False):
        return self._export(ExportID.PrevSpecies if is_prev else ExportID.Species)

    # -- episodes -----------------------------------------------------------
    def reset_tensor(self):
        """The live reset flags, int32 [num_worlds, 1] (MBOTS_EXPORT_RESET):
        write 1 to start a world's next episode at the next step(), e + 2 for
        episode e.  Taking it arms the manager."""
        return self._export(ExportID.Reset)

    def episode_tensor(self):
        """Each world's current episode, int32 [num_worlds, 1]."""
        return self._export(ExportID.Episode)

    def episode_step_tensor(self):
        """Steps since each world's last reset or creation, int32
        [num_worlds, 1] (1 after the step that reset it)."""
        return self._export(ExportID.EpisodeStep)

    def reset_worlds(self, worlds, episodes=None):
        """Flag `worlds` (a sequence or tensor of global world indices) to
        start over at the next step(): each at its next episode, or at
        episodes[k].  Indices outside this manager's worlds are ignored (every
        rank of a sharded run takes the same list)."""
        import numpy as np

        def arr(v, what):
            if isinstance(v, torch.Tensor):
                v = v.detach().cpu().numpy()
            v = np.asarray(list(v) if not isinstance(v, np.ndarray) else v).reshape(-1)
            if v.size and (v.min() < 0 or v.max() >= 2 ** 32):
                raise ValueError(f"madrona_bots: {what} out of range")
            return np.ascontiguousarray(v, dtype=np.uint32)

        w = arr(worlds, "world index")
        e = None
        if episodes is not None:
            e = arr(episodes, "episode")
            if e.size != w.size:
                raise ValueError(f"madrona_bots: {w.size} worlds but {e.size} episodes")
        _check(_lib.mbots_reset_worlds(self._h, ctypes.c_void_p(w.ctypes.data if w.size else None), int(w.size),
                                       ctypes.c_void_p(e.ctypes.data if e is not None and e.size else None),
                                       self._stream()))

    def set_episode_length(self, steps):
        """Reset every world whose episode_step has reached `steps` at the
        start of a step (0: off)."""
        _check(_lib.mbots_set_episode_length(self._h, int(steps)))
        self._episode_length = int(steps)

    # -- multi-step returns -------------------------------------------------
    def trajectory_window(self, horizon, max_rows, *, sequences=False, record_obs=False, record_state=False):
        """Open the manager's trajectory window (mbots_traj_open_ex): up to
        `horizon` consecutive tables of up to `max_rows` rows each.  Returns a
        TrajectoryWindow; one per manager, until its close().  The opt-in
        parts behind TrajectoryWindow.sequences() / batch() / gather():
        sequences (MBOTS_TRAJ_SEQ), record_obs (each push stores the rows'
        rollout records, MBOTS_TRAJ_REC_OBS), record_state (HiddenState and the
        Action mask, MBOTS_TRAJ_REC_STATE); a record_* implies sequences."""
        if self._traj is not None:
            raise RuntimeError("madrona_bots: the manager already holds a trajectory window")
        flags = (TrajectoryWindow.FLAG_SEQ if sequences or record_obs or record_state else 0) | \
                (TrajectoryWindow.FLAG_REC_OBS if record_obs else 0) | \
                (TrajectoryWindow.FLAG_REC_STATE if record_state else 0)
        _check(_lib.mbots_traj_open_ex(self._h, int(horizon), int(max_rows), flags))
        self._traj = TrajectoryWindow(self, int(horizon), int(max_rows), flags)
        return self._traj

    def set_action(self, agent_idx, forward, backward, rotate_left, rotate_right, shoot, breed):
        a = (ctypes.c_int32 * 6)(forward, backward, rotate_left, rotate_right, shoot, breed)
        _check(_lib.mbots_set_action(self._h, int(agent_idx), a))

    def agent_offset_for_world(self, world_idx):
        v = ctypes.c_uint32()
        _check(_lib.mbots_agent_offset_for_world(self._h, int(world_idx), ctypes.byref(v)))
        return v.value

    # -- build utilities ------------------------------------------------------
    def num_agents(self):
        v = ctypes.c_uint32()
        _check(_lib.mbots_num_agents(self._h, ctypes.byref(v)))
        return v.value

    def construct_obs(self, is_prev=False, out=None):
        """learn/util.py construct_obs over all N rows (every species, species-
        major) in one fused kernel: float32 [N, 69] = depth | health | position |
        semantic | surrounding, bit-identical to the torch.cat of the views.
        Slice [start:end] per species with species_count_tensor()."""
        import torch
        n = self.num_agents()
        if out is None:
            out = torch.empty((n, OBS_DIM), dtype=torch.float32, device=self.device)
        if out.dtype != torch.float32 or out.device != self.device or not out.is_contiguous() \
                or out.dim() != 2 or out.shape[1] != OBS_DIM or out.shape[0] < n:
            raise ValueError(f"out must be a contiguous float32 [>= {n}, {OBS_DIM}] tensor on "
                             f"{self.device}")
        _check(_lib.mbots_construct_obs(self._h, 1 if is_prev else 0,
                                        ctypes.c_void_p(out.data_ptr()), out.shape[0],
                                        self._stream()))
        return out[:n]

    def rollout_record_bytes(self):
        """Bytes per rollout record (include/mbots.h: 64, or 96 with real depth)."""
        v = ctypes.c_uint32()
        _check(_lib.mbots_rollout_record_bytes(self._h, ctypes.byref(v)))
        return v.value

    def pack_rollout(self, out=None):
        """The raw columns the learner reads after step() (semantic, health,
        position, surrounding, reward, stats; depth when fixed) as one uint8
        [N, rollout_record_bytes()] record per export row -- the payload of the
        config-5 gather to the learner rank; unpack_rollout()
        rebuilds construct_obs rows from it.  `out` may hold more rows (padding)."""
        import torch
        n = self.num_agents()
        rb = self.rollout_record_bytes()
        if out is None:
            out = torch.empty((n, rb), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() \
                or out.dim() != 2 or out.shape[1] != rb or out.shape[0] < n:
            raise ValueError(f"out must be a contiguous uint8 [>= {n}, {rb}] tensor on {self.device}")
        _check(_lib.mbots_pack_rollout(self._h, ctypes.c_void_p(out.data_ptr()), out.shape[0],
                                       self._stream()))
        return out[:n]

    def num_rows(self):
        """Every table row: num_agents() plus the shard ghost's rows (which
        follow row N; see write_actions)."""
        v = ctypes.c_uint32()
        _check(_lib.mbots_num_rows(self._h, ctypes.byref(v)))
        return v.value

    def learner_record_bytes(self, slim=False):
        """Bytes per learner record (include/mbots.h: 272, or 336 with real
        depth; slim records 128 / 192)."""
        if slim:
            return LEARNER_SLIM_BYTES_DEPTH if self._fix_depth else LEARNER_SLIM_BYTES
        v = ctypes.c_uint32()
        _check(_lib.mbots_learner_record_bytes(self._h, ctypes.byref(v)))
        return v.value

    def pack_learner(self, out=None, slim=False):
        """Everything the reference training loop reads after step() --
        current and previous observation columns, reward, stats, Action,
        HiddenState, PrevHiddenState (learn/training_loop.py:43-93) -- as one
        uint8 [N, learner_record_bytes()] record per export row: the payload of
        the config-5 gather (harness/gather.py); unpack_learner() rebuilds the
        learner's tensors.  `out` may hold more rows (padding).  slim=True:
        the 128-B records without Action / HiddenState / PrevHiddenState but
        with each row's provenance (include/mbots.h MBOTS_LEARNER_SLIM_BYTES),
        for a learner that rebuilds those from its own writes."""
        n = self.num_agents()
        rb = self.learner_record_bytes(slim)
        if out is None:
            out = torch.empty((n, rb), dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or out.device != self.device or not out.is_contiguous() \
                or out.dim() != 2 or out.shape[1] != rb or out.shape[0] < n:
            raise ValueError(f"out must be a contiguous uint8 [>= {n}, {rb}] tensor on {self.device}")
        fn = _lib.mbots_pack_learner_slim if slim else _lib.mbots_pack_learner
        _check(fn(self._h, ctypes.c_void_p(out.data_ptr()), out.shape[0], self._stream()))
        return out[:n]

    def write_actions(self, actions=None, memory=None):
        """The learner's writes for every row at once (training_loop.py:136-137:
        action_tensor[...] = one_hot; memory_tensor[...] = new_memory):
        int32 [R, 6] actions and/or float32 [R, 16] memory, R = num_agents() or
        num_rows() (the latter also drives the shard ghost's agents, which then
        act exactly as the next rank's first world does) -- mbots_write_actions."""
        def arg(t, cols, dtype):
            if t is None:
                return None, None
            if t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols or t.device != self.device:
                raise ValueError(f"expected {dtype} [rows, {cols}] on {self.device}")
            t = t.contiguous()
            return t, t.shape[0]
        a, ra = arg(actions, 6, torch.int32)
        m, rm = arg(memory, 16, torch.float32)
        rows = ra if ra is not None else rm
        if rows is None:
            return
        if ra is not None and rm is not None and ra != rm:
            raise ValueError("actions and memory must have the same rows")
        _check(_lib.mbots_write_actions(self._h, ctypes.c_void_p(a.data_ptr() if a is not None else None),
                                        ctypes.c_void_p(m.data_ptr() if m is not None else None), rows,
                                        self._stream()))

    # -- acting on the device -------------------------------------------------
    @property
    def policy_groups(self):
        """The policy groups' starts (set_policy_groups); [0]: one group."""
        n = ctypes.c_uint32()
        starts = (ctypes.c_uint32 * 64)()
        _check(_lib.mbots_policy_num_groups(self._h, ctypes.byref(n), starts))
        return list(starts[:n.value])

    def set_policy_groups(self, starts=None):
        """Policy groups: `starts`, 1..64 ascending global world indices with
        starts[0] == 0; group g owns the worlds [starts[g], starts[g + 1]) (the
        last every world from its start on) and acts through four nets of its
        own (set_policy(..., group=g)), all in the one launch of act().  The
        indices are global, so the shards of one run take the same starts.  New
        starts wait for the device and remove every net; the starts in place
        change nothing; None or []: back to one group (mbots_policy_groups)."""
        starts = [int(v) for v in starts] if starts is not None and len(starts) else [0]
        if any(not 0 <= v < 2 ** 32 for v in starts):
            raise ValueError("policy group starts are world indices in [0, 2^32)")
        if starts == self.policy_groups:
            return
        if self.exec_mode == ExecMode.HIP and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("madrona_bots: policy groups cannot be changed during a graph capture")
        arr = (ctypes.c_uint32 * max(len(starts), 1))(*starts)
        _check(_lib.mbots_policy_groups(self._h, arr, len(starts)))
        self._policy = [[None] * 4 for _ in starts]

    def policy_segments(self, out=None):
        """int32 [G, 4, 2] on `device`: the rows [lo, hi) of every (group,
        species) among the N exported rows of the current table -- rows are
        ordered (species, world, slot), so each is one contiguous range, lo ==
        hi where a group has no such row.  Stream-ordered, no host wait,
        capturable (mbots_policy_segments); one .tolist() gives a learner the
        slices of every flat [N, ...] tensor."""
        G = len(self._policy)
        if out is None:
            out = torch.empty((G, 4, 2), dtype=torch.int32, device=self.device)
        if out.dtype != torch.int32 or out.device != self.device or not out.is_contiguous() \
                or tuple(out.shape) != (G, 4, 2):
            raise ValueError(f"out must be a contiguous int32 [{G}, 4, 2] tensor on {self.device}")
        _check(_lib.mbots_policy_segments(self._h, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def _set_policy_one(self, species, net, group=None):
        dev = self.device

        def layer(spec):
            w, b, act = spec
            w = w.detach().to(device=dev, dtype=torch.float32).contiguous()
            b = None if b is None else b.detach().to(device=dev, dtype=torch.float32).contiguous()
            keep.extend((w, b))
            return _PolicyLayer(w.shape[1], w.shape[0], act, w.data_ptr(), None if b is None else b.data_ptr())

        keep = []
        c = _PolicyNet()
        c.n_trunk = len(net.trunk)
        for i, spec in enumerate(net.trunk):
            c.trunk[i] = layer(spec)
        for i in range(2):
            c.actor[i] = layer(net.actor[i])
            c.critic[i] = layer(net.critic[i])
        if net.memory is not None:
            c.memory = layer(net.memory)
        c.flags = 1 if net.memory_in else 0
        if net.gate is not None:
            c.gate = layer(net.gate)
            c.flags |= 2   # MBOTS_POLICY_GATE
        # (the upload reads the tensors in stream order on torch's current
        # stream, where the caching allocator also orders their release)
        if group is None:
            _check(_lib.mbots_policy_set(self._h, int(species), ctypes.byref(c), self._stream()))
        else:
            _check(_lib.mbots_policy_set_group(self._h, int(group), int(species), ctypes.byref(c), self._stream()))
        for g in (range(len(self._policy)) if group is None else [int(group)]):
            self._policy[g][species - 1] = net

    def _check_group(self, group):
        if group is not None and not 0 <= int(group) < len(self._policy):
            raise ValueError(f"policy group {group} out of range: the manager has {len(self._policy)} "
                             "(set_policy_groups)")

    def set_policy(self, net, species=None, group=None):
        """Give species 1..4 their policy nets (PolicyNet): one net for every
        species, a list of four, or one net for `species`.  The first call, or
        a net of another architecture, allocates; calling again with the same
        architecture -- after every optimiser step -- only re-uploads the
        weights, stream-ordered on torch's current stream (mbots_policy_set).
        group: the policy group (set_policy_groups) the nets are for; None:
        every group."""
        self._check_group(group)
        if species is not None:
            if isinstance(net, (list, tuple)):
                raise ValueError("one PolicyNet for one species")
            nets = {int(species): net}
        elif isinstance(net, (list, tuple)):
            if len(net) != 4:
                raise ValueError("a list of policy nets holds one per species (4)")
            nets = {i + 1: n for i, n in enumerate(net)}
        else:
            nets = {i + 1: net for i in range(4)}
        for sp, n in nets.items():
            if not isinstance(n, PolicyNet):
                raise TypeError("set_policy takes PolicyNet objects (PolicyNet.from_torch)")
            if not 1 <= sp <= 4:
                raise ValueError("species must be 1..4")
        for sp, n in nets.items():
            self._set_policy_one(sp, n, group)

    def clear_policy(self, species=None, group=None):
        self._check_group(group)
        for sp in ([int(species)] if species is not None else [1, 2, 3, 4]):
            if group is None:
                _check(_lib.mbots_policy_clear(self._h, sp))
            else:
                _check(_lib.mbots_policy_clear_group(self._h, int(group), sp))
            for g in (range(len(self._policy)) if group is None else [int(group)]):
                self._policy[g][sp - 1] = None

    def act(self, greedy=False, write=True, out=None):
        """One stream-ordered call for policy(construct_obs()) -> sample ->
        write_actions(): every table row (the shard ghost's too) runs the net
        of its species (with policy groups: of its world's group), an action is sampled from the manager's counter RNG
        (greedy: the first maximal logit), and -- unless write=False -- Action
        receives the one-hot and HiddenState the memory head's output.  Returns
        {"action": int32 [N, 1], "logp": float32 [N, 1], "value": float32
        [N, 1]} on `device` for the N exported rows.  `out`: a dict of such
        tensors with at least N rows to write into (required while the stream
        is being captured into a graph, where N is not known to the host; the
        tensors are then returned whole)."""
        capturing = self.exec_mode == ExecMode.HIP and torch.cuda.is_current_stream_capturing()
        if out is None:
            if capturing:
                raise ValueError("act() under graph capture needs out= (the row count is not known to the host)")
            n = self.num_agents()
            out = {"action": torch.empty((n, 1), dtype=torch.int32, device=self.device),
                   "logp": torch.empty((n, 1), dtype=torch.float32, device=self.device),
                   "value": torch.empty((n, 1), dtype=torch.float32, device=self.device)}
            rows = n
        else:
            rows = None
            for k, dt in (("action", torch.int32), ("logp", torch.float32), ("value", torch.float32)):
                t = out.get(k)
                if t is None:
                    continue
                if t.dtype != dt or t.device != self.device or not t.is_contiguous() or t.dim() != 2 \
                        or t.shape[1] != 1 or (rows is not None and t.shape[0] != rows):
                    raise ValueError(f"out[{k!r}] must be a contiguous {dt} [rows, 1] tensor on {self.device}, "
                                     "all of the same rows")
                rows = t.shape[0]
            n = None if capturing else self.num_agents()
            if rows is not None and n is not None and rows < n:
                raise ValueError(f"out tensors must hold at least {n} rows")

        def ptr(k):
            t = out.get(k)
            return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None)
        flags = (1 if greedy else 0) | (0 if write else 2)
        _check(_lib.mbots_policy_act(self._h, flags, ptr("action"), ptr("logp"), ptr("value"), rows or 0,
                                     self._stream()))
        if n is None:
            return out
        return {k: (t[:n] if t is not None else None) for k, t in out.items()}

    @property
    def policy_draw(self):
        """The draw counter of act(): read by every act() and advanced by one
        after it (so a replayed graph draws fresh numbers); set it back to
        reproduce a rollout.  Not part of a checkpoint."""
        v = ctypes.c_uint32()
        _check(_lib.mbots_policy_draw(self._h, 0, ctypes.byref(v)))
        return v.value

    @policy_draw.setter
    def policy_draw(self, value):
        v = ctypes.c_uint32(int(value) & 0xFFFFFFFF)
        _check(_lib.mbots_policy_draw(self._h, 1, ctypes.byref(v)))

    def save_checkpoint(self, path=None):
        """Live simulator state as bytes (and to `path` if given); see
        load_checkpoint.  Not in the reference."""
        import numpy as np
        n = ctypes.c_uint64()
        _check(_lib.mbots_checkpoint_size(self._h, ctypes.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        _check(_lib.mbots_save_checkpoint(self._h, ctypes.c_void_p(buf.ctypes.data), n.value))
        if path is not None:
            buf.tofile(path)
        return buf

    def load_checkpoint(self, src):
        """Restore a checkpoint (bytes/array or a file path) saved by a manager
        of the same configuration; the next step continues bit-exactly."""
        import numpy as np
        buf = np.fromfile(src, dtype=np.uint8) if isinstance(src, (str, os.PathLike)) \
            else np.ascontiguousarray(np.frombuffer(src, dtype=np.uint8))
        _check(_lib.mbots_load_checkpoint(self._h, ctypes.c_void_p(buf.ctypes.data), buf.size))

    def world_state(self, world_idx):
        """Debug dump of one world (replacing the viewer's
        state readback): live agents' position, rotation (w, z), species,
        health, finder slot, and the live food packages (chunk, x, y, rotation as
        a 22-bit quarter-turn fraction),
        as numpy arrays (save with numpy.savez)."""
        import numpy as np
        cap = self.agent_capacity
        xyr = np.zeros((cap, 4), np.float32)
        shf = np.zeros((cap, 3), np.int32)
        food = np.zeros(48, np.uint64)
        rot = np.zeros((5, 48), np.uint32)
        n = ctypes.c_int32()
        _check(_lib.mbots_world_state(self._h, int(world_idx), ctypes.c_void_p(xyr.ctypes.data),
                                      ctypes.c_void_p(shf.ctypes.data),
                                      ctypes.c_void_p(food.ctypes.data),
                                      ctypes.c_void_p(rot.ctypes.data), ctypes.byref(n)))
        k = n.value
        pk = []
        for c, rec in enumerate(food.tolist()):
            for q in range(5):
                if (rec >> (40 + q)) & 1:
                    xy = (rec >> (8 * q)) & 0xFF
                    pk.append((c, (c % 8) * 16 + (xy & 15), (c // 8) * 16 + (xy >> 4),
                               int(rot[q, c])))
        return {"position": xyr[:k, :2].copy(), "rotation_wz": xyr[:k, 2:].copy(),
                "species": shf[:k, 0].copy(), "health": shf[:k, 1].copy(),
                "finder": shf[:k, 2].copy(),
                "food": np.array(pk, np.int32).reshape(-1, 4)}

    def set_world_state(self, world_idx, position, rotation_wz, food):
        """Debug / test entry point, the inverse of world_state() for geometry
        (mbots_set_world_state): write the live agents' position [n, 2] and
        rotation (w, z) [n, 2] and replace the world's food by the packages
        [k, 4] of (chunk, x, y, rotation).  Population, species, health, finder
        slots, RNG and the exported table stay; a scene the simulator could
        not reach by its own steps raises RuntimeError and changes nothing.
        In HIP mode the call is a checkpoint round trip."""
        import numpy as np
        xyr = np.ascontiguousarray(np.concatenate(
            [np.asarray(position, np.float32).reshape(-1, 2),
             np.asarray(rotation_wz, np.float32).reshape(-1, 2)], axis=1))
        fd = np.ascontiguousarray(np.asarray(food, np.int32).reshape(-1, 4))
        _check(_lib.mbots_set_world_state(self._h, int(world_idx), ctypes.c_void_p(xyr.ctypes.data),
                                          len(xyr), ctypes.c_void_p(fd.ctypes.data), len(fd)))

    def render_worlds(self, worlds=None, scale=4, *, rgb=True, cls=False, slot=False, out=None):
        """Top-down images of `worlds` (local indices, any order, duplicates
        allowed; None: every exported world) as they stand in stream order
        (mbots_render_worlds; one kernel launch, no host synchronisation with
        the step): a dict of tensors on the manager's device with the keys
        asked for -- "rgb" uint8 [k, H, W, 3], "cls" uint8 [k, H, W] (CLS_*),
        "slot" int16 [k, H, W] (the agent slot of world_state(), -1 none) --
        H = 96 scale, W = 128 scale, scale in RENDER_SCALES, row 0 at y ~ 0.
        `out`: a dict of contiguous tensors of those shapes to write into
        (its keys select the outputs).  Scales 1 and 2 show no wall (the point
        samples do not reach it); a critic's map is cls at scale 1."""
        import numpy as np
        scale = int(scale)
        if worlds is None:
            k, wptr, w = self.num_worlds, None, None
        else:
            if isinstance(worlds, torch.Tensor):
                worlds = worlds.detach().cpu().numpy()
            w = np.asarray(list(worlds) if not isinstance(worlds, np.ndarray) else worlds).reshape(-1)
            if w.size and (w.min() < 0 or w.max() >= 2 ** 32):
                raise ValueError("madrona_bots: world index out of range")
            w = np.ascontiguousarray(w, dtype=np.uint32)
            k, wptr = int(w.size), (w.ctypes.data if w.size else None)
        H, W = RENDER_H * scale, RENDER_W * scale
        spec = {"rgb": ((k, H, W, 3), torch.uint8), "cls": ((k, H, W), torch.uint8),
                "slot": ((k, H, W), torch.int16)}
        if out is None:
            if scale not in RENDER_SCALES:
                raise RuntimeError(f"madrona_bots: scale {scale} is not one of {RENDER_SCALES}")
            want = [key for key, on in (("rgb", rgb), ("cls", cls), ("slot", slot)) if on]
            out = {key: torch.empty(spec[key][0], dtype=spec[key][1], device=self.device) for key in want}
        else:
            for key, t in out.items():
                if key not in spec:
                    raise ValueError(f"out: unknown key {key!r}")
                if t.dtype != spec[key][1] or tuple(t.shape) != spec[key][0] or t.device != self.device \
                        or not t.is_contiguous():
                    raise ValueError(f"out[{key!r}] must be a contiguous {spec[key][1]} {spec[key][0]} tensor "
                                     f"on {self.device}")
        ro = _RenderOut(**{key: (out[key].data_ptr() if key in out and out[key].numel() else None)
                           for key in ("cls", "slot", "rgb")})
        if k == 0 and out:
            return out
        _check(_lib.mbots_render_worlds(self._h, ctypes.c_void_p(wptr), k, scale, ctypes.byref(ro),
                                        self._stream()))
        return out

    def dump_worlds(self, path, worlds):
        """Write world_state() of each world in `worlds` to one .npz
        (keys "w<idx>/<field>") for offline inspection -- the build's
        replacement for the reference viewer's readback (src/gfx)."""
        import numpy as np
        arrays = {}
        for w in worlds:
            for k, v in self.world_state(w).items():
                arrays[f"w{int(w)}/{k}"] = v
        np.savez(path, **arrays)
        return sorted(arrays)

    def load_worlds(self, path):
        """Write the worlds of a dump_worlds() file back (set_world_state)."""
        import numpy as np
        z = np.load(path)
        for w in sorted({int(k.split("/")[0][1:]) for k in z.files}):
            self.set_world_state(w, z[f"w{w}/position"], z[f"w{w}/rotation_wz"], z[f"w{w}/food"])

    def join(self):
        """Make torch's current stream wait for the manager's outstanding
        sensor work (mbots_join): ends a sequence of steps captured into a
        HIP graph (torch.cuda.graph) with no unjoined work."""
        _check(_lib.mbots_join(self._h, self._stream()))

    def record_sensor_done(self, event):
        """Record a timing-enabled torch.cuda.Event on the manager's internal
        stream after the last step's sensor (mbots_record_sensor_done): a
        benchmark timing point that adds no wait to any stream."""
        if not event.cuda_event:   # torch creates its events on first record
            event.record()
        _check(_lib.mbots_record_sensor_done(self._h, ctypes.c_void_p(event.cuda_event)))

    def write_synthetic_actions(self, seed, step, write_hidden=False):
        _check(_lib.mbots_write_synthetic_actions(self._h, int(seed) & 0xFFFFFFFF,
                                                  int(step) & 0xFFFFFFFF,
                                                  1 if write_hidden else 0, self._stream()))

    def agent_steps(self):
        v = ctypes.c_uint64()
        _check(_lib.mbots_agent_steps(self._h, ctypes.byref(v)))
        return v.value

    def overflow(self):
        v = ctypes.c_uint64()
        _check(_lib.mbots_overflow(self._h, ctypes.byref(v)))
        return v.value

    def enable_kernel_timing(self, enable=True):
        self._ktiming = bool(enable)
        _check(_lib.mbots_enable_kernel_timing(self._h, 1 if enable else 0))

    def schedule_info(self):
        """The step schedule in use (mbots_schedule_info): {"k1_finder",
        "fork_by_value", "join_by_value", "swap", "mixed_classes", "episodes_armed",
        "hidden_lazy" (HiddenState is owed as a row map right now),
        "prev_action_lazy" (PrevAction is owed: the last shift launched no gather): bool,
        "epoch", "epoch_wraps", "steps": int}."""
        v = (ctypes.c_uint32 * 4)()
        _check(_lib.mbots_schedule_info(self._h, v))
        f = v[0]
        return {"k1_finder": bool(f & 1), "fork_by_value": bool(f & 2), "join_by_value": bool(f & 4),
                "swap": bool(f & 8), "mixed_classes": bool(f & 16), "episodes_armed": bool(f & 32),
                "hidden_lazy": bool(f & 64), "prev_action_lazy": bool(f & 128),
                "epoch": int(v[1]),
                "epoch_wraps": int(v[2]), "steps": int(v[3])}

    def kernel_times(self):
        """{kernel: (total_ms, launches)} since enable_kernel_timing()."""
        ms = (ctypes.c_double * len(KERNELS))()
        n = (ctypes.c_uint64 * len(KERNELS))()
        _check(_lib.mbots_kernel_times(self._h, ms, n))
        return {k: (ms[i], n[i]) for i, k in enumerate(KERNELS)}


# activation codes of the device actor (include/mbots.h; 6, 7 and 8: its own
# exp and log and the gate head's sigmoid, through policy_activation only)
ACTIVATIONS = {"Identity": 0, "ReLU": 1, "LeakyReLU": 2, "Tanh": 3, "ELU": 4, "LogSigmoid": 5, "exp": 6, "log": 7,
               "Sigmoid": 8}


def _activation_code(m, where):
    nn = torch.nn
    if isinstance(m, nn.ReLU):
        return 1
    if isinstance(m, nn.LeakyReLU):
        if m.negative_slope != 0.01:
            raise ValueError(f"{where}: LeakyReLU is supported with negative_slope 0.01 only, not {m.negative_slope}")
        return 2
    if isinstance(m, nn.Tanh):
        return 3
    if isinstance(m, nn.ELU):
        if m.alpha != 1.0:
            raise ValueError(f"{where}: ELU is supported with alpha 1 only, not {m.alpha}")
        return 4
    if isinstance(m, nn.LogSigmoid):
        return 5
    if isinstance(m, nn.Identity):
        return 0
    return None


class PolicyNet:
    """One species' net for SimManager.set_policy / act(): trunk, a list of
    (weight [out, in], bias [out] or None, activation code) for 1..4 Linear
    layers of one width H (a multiple of 16 in [16, 128]); actor and critic,
    two (weight, bias, 0) layers each -- Linear(H, H), ReLU, Linear(H, 6 / 1);
    memory, a (weight [16, H], bias, 0) Linear followed by Tanh whose output
    becomes HiddenState, or None; memory_in: the row's 16 HiddenState floats
    follow its 69 observation floats as the input; gate, a (weight [16, H],
    bias, 0) Linear followed by a sigmoid, or None: with it the new HiddenState
    is (1 - z) h + z c, z the gate's and c the memory head's output, h the
    state the row read (it needs memory and memory_in; DESIGN.md "Gated memory
    head").  The tensors are referenced, not copied: set_policy() uploads their
    values of that moment."""

    def __init__(self, trunk, actor, critic, memory=None, memory_in=False, gate=None):
        self.trunk, self.actor, self.critic = list(trunk), list(actor), list(critic)
        self.memory, self.memory_in, self.gate = memory, bool(memory_in), gate
        if gate is not None and (memory is None or not self.memory_in):
            raise ValueError("a gate needs a memory head and memory_in=True: it blends the memory head's output into "
                             "the HiddenState the net read")
        if not 1 <= len(self.trunk) <= 4:
            raise ValueError(f"a policy net has 1..4 trunk Linear layers, not {len(self.trunk)}")
        if len(self.actor) != 2 or len(self.critic) != 2:
            raise ValueError("actor and critic are Linear, ReLU, Linear")

    @staticmethod
    def _linears(seq, name):
        """[(weight, bias, code)] of a Sequential of Linear layers, each with at
        most one supported activation after it."""
        nn = torch.nn
        mods = list(seq) if isinstance(seq, nn.Sequential) else [seq]
        out = []
        for i, m in enumerate(mods):
            where = f"{name}[{i}] ({type(m).__name__})"
            if isinstance(m, nn.Linear):
                out.append([m.weight, m.bias, 0, False])
                continue
            code = _activation_code(m, where)
            if code is None:
                raise ValueError(f"{where}: only Linear, ReLU, LeakyReLU, Tanh, ELU, LogSigmoid and Identity are "
                                 "supported by the device actor")
            if not out or out[-1][3]:
                raise ValueError(f"{where}: an activation must follow a Linear layer, one at most")
            out[-1][2], out[-1][3] = code, True
        return [(w, b, c) for w, b, c, _ in out]

    @classmethod
    def from_torch(cls, feature, actor, critic, memory=None, memory_in=False, gate=None):
        """From nn.Sequential stacks of Linear plus {Tanh, ELU, LogSigmoid,
        LeakyReLU, ReLU}: the reference's a2c_nets.feature / .actor / .critic
        load unchanged (its recurrent module is not executed: see
        INTEGRATION.md).  memory: Sequential(Linear(H, 16), Tanh) or None; gate:
        Sequential(Linear(H, 16), Sigmoid) or None (with memory and memory_in)."""
        trunk = cls._linears(feature, "feature")
        heads = []
        for name, seq, width in (("actor", actor, 6), ("critic", critic, 1)):
            ls = cls._linears(seq, name)
            if len(ls) != 2 or ls[0][2] != 1 or ls[1][2] != 0:
                raise ValueError(f"{name}: expected Linear, ReLU, Linear (as the reference builds it)")
            if ls[1][0].shape[0] != width:
                raise ValueError(f"{name}: the last Linear must have {width} outputs, not {ls[1][0].shape[0]}")
            heads.append([(w, b, 0) for w, b, _ in ls])
        mem = None
        if memory is not None:
            ls = cls._linears(memory, "memory")
            if len(ls) != 1 or ls[0][2] != 3 or ls[0][0].shape[0] != 16:
                raise ValueError("memory: expected Linear(H, 16), Tanh")
            mem = (ls[0][0], ls[0][1], 0)
        gat = None
        if gate is not None:
            mods = list(gate) if isinstance(gate, torch.nn.Sequential) else [gate]
            if len(mods) != 2 or not isinstance(mods[0], torch.nn.Linear) or not isinstance(mods[1], torch.nn.Sigmoid):
                bad = next((f"gate[{i}] ({type(m).__name__})" for i, m in enumerate(mods)
                            if not isinstance(m, (torch.nn.Linear, torch.nn.Sigmoid) if i else torch.nn.Linear)),
                           f"gate ({len(mods)} modules)")
                raise ValueError(f"{bad}: expected Linear(H, 16), Sigmoid")
            if mods[0].weight.shape[0] != 16:
                raise ValueError(f"gate[0] (Linear): expected Linear(H, 16), not {mods[0].weight.shape[0]} outputs")
            gat = (mods[0].weight, mods[0].bias, 0)
        net = cls(trunk, heads[0], heads[1], mem, memory_in, gat)
        net._validate()
        return net

    def _validate(self):
        H = self.trunk[0][0].shape[0]
        if H % 16 or not 16 <= H <= 128:
            raise ValueError(f"feature[0] (Linear): the trunk width must be a multiple of 16 in [16, 128], not {H}")
        want = 85 if self.memory_in else 69
        for i, (w, _, _) in enumerate(self.trunk):
            if tuple(w.shape) != (H, want):
                raise ValueError(f"feature Linear {i}: expected weight [{H}, {want}], not {list(w.shape)}")
            want = H
        for name, head, width in (("actor", self.actor, 6), ("critic", self.critic, 1)):
            if tuple(head[0][0].shape) != (H, H) or tuple(head[1][0].shape) != (width, H):
                raise ValueError(f"{name}: expected Linear({H}, {H}), ReLU, Linear({H}, {width})")
        if self.memory is not None and tuple(self.memory[0].shape) != (16, H):
            raise ValueError(f"memory: expected Linear({H}, 16)")
        if self.gate is not None and tuple(self.gate[0].shape) != (16, H):
            raise ValueError(f"gate: expected Linear({H}, 16), not {list(self.gate[0].shape)}")

    def _seq_params(self):
        """_named_params() and what evaluate_sequences adds: the memory head's,
        then a gated net's gate head's."""
        out = self._named_params() + [("memory Linear weight", self.memory[0]), ("memory Linear bias", self.memory[1])]
        if self.gate is not None:
            out += [("gate Linear weight", self.gate[0]), ("gate Linear bias", self.gate[1])]
        return out

    # -- learning from what act() did -----------------------------------------
    def _named_params(self):
        """[(name, tensor or None)]: weight and bias of every layer evaluate()
        runs, in the order trunk, actor, critic (the memory head takes no part)."""
        out = []
        for name, layers in (("feature", self.trunk), ("actor", self.actor), ("critic", self.critic)):
            for i, (w, b, _) in enumerate(layers):
                out += [(f"{name} Linear {i} weight", w), (f"{name} Linear {i} bias", b)]
        return out

    def _c_net(self, params):
        """struct mbots_policy_net over `params` (the tensors of _named_params())."""
        c = _PolicyNet()
        c.n_trunk = len(self.trunk)
        codes = [code for _, _, code in self.trunk] + [0, 0, 0, 0]
        slots = [c.trunk[i] for i in range(len(self.trunk))] + [c.actor[0], c.actor[1], c.critic[0], c.critic[1]]
        for i, slot in enumerate(slots):
            w, b = params[2 * i], params[2 * i + 1]
            slot.in_, slot.out, slot.act = w.shape[1], w.shape[0], codes[i]
            slot.weight, slot.bias = w.data_ptr(), None if b is None else b.data_ptr()
        if len(params) > 2 * len(slots):   # evaluate_sequences: the memory head follows
            w, b = params[2 * len(slots)], params[2 * len(slots) + 1]
            c.memory.in_, c.memory.out, c.memory.act = w.shape[1], w.shape[0], 0
            c.memory.weight, c.memory.bias = w.data_ptr(), None if b is None else b.data_ptr()
        c.flags = 1 if self.memory_in else 0
        if len(params) > 2 * len(slots) + 2:   # a gated net's gate head after it
            w, b = params[2 * len(slots) + 2], params[2 * len(slots) + 3]
            c.gate.in_, c.gate.out, c.gate.act = w.shape[1], w.shape[0], 0
            c.gate.weight, c.gate.bias = w.data_ptr(), None if b is None else b.data_ptr()
            c.flags |= 2   # MBOTS_POLICY_GATE
        return c

    def evaluate(self, obs, action, hidden=None):
        """(logp, value, entropy), float32 [n] each on obs's device, of the
        recorded rows: obs float32 [n, 69] (construct_obs()), action int32
        [n] or [n, 1] (act()'s), hidden float32 [n, 16] for a memory_in net.
        logp and value are bit for bit what act() returned for these rows;
        the result is differentiable with respect to the net's parameters
        (the tensors this PolicyNet references: backward() leaves their .grad
        for any torch optimiser, set_policy() uploads the stepped weights),
        not to obs or hidden.  CUDA tensors run the HIP kernels, CPU tensors
        the host threads; both give the same bits, whatever the grid or the
        thread count (DESIGN.md "Differentiable evaluate")."""
        self._validate()
        dev = obs.device
        if obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[1] != 69:
            raise ValueError(f"obs must be float32 [n, 69], not {obs.dtype} {list(obs.shape)}")
        n = obs.shape[0]
        if action.dtype != torch.int32 or action.device != dev or action.numel() != n \
                or action.dim() not in (1, 2) or action.shape[0] != n:
            raise ValueError(f"action must be int32 [n] or [n, 1] on {dev} with obs's rows, not {action.dtype} "
                             f"{list(action.shape)} on {action.device}")
        if self.memory_in:
            if hidden is None:
                raise ValueError("a memory_in net needs hidden (float32 [n, 16])")
            if hidden.dtype != torch.float32 or hidden.device != dev or tuple(hidden.shape) != (n, 16):
                raise ValueError(f"hidden must be float32 [n, 16] on {dev}, not {hidden.dtype} {list(hidden.shape)} "
                                 f"on {hidden.device}")
            hidden = hidden.detach().contiguous()
        else:
            hidden = None
        named = self._named_params()
        for name, p in named:
            if p is not None and (p.dtype != torch.float32 or p.device != dev):
                raise ValueError(f"{name} must be float32 on {dev} (obs's device), not {p.dtype} on {p.device}")
        present = [i for i, (_, p) in enumerate(named) if p is not None]
        return _Evaluate.apply(self, obs.detach().contiguous(), action.detach().reshape(n).contiguous(), hidden,
                               present, *[named[i][1] for i in present])


    def evaluate_sequences(self, obs, action, length, hidden0, return_hidden=False):
        """(logp, value, entropy), float32 [L, B] each on obs's device, of a
        padded batch of sequences (TrajectoryWindow.batch(), one species'
        columns): obs float32 [L, B, 69], action int32 [L, B] or [L, B, 1],
        length int32 [B] in [0, L], hidden0 float32 [B, 16].  Element (k, b)
        is present iff k < length[b]; absent elements are +0.  The net -- one
        with a memory head and memory_in; evaluate() is for the others -- runs
        along each sequence with the memory head's output carried from step to
        step, so on unchanged parameters logp, value and the carried state are
        bit for bit what act() produced along that lifeline.  backward()
        backpropagates through time into every parameter, the memory head's
        included; obs and hidden0 receive no gradient (the window boundary is
        detached).  return_hidden: a fourth result, the non-differentiable
        float32 [L, B, 16] state each present element was evaluated with.
        Devices, bits and summation order as evaluate() (DESIGN.md
        "Backpropagation through HiddenState")."""
        self._validate()
        if self.memory is None or not self.memory_in:
            raise ValueError("evaluate_sequences needs a net with a memory head and memory_in=True (there is no state "
                             "to carry otherwise): use evaluate()")
        dev = obs.device
        if obs.dtype != torch.float32 or obs.dim() != 3 or obs.shape[2] != 69:
            raise ValueError(f"obs must be float32 [L, B, 69], not {obs.dtype} {list(obs.shape)}")
        L, B = obs.shape[0], obs.shape[1]
        if action.dtype != torch.int32 or action.device != dev or tuple(action.shape) not in ((L, B), (L, B, 1)):
            raise ValueError(f"action must be int32 [L, B] or [L, B, 1] on {dev} with obs's steps and sequences, not "
                             f"{action.dtype} {list(action.shape)} on {action.device}")
        if length.dtype != torch.int32 or length.device != dev or tuple(length.shape) != (B,):
            raise ValueError(f"length must be int32 [B] on {dev}, not {length.dtype} {list(length.shape)} on "
                             f"{length.device}")
        if hidden0.dtype != torch.float32 or hidden0.device != dev or tuple(hidden0.shape) != (B, 16):
            raise ValueError(f"hidden0 must be float32 [B, 16] on {dev}, not {hidden0.dtype} {list(hidden0.shape)} on "
                             f"{hidden0.device}")
        named = self._seq_params()
        for name, p in named:
            if p is not None and (p.dtype != torch.float32 or p.device != dev):
                raise ValueError(f"{name} must be float32 on {dev} (obs's device), not {p.dtype} on {p.device}")
        present = [i for i, (_, p) in enumerate(named) if p is not None]
        out = _EvaluateSequences.apply(self, obs.detach().contiguous(), action.detach().reshape(L, B).contiguous(),
                                       length.detach().contiguous(), hidden0.detach().contiguous(), bool(return_hidden),
                                       present, *[named[i][1] for i in present])
        return out if return_hidden else out[:3]


_workspaces = {}   # (device, bytes) -> uint8 buffer: evaluate()'s scratch


def _eval_call(net, obs, hidden, action, params, fn, seq=False):
    """The workspace and the device / stream arguments for one of the
    handle-free calls; fn(c_net, workspace pointer, bytes, device index, stream).
    seq: obs is evaluate_sequences' [L, B, 69]."""
    dev = obs.device
    c = net._c_net(params)
    need = ctypes.c_uint64()
    if seq:
        _check(_lib.mbots_policy_seq_workspace(ctypes.byref(c), obs.shape[0], obs.shape[1], ctypes.byref(need)))
    else:
        _check(_lib.mbots_policy_grad_workspace(ctypes.byref(c), obs.shape[0], ctypes.byref(need)))
    key = (dev, need.value)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(max(need.value, 64), dtype=torch.uint8, device=dev)
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            _check(fn(c, ctypes.c_void_p(ws.data_ptr()), need.value, dev.index, ctypes.c_void_p(_raw_stream(dev.index))))
    else:
        _check(fn(c, ctypes.c_void_p(ws.data_ptr()), need.value, -1, None))


def _ptr(t):
    return ctypes.c_void_p(None if t is None or t.numel() == 0 else t.data_ptr())


class _Evaluate(torch.autograd.Function):
    """PolicyNet.evaluate: mbots_policy_eval forward, mbots_policy_grad backward."""

    @staticmethod
    def forward(ctx, net, obs, action, hidden, present, *params):
        full = [None] * (2 * (len(net.trunk) + 4))
        for i, p in zip(present, params):
            full[i] = p.detach().contiguous()
        n = obs.shape[0]
        logp, value, entropy = (torch.empty(n, dtype=torch.float32, device=obs.device) for _ in range(3))
        _eval_call(net, obs, hidden, action, full, lambda c, ws, nb, d, st: _lib.mbots_policy_eval(
            ctypes.byref(c), _ptr(obs), _ptr(hidden), _ptr(action), n, _ptr(logp), _ptr(value), _ptr(entropy), ws, nb,
            d, st))
        ctx.net, ctx.rows, ctx.present, ctx.full = net, (obs, action, hidden), present, full
        ctx.set_materialize_grads(False)   # an output the loss does not use: no g_* (zeros)
        return logp, value, entropy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logp, g_value, g_entropy):
        net, (obs, action, hidden), present, full = ctx.net, ctx.rows, ctx.present, ctx.full
        n = obs.shape[0]
        g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_logp, g_value, g_entropy)]
        grads = [None] * len(full)
        for k, i in enumerate(present):
            if ctx.needs_input_grad[5 + k]:
                grads[i] = torch.empty_like(full[i])
        out = _PolicyGrads()
        slots = [out.trunk[i] for i in range(len(net.trunk))] + [out.actor[0], out.actor[1], out.critic[0], out.critic[1]]
        for i, slot in enumerate(slots):
            slot.weight, slot.bias = _ptr(grads[2 * i]).value, _ptr(grads[2 * i + 1]).value
        _eval_call(net, obs, hidden, action, full, lambda c, ws, nb, d, st: _lib.mbots_policy_grad(
            ctypes.byref(c), _ptr(obs), _ptr(hidden), _ptr(action), n, _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
            ctypes.byref(out), ws, nb, d, st))
        return (None, None, None, None, None) + tuple(grads[i] for i in present)


class _EvaluateSequences(torch.autograd.Function):
    """PolicyNet.evaluate_sequences: mbots_policy_seq_eval forward,
    mbots_policy_seq_grad backward."""

    @staticmethod
    def forward(ctx, net, obs, action, length, hidden0, want_hidden, present, *params):
        full = [None] * (2 * (len(net.trunk) + (5 if net.gate is None else 6)))
        for i, p in zip(present, params):
            full[i] = p.detach().contiguous()
        L, B = obs.shape[0], obs.shape[1]
        logp, value, entropy = (torch.empty(L, B, dtype=torch.float32, device=obs.device) for _ in range(3))
        hidden = torch.empty(L, B, 16, dtype=torch.float32, device=obs.device) if want_hidden else None
        _eval_call(net, obs, None, None, full, lambda c, ws, nb, d, st: _lib.mbots_policy_seq_eval(
            ctypes.byref(c), _ptr(obs), _ptr(action), _ptr(length), _ptr(hidden0), L, B, _ptr(logp), _ptr(value),
            _ptr(entropy), _ptr(hidden), ws, nb, d, st), seq=True)
        ctx.net, ctx.rows, ctx.present, ctx.full = net, (obs, action, length, hidden0), present, full
        ctx.set_materialize_grads(False)
        if hidden is None:
            hidden = torch.empty(0, dtype=torch.float32, device=obs.device)
        ctx.mark_non_differentiable(hidden)
        return logp, value, entropy, hidden

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logp, g_value, g_entropy, _g_hidden):
        net, (obs, action, length, hidden0), present, full = ctx.net, ctx.rows, ctx.present, ctx.full
        L, B = obs.shape[0], obs.shape[1]
        g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_logp, g_value, g_entropy)]
        grads = [None] * len(full)
        for k, i in enumerate(present):
            if ctx.needs_input_grad[7 + k]:
                grads[i] = torch.empty_like(full[i])
        out = _PolicyGrads()
        slots = [out.trunk[i] for i in range(len(net.trunk))] + [out.actor[0], out.actor[1], out.critic[0], out.critic[1],
                                                                 out.memory] + ([] if net.gate is None else [out.gate])
        for i, slot in enumerate(slots):
            slot.weight, slot.bias = _ptr(grads[2 * i]).value, _ptr(grads[2 * i + 1]).value
        _eval_call(net, obs, None, None, full, lambda c, ws, nb, d, st: _lib.mbots_policy_seq_grad(
            ctypes.byref(c), _ptr(obs), _ptr(action), _ptr(length), _ptr(hidden0), L, B, _ptr(g[0]), _ptr(g[1]),
            _ptr(g[2]), ctypes.byref(out), ws, nb, d, st), seq=True)
        return (None,) * 7 + tuple(grads[i] for i in present)


def _species_name(g, s):
    return f"nets[{g}][{s}] (group {g}, species {s + 1})"


def evaluate_groups(nets, obs, action, segments, hidden=None):
    """(logp, value, entropy), float32 [n] each on obs's device: every (group,
    species) segment of a table through its own net, in one forward call and
    one backward call (the learner's half of policy groups; DESIGN.md "Grouped
    evaluate").  nets: a list of 1..64 groups, each a list of four PolicyNet
    (species 1..4) or one PolicyNet for all four; None where a pair has no
    net; the nets may differ in every part of the architecture.  obs float32
    [n, 69], action int32 [n] or [n, 1], hidden float32 [n, 16] iff any net
    is memory_in; segments int32 [G, 4, 2] on obs's device, exactly what
    SimManager.policy_segments() returns: on a GPU it is read by the kernels
    only, never by the host.

    A row inside segment (g, s) gets, bit for bit, what
    nets[g][s].evaluate(obs[lo:hi], action[lo:hi], hidden[lo:hi]) gives it; a
    row in no segment, or in the segment of a None, gets +0 and takes no part
    in any gradient.  backward() leaves in every parameter that one net owns,
    bit for bit, the gradient the per-net call's backward leaves (sums in
    evaluate's order counted from the segment's lo; zeros for an empty
    segment).  A parameter tensor shared by several segments receives the sum
    of its segments' gradients, added by autograd in torch's order: the
    bitwise claim covers unshared parameters only.  obs and hidden receive no
    gradient; the memory head takes no part.

    segments must hold 0 <= lo <= hi <= n, pairwise disjoint: CPU tensors are
    checked (a violation names the pair); on a GPU hi is read as min(hi, n),
    lo as min(lo, hi), and disjointness is the caller's contract.  Forward
    and backward allocate no workspace after the first call of a shape and
    never wait for the host, so both can be recorded into a graph and
    replayed on other contents of `segments`."""
    groups = [list(g) if isinstance(g, (list, tuple)) else [g] * 4 for g in nets]
    G = len(groups)
    if not 1 <= G <= 64:
        raise ValueError(f"nets must hold 1..64 groups, not {G}")
    for g, four in enumerate(groups):
        if len(four) != 4 or any(x is not None and not isinstance(x, PolicyNet) for x in four):
            raise ValueError(f"nets[{g}] must be four PolicyNet (or None), or one PolicyNet for all species")
    dev = obs.device
    if obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[1] != 69:
        raise ValueError(f"obs must be float32 [n, 69], not {obs.dtype} {list(obs.shape)}")
    n = obs.shape[0]
    if action.dtype != torch.int32 or action.device != dev or action.numel() != n \
            or action.dim() not in (1, 2) or action.shape[0] != n:
        raise ValueError(f"action must be int32 [n] or [n, 1] on {dev} with obs's rows, not {action.dtype} "
                         f"{list(action.shape)} on {action.device}")
    if segments.dtype != torch.int32 or segments.device != dev or tuple(segments.shape) != (G, 4, 2):
        raise ValueError(f"segments must be int32 [{G}, 4, 2] on {dev} (policy_segments() of the nets' {G} groups), "
                         f"not {segments.dtype} {list(segments.shape)} on {segments.device}")
    flat = [x for four in groups for x in four]
    if any(x is not None and x.memory_in for x in flat):
        if hidden is None:
            raise ValueError("hidden (float32 [n, 16]) is needed: a net is memory_in")
        if hidden.dtype != torch.float32 or hidden.device != dev or tuple(hidden.shape) != (n, 16):
            raise ValueError(f"hidden must be float32 [n, 16] on {dev}, not {hidden.dtype} {list(hidden.shape)} "
                             f"on {hidden.device}")
        hidden = hidden.detach().contiguous()
    else:
        hidden = None
    index, params = [], []       # (segment, slot of _named_params) of every parameter passed on
    for e, x in enumerate(flat):
        if x is None:
            continue
        try:
            x._validate()
        except ValueError as err:
            raise ValueError(f"{_species_name(e // 4, e % 4)}: {err}") from None
        for i, (name, p) in enumerate(x._named_params()):
            if p is None:
                continue
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError(f"{_species_name(e // 4, e % 4)}: {name} must be float32 on {dev} (obs's device), "
                                 f"not {p.dtype} on {p.device}")
            index.append((e, i))
            params.append(p)
    return _EvaluateGroups.apply(flat, obs.detach().contiguous(), action.detach().reshape(n).contiguous(), hidden,
                                 segments.detach().contiguous(), index, *params)


def _groups_call(flat, full, obs, fn):
    """The C net table [G][4] over `full` (per segment the tensors of
    _named_params(), None: no net), the workspace, and the device / stream
    arguments; fn(nets, groups, workspace pointer, bytes, device index, stream)."""
    dev = obs.device
    c = (_PolicyNet * len(flat))()
    for e, x in enumerate(flat):
        if x is not None:
            c[e] = x._c_net(full[e])
    G = len(flat) // 4
    need = ctypes.c_uint64()
    _check(_lib.mbots_policy_groups_workspace(c, G, obs.shape[0], ctypes.byref(need)))
    key = (dev, need.value)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(max(need.value, 64), dtype=torch.uint8, device=dev)
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            _check(fn(c, G, ctypes.c_void_p(ws.data_ptr()), need.value, dev.index,
                      ctypes.c_void_p(_raw_stream(dev.index))))
    else:
        _check(fn(c, G, ctypes.c_void_p(ws.data_ptr()), need.value, -1, None))


class _EvaluateGroups(torch.autograd.Function):
    """evaluate_groups: mbots_policy_eval_groups forward, mbots_policy_grad_groups
    backward, one node over the parameters of every net."""

    @staticmethod
    def forward(ctx, flat, obs, action, hidden, segments, index, *params):
        full = [None if x is None else [None] * (2 * (len(x.trunk) + 4)) for x in flat]
        for (e, i), p in zip(index, params):
            full[e][i] = p.detach().contiguous()
        n = obs.shape[0]
        logp, value, entropy = (torch.empty(n, dtype=torch.float32, device=obs.device) for _ in range(3))
        _groups_call(flat, full, obs, lambda c, G, ws, nb, d, st: _lib.mbots_policy_eval_groups(
            c, G, _ptr(segments), _ptr(obs), _ptr(hidden), _ptr(action), n, _ptr(logp), _ptr(value), _ptr(entropy),
            ws, nb, d, st))
        ctx.flat, ctx.rows, ctx.index, ctx.full = flat, (obs, action, hidden, segments), index, full
        ctx.set_materialize_grads(False)   # an output the loss does not use: no g_* (zeros)
        return logp, value, entropy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logp, g_value, g_entropy):
        flat, (obs, action, hidden, segments), index, full = ctx.flat, ctx.rows, ctx.index, ctx.full
        n = obs.shape[0]
        g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_logp, g_value, g_entropy)]
        out = (_PolicyGrads * len(flat))()
        grads = []
        for k, (e, i) in enumerate(index):
            if not ctx.needs_input_grad[6 + k]:
                grads.append(None)
                continue
            grads.append(torch.empty_like(full[e][i]))
            T = len(flat[e].trunk)
            layer, slots = i // 2, out[e]
            slot = slots.trunk[layer] if layer < T else (slots.actor, slots.critic)[(layer - T) // 2][(layer - T) % 2]
            if i % 2:
                slot.bias = grads[-1].data_ptr()
            else:
                slot.weight = grads[-1].data_ptr()
        _groups_call(flat, full, obs, lambda c, G, ws, nb, d, st: _lib.mbots_policy_grad_groups(
            c, G, _ptr(segments), _ptr(obs), _ptr(hidden), _ptr(action), n, _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
            out, ws, nb, d, st))
        return (None,) * 6 + tuple(grads)


def sequence_segments(net_id, groups):
    """(order int32 [B], segments int32 [groups, 4, 2]) on net_id's device:
    the columns of a padded sequence batch sorted by their net, for
    evaluate_sequences_groups.  net_id int32 [B]: each column's group * 4 +
    (species - 1); anything outside [0, 4 * groups) means "no net".
    order[lo:hi] of pair (g, s) holds exactly the columns with net_id == 4 g +
    s, ascending (torch.nonzero(net_id == 4 g + s)); the segments lie in
    ascending 4 g + s from position 0, and order past the last one is -1.  On a
    GPU it is a stable counting sort in the library: no wait for the host,
    nothing allocated beyond its cached workspace, capturable; CPU tensors run
    on the host and give the same values."""
    groups = int(groups)
    if not 1 <= groups <= 64:
        raise ValueError(f"groups must be 1..64, not {groups}")
    if net_id.dtype != torch.int32 or net_id.dim() != 1:
        raise ValueError(f"net_id must be int32 [B], not {net_id.dtype} {list(net_id.shape)}")
    net_id = net_id.detach().contiguous()
    dev, B = net_id.device, net_id.shape[0]
    order = torch.empty(B, dtype=torch.int32, device=dev)
    segments = torch.empty(groups, 4, 2, dtype=torch.int32, device=dev)
    if dev.type == "cuda":
        need = (B + 1023) // 1024 * 1024 + 256   # MBOTS_POLICY_SEQ_ORDER_WORKSPACE(B)
        key = (dev, need)
        ws = _workspaces.get(key)
        if ws is None:
            ws = _workspaces[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _check(_lib.mbots_policy_seq_order(_ptr(net_id), B, groups, _ptr(order), _ptr(segments),
                                               ctypes.c_void_p(ws.data_ptr()), need, dev.index,
                                               ctypes.c_void_p(_raw_stream(dev.index))))
    else:
        _check(_lib.mbots_policy_seq_order(_ptr(net_id), B, groups, _ptr(order), _ptr(segments), None, 0, -1, None))
    return order, segments


def evaluate_sequences_groups(nets, obs, action, length, hidden0, order, segments, return_hidden=False):
    """(logp, value, entropy), float32 [L, B] each on obs's device: every
    (group, species) net along its own columns of one padded sequence batch,
    in one forward call and one backward call (the recurrent learner's half of
    policy groups; DESIGN.md "Grouped evaluate_sequences").  nets as
    evaluate_groups': 1..64 groups, each four PolicyNet or one for all four,
    None where a pair has no net; every net present needs a memory head and
    memory_in (evaluate_groups is for the others); they may differ in H, depth
    and activations.  obs float32 [L, B, 69], action int32 [L, B] or [L, B, 1],
    length int32 [B], hidden0 float32 [B, 16]: the whole batch as
    TrajectoryWindow.batch() / gather() hand it out, read in place.  order
    int32 [B] and segments int32 [G, 4, 2] are sequence_segments': position p
    of segment (g, s) stands for column order[p]; on a GPU both are read by the
    kernels only.

    Column order[p], lo <= p < hi of (g, s), gets bit for bit what
    nets[g][s].evaluate_sequences(obs.index_select(1, order[lo:hi]), ...) gives
    it; a column named by no evaluated segment, or by the segment of a None,
    gets +0 at every step and takes no part in any gradient.  backward() leaves
    a gradient in every parameter of every net, memory head included: for a net
    that owns its parameters bit for bit the per-net call's (sums in
    evaluate_sequences' order, counted in positions from lo; zeros for an empty
    segment); a tensor shared between segments receives autograd's sum.  obs
    and hidden0 receive none.  return_hidden: a fourth result, float32 [L, B,
    16], in the batch's own column layout like the others.

    Contract: 0 <= lo <= hi <= B, segments pairwise disjoint, every order[p] of
    an evaluated segment in [0, B), no column twice, length in [0, L], present
    actions in 0..5.  CPU tensors are checked (a violation names the pair); on
    a GPU bounds are clamped as in evaluate_groups, an order entry outside
    [0, B) is a column of length 0 that is neither read nor written, and
    duplicates and overlaps are the caller's contract.  After the first call of
    a shape forward and backward allocate no workspace and never wait for the
    host, so both can be captured; a replay reads order and segments as they
    are then."""
    groups = [list(g) if isinstance(g, (list, tuple)) else [g] * 4 for g in nets]
    G = len(groups)
    if not 1 <= G <= 64:
        raise ValueError(f"nets must hold 1..64 groups, not {G}")
    for g, four in enumerate(groups):
        if len(four) != 4 or any(x is not None and not isinstance(x, PolicyNet) for x in four):
            raise ValueError(f"nets[{g}] must be four PolicyNet (or None), or one PolicyNet for all species")
    dev = obs.device
    if obs.dtype != torch.float32 or obs.dim() != 3 or obs.shape[2] != 69:
        raise ValueError(f"obs must be float32 [L, B, 69], not {obs.dtype} {list(obs.shape)}")
    L, B = obs.shape[0], obs.shape[1]
    if action.dtype != torch.int32 or action.device != dev or tuple(action.shape) not in ((L, B), (L, B, 1)):
        raise ValueError(f"action must be int32 [L, B] or [L, B, 1] on {dev} with obs's steps and sequences, not "
                         f"{action.dtype} {list(action.shape)} on {action.device}")
    if length.dtype != torch.int32 or length.device != dev or tuple(length.shape) != (B,):
        raise ValueError(f"length must be int32 [B] on {dev}, not {length.dtype} {list(length.shape)} on "
                         f"{length.device}")
    if hidden0.dtype != torch.float32 or hidden0.device != dev or tuple(hidden0.shape) != (B, 16):
        raise ValueError(f"hidden0 must be float32 [B, 16] on {dev}, not {hidden0.dtype} {list(hidden0.shape)} on "
                         f"{hidden0.device}")
    if order.dtype != torch.int32 or order.device != dev or tuple(order.shape) != (B,):
        raise ValueError(f"order must be int32 [B] on {dev} (sequence_segments()), not {order.dtype} "
                         f"{list(order.shape)} on {order.device}")
    if segments.dtype != torch.int32 or segments.device != dev or tuple(segments.shape) != (G, 4, 2):
        raise ValueError(f"segments must be int32 [{G}, 4, 2] on {dev} (sequence_segments() of the nets' {G} groups), "
                         f"not {segments.dtype} {list(segments.shape)} on {segments.device}")
    flat = [x for four in groups for x in four]
    index, params = [], []       # (segment, slot of the net's parameters) of every parameter passed on
    for e, x in enumerate(flat):
        if x is None:
            continue
        where = _species_name(e // 4, e % 4)
        try:
            x._validate()
        except ValueError as err:
            raise ValueError(f"{where}: {err}") from None
        if x.memory is None or not x.memory_in:
            raise ValueError(f"{where}: evaluate_sequences_groups needs a net with a memory head and memory_in=True "
                             "(there is no state to carry otherwise): use evaluate_groups()")
        named = x._seq_params()
        for i, (name, p) in enumerate(named):
            if p is None:
                continue
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError(f"{where}: {name} must be float32 on {dev} (obs's device), not {p.dtype} on {p.device}")
            index.append((e, i))
            params.append(p)
    out = _EvaluateSequencesGroups.apply(flat, obs.detach().contiguous(), action.detach().reshape(L, B).contiguous(),
                                         length.detach().contiguous(), hidden0.detach().contiguous(),
                                         order.detach().contiguous(), segments.detach().contiguous(),
                                         bool(return_hidden), index, *params)
    return out if return_hidden else out[:3]


def _seq_groups_call(flat, full, obs, fn):
    """_groups_call for evaluate_sequences_groups: obs is [L, B, 69] and the
    workspace is mbots_policy_seq_groups_workspace's."""
    dev = obs.device
    c = (_PolicyNet * len(flat))()
    for e, x in enumerate(flat):
        if x is not None:
            c[e] = x._c_net(full[e])
    G = len(flat) // 4
    need = ctypes.c_uint64()
    _check(_lib.mbots_policy_seq_groups_workspace(c, G, obs.shape[0], obs.shape[1], ctypes.byref(need)))
    key = (dev, need.value)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(max(need.value, 64), dtype=torch.uint8, device=dev)
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            _check(fn(c, G, ctypes.c_void_p(ws.data_ptr()), need.value, dev.index,
                      ctypes.c_void_p(_raw_stream(dev.index))))
    else:
        _check(fn(c, G, ctypes.c_void_p(ws.data_ptr()), need.value, -1, None))


class _EvaluateSequencesGroups(torch.autograd.Function):
    """evaluate_sequences_groups: mbots_policy_seq_eval_groups forward,
    mbots_policy_seq_grad_groups backward, one node over the parameters of
    every net."""

    @staticmethod
    def forward(ctx, flat, obs, action, length, hidden0, order, segments, want_hidden, index, *params):
        full = [None if x is None else [None] * (2 * (len(x.trunk) + (5 if x.gate is None else 6))) for x in flat]
        for (e, i), p in zip(index, params):
            full[e][i] = p.detach().contiguous()
        L, B = obs.shape[0], obs.shape[1]
        logp, value, entropy = (torch.empty(L, B, dtype=torch.float32, device=obs.device) for _ in range(3))
        hidden = torch.empty(L, B, 16, dtype=torch.float32, device=obs.device) if want_hidden else None
        _seq_groups_call(flat, full, obs, lambda c, G, ws, nb, d, st: _lib.mbots_policy_seq_eval_groups(
            c, G, _ptr(order), _ptr(segments), _ptr(obs), _ptr(action), _ptr(length), _ptr(hidden0), L, B, _ptr(logp),
            _ptr(value), _ptr(entropy), _ptr(hidden), ws, nb, d, st))
        ctx.flat, ctx.rows, ctx.index, ctx.full = flat, (obs, action, length, hidden0, order, segments), index, full
        ctx.set_materialize_grads(False)
        if hidden is None:
            hidden = torch.empty(0, dtype=torch.float32, device=obs.device)
        ctx.mark_non_differentiable(hidden)
        return logp, value, entropy, hidden

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logp, g_value, g_entropy, _g_hidden):
        flat, (obs, action, length, hidden0, order, segments), index, full = ctx.flat, ctx.rows, ctx.index, ctx.full
        L, B = obs.shape[0], obs.shape[1]
        g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_logp, g_value, g_entropy)]
        out = (_PolicyGrads * len(flat))()
        grads = []
        for k, (e, i) in enumerate(index):
            if not ctx.needs_input_grad[9 + k]:
                grads.append(None)
                continue
            grads.append(torch.empty_like(full[e][i]))
            T = len(flat[e].trunk)
            layer, slots = i // 2, out[e]
            if layer < T:
                slot = slots.trunk[layer]
            elif layer < T + 4:
                slot = (slots.actor, slots.critic)[(layer - T) // 2][(layer - T) % 2]
            elif layer == T + 4:
                slot = slots.memory
            else:
                slot = slots.gate
            if i % 2:
                slot.bias = grads[-1].data_ptr()
            else:
                slot.weight = grads[-1].data_ptr()
        _seq_groups_call(flat, full, obs, lambda c, G, ws, nb, d, st: _lib.mbots_policy_seq_grad_groups(
            c, G, _ptr(order), _ptr(segments), _ptr(obs), _ptr(action), _ptr(length), _ptr(hidden0), L, B, _ptr(g[0]),
            _ptr(g[1]), _ptr(g[2]), out, ws, nb, d, st))
        return (None,) * 9 + tuple(grads)


def policy_activation(act, x):
    """The device actor's own activation (a name of ACTIVATIONS or its code)
    of a float32 tensor, on the tensor's device: what act() computes, bit for
    bit, in both execution modes (mbots_policy_activation)."""
    code = ACTIVATIONS[act] if isinstance(act, str) else int(act)
    x = x.contiguous()
    if x.dtype != torch.float32:
        raise ValueError("policy_activation takes float32")
    y = torch.empty_like(x)
    if x.is_cuda:
        with torch.cuda.device(x.device):
            _check(_lib.mbots_policy_activation(code, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                                x.numel(), x.device.index,
                                                ctypes.c_void_p(_raw_stream(x.device.index))))
    else:
        _check(_lib.mbots_policy_activation(code, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()),
                                            x.numel(), -1, None))
    return y


def _on_device(dev, fn):
    """fn(device index, stream) of a handle-free call on `dev`'s memory."""
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            _check(fn(dev.index, ctypes.c_void_p(_raw_stream(dev.index))))
    else:
        _check(fn(-1, None))


def policy_group_rows(segments, rows):
    """rows[g] += the rows of group g's four segments (mbots_policy_group_rows).
    segments int32 [G, 4, 2] as policy_segments() returns it, rows int64 [G] on
    the same device, zeroed by the caller and passed once per table of an
    update; returns rows.  On a GPU nothing is read by the host."""
    if segments.dtype != torch.int32 or segments.dim() != 3 or tuple(segments.shape[1:]) != (4, 2):
        raise ValueError(f"segments must be int32 [G, 4, 2], not {segments.dtype} {list(segments.shape)}")
    G = segments.shape[0]
    if rows.dtype != torch.int64 or tuple(rows.shape) != (G,) or rows.device != segments.device \
            or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous int64 [{G}] on {segments.device}, not {rows.dtype} "
                         f"{list(rows.shape)} on {rows.device}")
    segments = segments.detach().contiguous()
    _on_device(rows.device, lambda d, st: _lib.mbots_policy_group_rows(_ptr(segments), G, _ptr(rows), d, st))
    return rows


def a2c_loss_groups(logp, value, entropy, adv, ret, end, segments, rows, value_coef=0.5, entropy_coef=0.01, loss=None):
    """(g_logp, g_value, g_entropy, loss): the A2C loss of a table's recorded
    rows and its gradients with respect to evaluate's three outputs, in one
    pass of the library's own arithmetic (mbots_policy_a2c_loss; DESIGN.md
    "Device learner step").  logp, value, entropy: float32 [n], what
    evaluate_groups() (or evaluate()) returned, read detached; adv, ret: the
    window's columns of the table, float32 [n] or [n, 1]; end: its END column,
    int32 [n] or [n, 1], or None to keep every row; segments int32 [G, 4, 2];
    rows int64 [G], every group's row total over the whole update
    (policy_group_rows).  A row of group g weighs (end != END_RESET) / rows[g]:

        per_row = (-adv * logp + value_coef * (value - ret)**2 - entropy_coef * entropy) * weight

    and g_* are its derivatives; rows in no segment get +0.  loss: float64 [G],
    accumulated into (None: zeros); the sums run in a fixed order, so CPU and
    GPU tensors give the same bits.  Then

        torch.autograd.backward([logp, value, entropy], [g_logp, g_value, g_entropy])

    runs evaluate's backward.  Nothing waits for the host; capturable."""
    dev = logp.device
    n = logp.numel()
    G = segments.shape[0] if segments.dim() == 3 else 0
    if segments.dtype != torch.int32 or segments.device != dev or tuple(segments.shape) != (G, 4, 2) or not 1 <= G <= 64:
        raise ValueError(f"segments must be int32 [G, 4, 2] of 1..64 groups on {dev}, not {segments.dtype} "
                         f"{list(segments.shape)} on {segments.device}")
    cols = []
    for name, t in (("logp", logp), ("value", value), ("entropy", entropy), ("adv", adv), ("ret", ret)):
        if t.dtype != torch.float32 or t.device != dev or t.numel() != n or tuple(t.shape) not in ((n,), (n, 1)):
            raise ValueError(f"{name} must be float32 [n] or [n, 1] on {dev} with logp's {n} rows, not {t.dtype} "
                             f"{list(t.shape)} on {t.device}")
        cols.append(t.detach().reshape(n).contiguous())
    if end is not None:
        if end.dtype != torch.int32 or end.device != dev or tuple(end.shape) not in ((n,), (n, 1)):
            raise ValueError(f"end must be int32 [n] or [n, 1] on {dev}, not {end.dtype} {list(end.shape)} on "
                             f"{end.device}")
        end = end.detach().reshape(n).contiguous()
    if rows.dtype != torch.int64 or rows.device != dev or tuple(rows.shape) != (G,) or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous int64 [{G}] on {dev}, not {rows.dtype} {list(rows.shape)} on "
                         f"{rows.device}")
    if loss is None:
        loss = torch.zeros(G, dtype=torch.float64, device=dev)
    elif loss.dtype != torch.float64 or loss.device != dev or tuple(loss.shape) != (G,) or not loss.is_contiguous():
        raise ValueError(f"loss must be a contiguous float64 [{G}] on {dev}, not {loss.dtype} {list(loss.shape)} on "
                         f"{loss.device}")
    segments = segments.detach().contiguous()
    g = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)]
    _on_device(dev, lambda d, st: _lib.mbots_policy_a2c_loss(
        _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), _ptr(cols[4]), _ptr(end), n, _ptr(segments), G,
        _ptr(rows), value_coef, entropy_coef, _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(loss), d, st))
    return g[0], g[1], g[2], loss


def _sequence_columns(length, t0, end, order, segments, rows, dev):
    """The checked [B] columns, order and segments of the sequence loss calls:
    (B, G, length, t0, end, order, segments), contiguous."""
    G = segments.shape[0] if segments.dim() == 3 else 0
    if segments.dtype != torch.int32 or segments.device != dev or tuple(segments.shape) != (G, 4, 2) or not 1 <= G <= 64:
        raise ValueError(f"segments must be int32 [G, 4, 2] of 1..64 groups on {dev} (sequence_segments()), not "
                         f"{segments.dtype} {list(segments.shape)} on {segments.device}")
    B = length.numel()
    cols = []
    for name, t in (("length", length), ("t0", t0), ("end", end), ("order", order)):
        if t.dtype != torch.int32 or t.device != dev or tuple(t.shape) != (B,):
            raise ValueError(f"{name} must be int32 [{B}] on {dev}, not {t.dtype} {list(t.shape)} on {t.device}")
        cols.append(t.detach().contiguous())
    if rows.dtype != torch.int64 or rows.device != dev or tuple(rows.shape) != (G,) or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous int64 [{G}] on {dev}, not {rows.dtype} {list(rows.shape)} on "
                         f"{rows.device}")
    return (B, G, *cols, segments.detach().contiguous())


def sequence_group_rows(length, t0, end, order, segments, rows, last_table=-1):
    """rows[g] += the kept elements of the columns of group g's four segments
    (mbots_policy_seq_group_rows).  length, t0, end: int32 [B], the "len",
    "t0" and "end" columns of TrajectoryWindow.batch(); order int32 [B] and
    segments int32 [G, 4, 2] from sequence_segments(); rows int64 [G] on the
    same device, zeroed by the caller; returns rows.  Element (k, b) is kept
    iff k < length[b], t0[b] + k < last_table (a learner passes horizon - 1,
    the table that only bootstraps; negative: no bound) and it is not the last
    row of a lifeline a reset ended.  On a GPU nothing is read by the host."""
    dev = rows.device
    B, G, length, t0, end, order, segments = _sequence_columns(length, t0, end, order, segments, rows, dev)
    _on_device(dev, lambda d, st: _lib.mbots_policy_seq_group_rows(
        _ptr(length), _ptr(t0), _ptr(end), B, _ptr(order), _ptr(segments), G, int(last_table), _ptr(rows), d, st))
    return rows


def a2c_loss_sequences(logp, value, entropy, adv, ret, length, t0, end, order, segments, rows, last_table=-1,
                       value_coef=0.5, entropy_coef=0.01, loss=None):
    """(g_logp, g_value, g_entropy, loss): a2c_loss_groups for the padded
    [L, B] sequence batches (mbots_policy_seq_a2c_loss; DESIGN.md "Device
    learner step").  logp, value, entropy: float32 [L, B], what
    evaluate_sequences_groups() returned, read detached; adv, ret: the batch's
    float32 [L, B]; length, t0, end, order, segments, last_table as
    sequence_group_rows'; rows int64 [G], every group's kept elements over
    the whole update.  A kept element of a column of group g weighs
    1 / rows[g] in a2c_loss_groups' formulas; every other element gets +0 in
    the three gradients and takes no part in loss, and so does all of a group
    with rows[g] == 0.  loss: float64 [G], accumulated into (None: zeros), in
    a fixed order, so CPU and GPU tensors give the same bits.  Then

        torch.autograd.backward([logp, value, entropy], [g_logp, g_value, g_entropy])

    runs evaluate_sequences_groups' backward.  Nothing waits for the host;
    capturable."""
    dev = logp.device
    if logp.dim() != 2:
        raise ValueError(f"logp must be float32 [L, B], not {list(logp.shape)}")
    L, B = logp.shape
    cols = []
    for name, t in (("logp", logp), ("value", value), ("entropy", entropy), ("adv", adv), ("ret", ret)):
        if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (L, B):
            raise ValueError(f"{name} must be float32 [{L}, {B}] on {dev}, not {t.dtype} {list(t.shape)} on "
                             f"{t.device}")
        cols.append(t.detach().contiguous())
    if length.numel() != B:
        raise ValueError(f"length must be int32 [{B}] on {dev}, not {length.dtype} {list(length.shape)} on "
                         f"{length.device}")
    _, G, length, t0, end, order, segments = _sequence_columns(length, t0, end, order, segments, rows, dev)
    if loss is None:
        loss = torch.zeros(G, dtype=torch.float64, device=dev)
    elif loss.dtype != torch.float64 or loss.device != dev or tuple(loss.shape) != (G,) or not loss.is_contiguous():
        raise ValueError(f"loss must be a contiguous float64 [{G}] on {dev}, not {loss.dtype} {list(loss.shape)} on "
                         f"{loss.device}")
    g = [torch.empty((L, B), dtype=torch.float32, device=dev) for _ in range(3)]
    _on_device(dev, lambda d, st: _lib.mbots_policy_seq_a2c_loss(
        _ptr(cols[0]), _ptr(cols[1]), _ptr(cols[2]), _ptr(cols[3]), _ptr(cols[4]), _ptr(length), _ptr(t0), _ptr(end),
        L, B, _ptr(order), _ptr(segments), G, int(last_table), _ptr(rows), value_coef, entropy_coef, _ptr(g[0]),
        _ptr(g[1]), _ptr(g[2]), _ptr(loss), d, st))
    return g[0], g[1], g[2], loss


def _ppo_workspace(n, G, dev):
    """The cached scratch of the PPO calls over n rows (or L * B elements):
    (uint8 buffer, bytes)."""
    need = ctypes.c_uint64()
    _check(_lib.mbots_policy_ppo_workspace(n, G, ctypes.byref(need)))
    key = (dev, need.value)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(max(need.value, 64), dtype=torch.uint8, device=dev)
    return ws, need.value


def _ppo_f64(name, t, shape, dev):
    """A caller's float64 accumulator of `shape` on dev, or zeros for None."""
    if t is None:
        return torch.zeros(shape, dtype=torch.float64, device=dev)
    if t.dtype != torch.float64 or t.device != dev or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float64 {list(shape)} on {dev}, not {t.dtype} {list(t.shape)} "
                         f"on {t.device}")
    return t


def _ppo_segments(segments, dev):
    G = segments.shape[0] if segments.dim() == 3 else 0
    if segments.dtype != torch.int32 or segments.device != dev or tuple(segments.shape) != (G, 4, 2) or not 1 <= G <= 64:
        raise ValueError(f"segments must be int32 [G, 4, 2] of 1..64 groups on {dev}, not {segments.dtype} "
                         f"{list(segments.shape)} on {segments.device}")
    return G, segments.detach().contiguous()


def _ppo_rows(named, end, dev):
    """The checked float32 [n] (or [n, 1]) columns and the END column."""
    n = named[0][1].numel()
    cols = []
    for name, t in named:
        if t is None:
            cols.append(None)
            continue
        if t.dtype != torch.float32 or t.device != dev or t.numel() != n or tuple(t.shape) not in ((n,), (n, 1)):
            raise ValueError(f"{name} must be float32 [n] or [n, 1] on {dev} with {named[0][0]}'s {n} rows, not "
                             f"{t.dtype} {list(t.shape)} on {t.device}")
        cols.append(t.detach().reshape(n).contiguous())
    if end is not None:
        if end.dtype != torch.int32 or end.device != dev or tuple(end.shape) not in ((n,), (n, 1)):
            raise ValueError(f"end must be int32 [n] or [n, 1] on {dev}, not {end.dtype} {list(end.shape)} on "
                             f"{end.device}")
        end = end.detach().reshape(n).contiguous()
    return n, cols, end


def _ppo_coefs(clip, value_clip, value_coef):
    if not 0.0 < clip < 1.0:
        raise ValueError(f"clip must lie in (0, 1), not {clip}")
    if not value_coef >= 0.0:
        raise ValueError(f"value_coef must not be negative, not {value_coef}")
    return 0.0 if value_clip is None else float(value_clip)


def advantage_moments_groups(adv, end, segments, moments=None):
    """moments[g] += (count, sum adv, sum adv**2) of group g's kept rows of one
    table, in exact float64 and a fixed order (mbots_policy_adv_moments;
    DESIGN.md "PPO on the device"): what ppo_loss_groups normalises
    advantages with.  adv float32 [n] or [n, 1]; end int32 [n] or [n, 1], the
    window's END column (rows with END_RESET are left out), or None: every row
    counts; segments int32 [G, 4, 2]; moments float64 [G, 3], accumulated into
    (None: zeros) and returned -- pass every table of the update once.  CPU and
    GPU tensors give the same bits.  Nothing waits for the host; capturable."""
    dev = adv.device
    G, segments = _ppo_segments(segments, dev)
    n, (adv,), end = _ppo_rows([("adv", adv)], end, dev)
    moments = _ppo_f64("moments", moments, (G, 3), dev)
    ws, nb = _ppo_workspace(n, G, dev)
    _on_device(dev, lambda d, st: _lib.mbots_policy_adv_moments(
        _ptr(adv), _ptr(end), n, _ptr(segments), G, _ptr(moments), _ptr(ws), nb, d, st))
    return moments


def advantage_moments_sequences(adv, length, t0, end, order, segments, last_table=-1, moments=None):
    """advantage_moments_groups for a padded [L, B] sequence batch
    (mbots_policy_seq_adv_moments): moments[g] += (count, sum, sum of squares)
    of the kept elements of the columns of group g's segments.  adv float32
    [L, B]; length, t0, end, order, segments, last_table as
    sequence_group_rows'.  Returns moments, float64 [G, 3]."""
    dev = adv.device
    if adv.dim() != 2 or adv.dtype != torch.float32:
        raise ValueError(f"adv must be float32 [L, B], not {adv.dtype} {list(adv.shape)}")
    L, B = adv.shape
    if length.numel() != B:
        raise ValueError(f"length must be int32 [{B}] on {dev}, not {length.dtype} {list(length.shape)} on "
                         f"{length.device}")
    none = torch.zeros(segments.shape[0] if segments.dim() == 3 else 0, dtype=torch.int64, device=dev)
    _, G, length, t0, end, order, segments = _sequence_columns(length, t0, end, order, segments, none, dev)
    moments = _ppo_f64("moments", moments, (G, 3), dev)
    adv = adv.detach().contiguous()
    ws, nb = _ppo_workspace(L * B, G, dev)
    _on_device(dev, lambda d, st: _lib.mbots_policy_seq_adv_moments(
        _ptr(adv), _ptr(length), _ptr(t0), _ptr(end), L, B, _ptr(order), _ptr(segments), G, int(last_table),
        _ptr(moments), _ptr(ws), nb, d, st))
    return moments


def ppo_loss_groups(logp, value, entropy, old_logp, old_value, adv, ret, end, segments, rows, clip=0.2,
                    value_clip=None, value_coef=0.5, entropy_coef=0.01, moments=None, stats=None):
    """(g_logp, g_value, g_entropy, stats): PPO's clipped loss of a table's
    recorded rows and its gradients with respect to evaluate's three outputs,
    in one pass of the library's own arithmetic (mbots_policy_ppo_loss;
    DESIGN.md "PPO on the device").  logp, value, entropy: float32 [n], what
    evaluate_groups() returned for the current parameters, read detached;
    old_logp, old_value: act()'s "logp" and "value" of the table when it was
    recorded (old_value may be None); adv, ret, end, segments, rows as
    a2c_loss_groups'.  A row of group g weighs w = (end != END_RESET) / rows[g]:

        A       = (adv - mean_g) / (std_g + 1e-8)  with moments, else adv
        ratio   = exp(logp - old_logp)
        pol     = -min(ratio * A, clamp(ratio, 1 - clip, 1 + clip) * A)
        vl      = (value - ret)**2, or with value_clip > 0 and old_value its maximum with
                  (old_value + clamp(value - old_value, -value_clip, value_clip) - ret)**2
        per_row = (pol + value_coef * vl - entropy_coef * entropy) * w

    and g_* are per_row's derivatives (a tie of the two surrogates takes the
    unclipped one); rows in no segment get +0.  moments: float64 [G, 3] from
    advantage_moments_groups over the whole update -- the unbiased standard
    deviation; fewer than two rows: no normalisation -- or None: raw
    advantages.  stats: float64 [G, 6], accumulated into (None: zeros): the
    groups' sums of per_row, pol * w, vl * w, entropy * w, the KL estimate
    ((ratio - 1) - log ratio) * w and the clipped fraction (clamp changed the
    ratio) * w, in a fixed two-level order that is a property of the row
    indices alone, so CPU and GPU tensors give the same bits.  Non-finite
    inputs propagate into stats; a NaN KL closes ppo_kl_gate, and a clipped
    PolicyAdam leaves a group with a non-finite gradient norm untouched.  Then

        torch.autograd.backward([logp, value, entropy], [g_logp, g_value, g_entropy])

    runs evaluate's backward.  After the first call of a shape nothing
    allocates but the three outputs; nothing waits for the host; capturable."""
    dev = logp.device
    G, segments = _ppo_segments(segments, dev)
    value_clip = _ppo_coefs(clip, value_clip, value_coef)
    n, cols, end = _ppo_rows([("logp", logp), ("value", value), ("entropy", entropy), ("old_logp", old_logp),
                              ("old_value", old_value), ("adv", adv), ("ret", ret)], end, dev)
    if rows.dtype != torch.int64 or rows.device != dev or tuple(rows.shape) != (G,) or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous int64 [{G}] on {dev}, not {rows.dtype} {list(rows.shape)} on "
                         f"{rows.device}")
    if moments is not None:
        moments = _ppo_f64("moments", moments, (G, 3), dev)
    stats = _ppo_f64("stats", stats, (G, 6), dev)
    ws, nb = _ppo_workspace(n, G, dev)
    g = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3)]
    _on_device(dev, lambda d, st: _lib.mbots_policy_ppo_loss(
        *[_ptr(c) for c in cols], _ptr(end), n, _ptr(segments), G, _ptr(rows), _ptr(moments), clip, value_clip,
        value_coef, entropy_coef, _ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(stats), _ptr(ws), nb, d, st))
    return g[0], g[1], g[2], stats


def ppo_loss_sequences(logp, value, entropy, old_logp, old_value, adv, ret, length, t0, end, order, segments, rows,
                       last_table=-1, clip=0.2, value_clip=None, value_coef=0.5, entropy_coef=0.01, moments=None,
                       stats=None):
    """(g_logp, g_value, g_entropy, stats): ppo_loss_groups for the padded
    [L, B] sequence batches (mbots_policy_seq_ppo_loss).  logp, value, entropy:
    float32 [L, B] from evaluate_sequences_groups(); old_logp: the window's
    gather() of act()'s "logp" tables; old_value: the batch's "value" (or
    None); adv, ret: the batch's; length, t0, end, order, segments, rows,
    last_table as a2c_loss_sequences'.  A kept element of a column of group g
    weighs 1 / rows[g]; every other element gets +0 and takes no part in
    stats, and so does all of a group with rows[g] == 0.  moments from
    advantage_moments_sequences.  The sums run over the segments' positions in
    the same two-level order, a column's kept steps in ascending order."""
    dev = logp.device
    if logp.dim() != 2:
        raise ValueError(f"logp must be float32 [L, B], not {list(logp.shape)}")
    L, B = logp.shape
    value_clip = _ppo_coefs(clip, value_clip, value_coef)
    cols = []
    for name, t in (("logp", logp), ("value", value), ("entropy", entropy), ("old_logp", old_logp),
                    ("old_value", old_value), ("adv", adv), ("ret", ret)):
        if t is None and name == "old_value":
            cols.append(None)
            continue
        if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (L, B):
            raise ValueError(f"{name} must be float32 [{L}, {B}] on {dev}, not {t.dtype} {list(t.shape)} on "
                             f"{t.device}")
        cols.append(t.detach().contiguous())
    if length.numel() != B:
        raise ValueError(f"length must be int32 [{B}] on {dev}, not {length.dtype} {list(length.shape)} on "
                         f"{length.device}")
    _, G, length, t0, end, order, segments = _sequence_columns(length, t0, end, order, segments, rows, dev)
    if moments is not None:
        moments = _ppo_f64("moments", moments, (G, 3), dev)
    stats = _ppo_f64("stats", stats, (G, 6), dev)
    ws, nb = _ppo_workspace(L * B, G, dev)
    g = [torch.empty((L, B), dtype=torch.float32, device=dev) for _ in range(3)]
    _on_device(dev, lambda d, st: _lib.mbots_policy_seq_ppo_loss(
        *[_ptr(c) for c in cols], _ptr(length), _ptr(t0), _ptr(end), L, B, _ptr(order), _ptr(segments), G,
        int(last_table), _ptr(rows), _ptr(moments), clip, value_clip, value_coef, entropy_coef, _ptr(g[0]), _ptr(g[1]),
        _ptr(g[2]), _ptr(stats), _ptr(ws), nb, d, st))
    return g[0], g[1], g[2], stats


def ppo_kl_gate(stats, rows, target_kl, gate):
    """PPO's KL early stop without a read by the host (mbots_policy_ppo_gate):

        gate[g] = rows[g] if gate[g] != 0 and rows[g] != 0 and stats[g, 4] <= target_kl else 0

    stats float64 [G, 6], an epoch's from ppo_loss_groups / ppo_loss_sequences
    (slot 4: the group's KL estimate); rows, gate int64 [G] on the same device.
    Start an update with gate = rows.clone() and pass the gate to
    PolicyAdam.step(gate): a group whose KL passed target_kl -- or is NaN --
    is left untouched by this and every later step of the update, as an idle
    group is; a closed gate stays closed until the caller sets it again.
    Returns gate.  Capturable."""
    dev = stats.device
    G = stats.shape[0] if stats.dim() == 2 else 0
    if not 1 <= G <= 64:
        raise ValueError(f"stats must be float64 [G, 6] of 1..64 groups, not {list(stats.shape)}")
    _ppo_f64("stats", stats, (G, 6), dev)
    for name, t in (("rows", rows), ("gate", gate)):
        if t.dtype != torch.int64 or t.device != dev or tuple(t.shape) != (G,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 [{G}] on {dev}, not {t.dtype} {list(t.shape)} on "
                             f"{t.device}")
    _on_device(dev, lambda d, st: _lib.mbots_policy_ppo_gate(_ptr(stats), _ptr(rows), G, float(target_kl), _ptr(gate),
                                                             d, st))
    return gate


class PolicyAdam:
    """Adam over the parameters of every net of every policy group in one call
    (mbots_policy_adam; DESIGN.md "Device learner step"): torch.optim.Adam's
    update without weight decay, in the library's own float32 arithmetic, so
    host tensors and GPU tensors end with the same bits.  nets as
    evaluate_groups': a list of G groups, each four PolicyNet or one for all
    four, None where a pair has none; a flat list of four nets, or one net,
    is one group.  Every distinct tensor the nets reference with
    requires_grad -- memory head and gate included -- is updated, once, with
    its group's step count; a tensor shared across groups raises.

    step(rows=None) reads every parameter's .grad (None: skipped) and updates
    the parameters in place; rows int64 [G] on the parameters' device: a group
    with rows[g] == 0 is left untouched, state included.  zero_grad() binds
    every .grad to a slice of one buffer the optimiser owns and zeroes that
    buffer with one stream-ordered fill, so the gradients keep their
    addresses from update to update and a captured update replays.  Neither
    waits for the host.

    max_grad_norm (None: off) clips every group's gradient to that global
    norm by torch.nn.utils.clip_grad_norm_'s rule, and weight_decay is
    torch.optim.AdamW's decoupled p -= lr * weight_decay * p, both inside the
    one call (mbots_policy_adam_clip) with the norm summed in a fixed order.
    With either, grad_norm (float32 [G] on the parameters' device) holds the
    last step's norms of all groups, idle ones included, and a group whose
    norm is inf or NaN is left untouched -- parameters, moments and step
    count -- as an idle group is.  Without both, step() is the plain call."""

    def __init__(self, nets, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, weight_decay=0.0):
        if isinstance(nets, PolicyNet):
            nets = [[nets] * 4]
        nets = list(nets)
        if len(nets) == 4 and all(x is None or isinstance(x, PolicyNet) for x in nets):
            nets = [nets]
        groups = [list(g) if isinstance(g, (list, tuple)) else [g] * 4 for g in nets]
        G = len(groups)
        if not 1 <= G <= 64:
            raise ValueError(f"nets must hold 1..64 groups, not {G}")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.weight_decay = float(weight_decay)
        if self.max_grad_norm is not None and not self.max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm must be a positive number or None, not {max_grad_norm}")
        if not 0.0 <= self.weight_decay < float("inf"):
            raise ValueError(f"weight_decay must be a finite number >= 0, not {weight_decay}")
        self.params, self.names, self.param_group = [], [], []
        seen = {}                                     # id(tensor) -> (group, name)
        for g, four in enumerate(groups):
            if len(four) != 4 or any(x is not None and not isinstance(x, PolicyNet) for x in four):
                raise ValueError(f"nets[{g}] must be four PolicyNet (or None), or one PolicyNet for all species")
            for s, x in enumerate(four):
                if x is None:
                    continue
                named = x._named_params()
                if x.memory is not None:
                    named += [("memory Linear weight", x.memory[0]), ("memory Linear bias", x.memory[1])]
                if x.gate is not None:
                    named += [("gate Linear weight", x.gate[0]), ("gate Linear bias", x.gate[1])]
                for name, p in named:
                    if p is None or not p.requires_grad:
                        continue
                    where = f"{_species_name(g, s)}: {name}"
                    if id(p) in seen:
                        g0, first = seen[id(p)]
                        if g0 != g:
                            raise ValueError(f"{where} is also {first}: a parameter tensor shared across groups has "
                                             "no one step count")
                        continue
                    if p.dtype != torch.float32 or not p.is_contiguous():
                        raise ValueError(f"{where} must be a contiguous float32 tensor, not {p.dtype} with strides "
                                         f"{list(p.stride())}")
                    if self.params and p.device != self.params[0].device:
                        raise ValueError(f"{where} is on {p.device}, other parameters on {self.params[0].device}")
                    seen[id(p)] = (g, where)
                    self.params.append(p)
                    self.names.append(where)
                    self.param_group.append(g)
        if not self.params:
            raise ValueError("the nets hold no parameter with requires_grad")
        self.groups, dev = G, self.params[0].device
        self.device = dev
        # every tensor's slice of m, v and the gradient buffer starts 16-byte aligned
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self._m = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._g = torch.zeros(total, dtype=torch.float32, device=dev)
        self._views = [self._g[o:o + p.numel()].view(p.shape) for o, p in zip(self.offsets, self.params)]
        # struct mbots_policy_adam_state [G]: {t, bits of b1t, bits of b2t}
        self._state = torch.tensor([[0, 0x3F800000, 0x3F800000]] * G, dtype=torch.int32, device=dev)
        self._desc = (_AdamTensor * len(self.params))()
        for i, (p, o, g) in enumerate(zip(self.params, self.offsets, self.param_group)):
            d = self._desc[i]
            d.param, d.group = p.data_ptr(), g
            d.m, d.v = self._m.data_ptr() + 4 * o, self._v.data_ptr() + 4 * o
        # the clipped call's workspace and norms, sized for every parameter with a gradient
        self._clip = self.max_grad_norm is not None or self.weight_decay != 0.0
        self.grad_norm = torch.zeros(G, dtype=torch.float32, device=dev)
        self._ws = None
        if self._clip:
            for d, p in zip(self._desc, self.params):
                d.n = p.numel()
            need = ctypes.c_uint64()
            _check(_lib.mbots_policy_adam_clip_workspace(self._desc, len(self.params), G, ctypes.byref(need)))
            self._ws = torch.zeros((need.value + 7) // 8, dtype=torch.float64, device=dev)

    def zero_grad(self):
        for p, view in zip(self.params, self._views):
            g = p.grad
            if g is None or g.data_ptr() != view.data_ptr():
                p.grad = view
        self._g.zero_()

    def step(self, rows=None):
        G, dev = self.groups, self.device
        if rows is not None and (rows.dtype != torch.int64 or rows.device != dev or tuple(rows.shape) != (G,)
                                 or not rows.is_contiguous()):
            raise ValueError(f"rows must be a contiguous int64 [{G}] on {dev}, not {rows.dtype} {list(rows.shape)} "
                             f"on {rows.device}")
        desc = self._desc
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                desc[i].n = 0
                continue
            if g.dtype != torch.float32 or g.device != dev or g.shape != p.shape or not g.is_contiguous():
                raise ValueError(f"{self.names[i]}: .grad must be a contiguous float32 tensor of the parameter's "
                                 f"shape on {dev}, not {g.dtype} {list(g.shape)} on {g.device}")
            desc[i].param, desc[i].grad, desc[i].n = p.data_ptr(), g.data_ptr(), p.numel()
        with torch.no_grad():
            if self._clip:
                max_norm = -1.0 if self.max_grad_norm is None else self.max_grad_norm
                _on_device(dev, lambda d, st: _lib.mbots_policy_adam_clip(
                    desc, len(self.params), _ptr(self._state), G, _ptr(rows), self.lr, self.betas[0], self.betas[1],
                    self.eps, self.weight_decay, max_norm, _ptr(self.grad_norm), _ptr(self._ws),
                    self._ws.numel() * 8, d, st))
                return
            _on_device(dev, lambda d, st: _lib.mbots_policy_adam(
                desc, len(self.params), _ptr(self._state), G, _ptr(rows), self.lr, self.betas[0], self.betas[1],
                self.eps, d, st))

    @property
    def steps(self):
        """int32 [G] on the parameters' device: the steps every group has taken."""
        return self._state[:, 0].clone()

    def state_dict(self):
        """{"m", "v": float32 [P], "state": int32 [G, 3]} -- copies; the
        moments of the parameters in the optimiser's order, each slice padded
        to a multiple of 4 floats; state rows are (t, bits of beta1^t, bits of
        beta2^t)."""
        return {"m": self._m.clone(), "v": self._v.clone(), "state": self._state.clone()}

    def load_state_dict(self, sd):
        for key, mine in (("m", self._m), ("v", self._v), ("state", self._state)):
            t = sd[key]
            if t.dtype != mine.dtype or tuple(t.shape) != tuple(mine.shape):
                raise ValueError(f"state_dict[{key!r}] must be {mine.dtype} {list(mine.shape)}, not {t.dtype} "
                                 f"{list(t.shape)}: the nets differ from those it was saved for")
        for key, mine in (("m", self._m), ("v", self._v), ("state", self._state)):
            mine.copy_(sd[key])


class TrajectoryWindow:
    """Agent lifelines, returns and GAE(lambda) over up to `horizon`
    consecutive tables (include/mbots.h "Trajectory window"), from
    SimManager.trajectory_window().  push(value) after the constructor (the
    initial table) or after a step() records the table's provenance, rewards,
    world indices and the caller's value estimates; compute() returns, per
    pushed table, the maps and sweeps as torch views of the window's storage.
    The learner keeps its own per-step tensors (observations, log-probs) in each
    step's row order and gathers them with "next" / lifelines() -- or opens the
    window with record_obs / record_state and takes padded sequence batches
    from sequences() / batch() / gather()."""

    LINK, NEXT, END, WORLD, REWARD, VALUE, ADV, RET = range(8)   # enum mbots_traj_view_id
    END_NONE, END_DIED, END_RESET, END_WINDOW = range(4)
    _KEYS = (("link", LINK), ("next", NEXT), ("end", END), ("world", WORLD), ("reward", REWARD),
             ("value", VALUE), ("adv", ADV), ("ret", RET))

    SEQ_ID, SEQ_POS = 8, 9
    FLAG_SEQ, FLAG_REC_OBS, FLAG_REC_STATE = 1, 2, 4   # MBOTS_TRAJ_SEQ, _REC_OBS, _REC_STATE
    OBS_DIM, HIDDEN_DIM = 69, 16

    def __init__(self, mgr, horizon, max_rows, flags=0):
        self._mgr = weakref.ref(mgr)   # (the manager holds the window: no cycle)
        self.horizon = horizon
        self.max_rows = max_rows
        self.flags = flags
        self._last = None
        self._S = None                 # sequences of the last sequences(), None: stale

    def _live(self):
        m = self._mgr() if self._mgr is not None else None
        if m is None:
            raise RuntimeError("madrona_bots: the trajectory window is closed")
        return m

    @property
    def num_tables(self):
        """Tables pushed since the last clear()."""
        v = ctypes.c_uint32()
        _check(_lib.mbots_traj_num_tables(self._live()._h, ctypes.byref(v)))
        return v.value

    def push(self, value=None):
        """Record the current table (mbots_traj_push; no host synchronisation).
        value: float32 [N] or [N, 1] on the manager's device in the table's row
        order (the critic's estimate per row; a longer buffer's first N entries
        are read), or None for zeros."""
        m = self._live()
        ptr = None
        if value is not None:
            if value.dtype != torch.float32 or value.device != m.device:
                raise ValueError(f"value must be a float32 tensor on {m.device}")
            value = value.reshape(-1).contiguous()
            # the launch reads min(N, max_rows) values: a buffer of max_rows is
            # always enough; a shorter one must hold the table's N (a host wait
            # for the row count, which the learner's own reads already made)
            if value.numel() < self.max_rows and value.numel() < m.num_agents():
                raise ValueError(f"value holds {value.numel()} entries, the table {m.num_agents()} rows")
            ptr = value.data_ptr()
        _check(_lib.mbots_traj_push(m._h, ctypes.c_void_p(ptr), m._stream()))
        self._last = None
        self._S = None

    def view(self, what, t):
        """One column of table t as a [N_t, 1] torch view (mbots_traj_view)."""
        m = self._live()
        ct = _CTensor()
        _check(_lib.mbots_traj_view(m._h, int(what), int(t), ctypes.byref(ct)))
        return Tensor(m._hd, ct).to_torch()

    def compute(self, gamma, lam=1.0, death_reward=0.0):
        """mbots_traj_compute over the n pushed tables: {"rows": [N_0..N_{n-1}],
        "link", "world", "reward", "value", "end", "adv", "ret": n tensors
        [N_t, 1] each, "next": n - 1 tensors}, views of the window's storage
        (valid until the next clear() / close(); a later compute() rewrites the
        derived ones in place).  The one host synchronisation of the window."""
        m = self._live()
        rows = (ctypes.c_int64 * self.horizon)()
        n = ctypes.c_uint32()
        _check(_lib.mbots_traj_compute(m._h, float(gamma), float(lam), float(death_reward), rows,
                                       ctypes.byref(n), m._stream()))
        n = n.value
        out = {"rows": [int(rows[t]) for t in range(n)]}
        for key, what in self._KEYS:
            out[key] = [self.view(what, t) for t in range(n - 1 if what == self.NEXT else n)]
        self._last = out
        return out

    def lifelines(self, t0=0):
        """int64 [n - t0, N_t0]: column j is agent j of table t0 followed
        forward -- row k holds its row in table t0 + k, -1 from the step after
        its end -- composed from the "next" maps of the last compute().  What a
        recurrent learner gathers its own per-step tensors with."""
        if self._last is None:
            raise RuntimeError("madrona_bots: lifelines() follows a compute() of the pushed tables")
        nxt, rows = self._last["next"], self._last["rows"]
        n = len(rows)
        if not 0 <= t0 < n:
            raise ValueError(f"t0 must be in [0, {n})")
        dev = self._live().device
        cur = torch.arange(rows[t0], dtype=torch.int64, device=dev)
        out = [cur]
        for t in range(t0, n - 1):
            alive = cur >= 0
            step = torch.full_like(cur, -1)
            if nxt[t].shape[0]:
                step[alive] = nxt[t].reshape(-1).to(torch.int64)[cur[alive]]
            cur = step
            out.append(cur)
        return torch.stack(out)

    def sequences(self):
        """Number the sequences of the computed tables (mbots_traj_sequences;
        needs sequences=True and a compute(); the window's second host
        synchronisation): fills the SEQ_ID / SEQ_POS views and returns S.  A
        sequence is a maximal lifeline inside the window, numbered in
        ascending (start table, start row) order."""
        m = self._live()
        S = ctypes.c_uint64()
        _check(_lib.mbots_traj_sequences(m._h, ctypes.byref(S), m._stream()))
        self._S = int(S.value)
        return self._S

    def _batch_keys(self):
        off = ((), ("obs",))[not self.flags & self.FLAG_REC_OBS] + \
              ((), ("action_in", "hidden0"))[not self.flags & self.FLAG_REC_STATE]
        return [k for k, _ in _TrajBatch._fields_ if k not in off]

    def _batch_range(self, lo, hi):
        """(lo, hi, L) of a batch / gather; the library's refusal when no
        sequences() of the tables now in the window has run."""
        m = self._live()
        if self._S is None or self._last is None:
            _check(_lib.mbots_traj_batch(m._h, 0, 0, ctypes.byref(_TrajBatch()), m._stream()))
            raise RuntimeError("madrona_bots: batch() / gather() follow this object's compute() and sequences()")
        lo = int(lo)
        hi = self._S if hi is None else int(hi)
        if not 0 <= lo <= hi <= self._S:   # (the library's refusal)
            _check(_lib.mbots_traj_batch(m._h, lo, hi, ctypes.byref(_TrajBatch()), m._stream()))
            raise RuntimeError(f"madrona_bots: sequences [{lo}, {hi}) are not within [0, {self._S})")
        return lo, hi, len(self._last["rows"])

    def batch(self, lo=0, hi=None, keys=None, out=None):
        """Sequences [lo, hi) (hi None: S) as padded, start-aligned, time-major
        tensors on the manager's device (mbots_traj_batch; no host
        synchronisation), B = hi - lo, L = the computed tables: "rows" int32
        [L, B] (-1 past a sequence's end); "t0", "len", "end" int32 [B];
        "obs" float32 [L, B, 69] (record_obs); "reward", "value", "adv", "ret"
        float32 [L, B]; "action_in" uint8 [L, B] and "hidden0" float32 [B, 16]
        (record_state); zeros past the end.  keys: the fields wanted (default:
        all the window's flags allow).  out: a dict of contiguous tensors of
        those shapes to write into (its keys select the fields).  obs[:len[b],
        b] with lengths len is what pack_padded_sequence(enforce_sorted=False)
        takes."""
        m = self._live()
        lo, hi, L = self._batch_range(lo, hi)
        B = hi - lo
        f32, i32 = torch.float32, torch.int32
        spec = {"rows": ((L, B), i32), "t0": ((B,), i32), "len": ((B,), i32), "end": ((B,), i32),
                "obs": ((L, B, self.OBS_DIM), f32), "reward": ((L, B), f32), "value": ((L, B), f32),
                "adv": ((L, B), f32), "ret": ((L, B), f32), "action_in": ((L, B), torch.uint8),
                "hidden0": ((B, self.HIDDEN_DIM), f32)}
        if out is None:
            want = self._batch_keys() if keys is None else list(keys)
            for key in want:
                if key not in spec:
                    raise ValueError(f"keys: unknown key {key!r}")
            out = {key: torch.empty(spec[key][0], dtype=spec[key][1], device=m.device) for key in want}
        else:
            for key, t in out.items():
                if key not in spec:
                    raise ValueError(f"out: unknown key {key!r}")
                if t.dtype != spec[key][1] or tuple(t.shape) != spec[key][0] or t.device != m.device \
                        or not t.is_contiguous():
                    raise ValueError(f"out[{key!r}] must be a contiguous {spec[key][1]} {spec[key][0]} tensor "
                                     f"on {m.device}")
        # (an empty tensor's pointer may be null: a field asked for is always handed over)
        tb = _TrajBatch(**{key: (t.data_ptr() or 1) if B else 1 for key, t in out.items()})
        _check(_lib.mbots_traj_batch(m._h, lo, hi, ctypes.byref(tb), m._stream()))
        return out

    def gather(self, tensors, lo=0, hi=None, out=None):
        """The learner's own per-table tensors along sequences [lo, hi)
        (mbots_traj_gather): `tensors` is a list of one contiguous tensor per
        computed table, [N_t, C] or [N_t], of one 4-byte dtype, on the
        manager's device and in that table's row order; returns [L, B, C] of
        that dtype, row (k, b) the row of table t0[b] + k, zeros past the end."""
        m = self._live()
        lo, hi, L = self._batch_range(lo, hi)
        B = hi - lo
        tensors = list(tensors)
        rows = self._last["rows"]
        if len(tensors) != L:
            raise ValueError(f"gather() takes one tensor per computed table ({L})")
        dt = tensors[0].dtype
        C = int(tensors[0].numel() // rows[0]) if rows[0] else (tensors[0].shape[1] if tensors[0].dim() > 1 else 1)
        if dt.itemsize != 4 or not 1 <= C <= 256:
            raise ValueError("gather() takes tensors of a 4-byte dtype with 1 to 256 columns")
        for t, x in enumerate(tensors):
            if x.dtype != dt or x.device != m.device or not x.is_contiguous() or x.numel() != rows[t] * C:
                raise ValueError(f"tensors[{t}] must be a contiguous {dt} [{rows[t]}, {C}] tensor on {m.device}")
        if out is None:
            out = torch.empty((L, B, C), dtype=dt, device=m.device)
        elif out.dtype != dt or tuple(out.shape) != (L, B, C) or out.device != m.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {dt} {(L, B, C)} tensor on {m.device}")
        if B == 0:
            return out
        ptrs = (ctypes.c_void_p * L)(*[x.data_ptr() or None for x in tensors])
        _check(_lib.mbots_traj_gather(m._h, lo, hi, ptrs, L, 4 * C, ctypes.c_void_p(out.data_ptr()), m._stream()))
        return out

    def clear(self, keep_last=False):
        """Empty the window (mbots_traj_clear); keep_last: its newest table
        becomes table 0 of the next window, so consecutive windows chain."""
        _check(_lib.mbots_traj_clear(self._live()._h, 1 if keep_last else 0))
        self._last = None
        self._S = None

    def close(self):
        """Free the window (mbots_traj_close); its views must not be used
        afterwards, and every later call on this object raises."""
        m = self._live()
        _check(_lib.mbots_traj_close(m._h))
        m._traj = None
        self._mgr = None
        self._last = None


class ScriptBotsViewer:
    """The reference module's second class (src/entry/entry.cpp:47-80): a
    windowed viewer around a Manager (src/gfx, Vulkan) whose ``loop(num_epochs,
    step_fn, carry)`` calls ``step_fn(epoch, carry)`` once per rendered frame
    and whose ``get_sim_mgr()`` returns the manager.  The viewer is out of this
    build's scope, so the name exists
    for the reference's imports -- ``from madrona_bots import SimManager,
    ScriptBotsViewer`` (learn/training_loop.py:8, learn/env_app.py:2,
    learn/app.py:1) -- and constructing it raises.  Headless training takes the
    training loop's other branch (``TrainLoopManager`` over ``SimManager``,
    training_loop.py:15-26, :172-173); ``SimManager.render_worlds`` draws the
    worlds without a window, ``SimManager.world_state`` / ``dump_worlds`` replace
    the viewer's readback for offline inspection."""

    def __init__(self, gpu_id, num_worlds, rand_seed, init_num_agents_per_world, window_width,
                 window_height):
        raise NotImplementedError(
            "madrona_bots: ScriptBotsViewer (the reference's Vulkan viewer, src/gfx) is not part of this "
            "build; run headless with SimManager (learn/training_loop.py without --enable_viewer) and "
            "inspect worlds with SimManager.world_state() / dump_worlds()")
