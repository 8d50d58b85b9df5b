"""Helpers for the committed golden fixtures (tests/golden/*.npz)."""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["species", "pos", "health", "surround", "reward", "action", "stats", "hidden",
         "semantic", "depth"]
FIXTURES = [
    ("oracle_w4_a32_s69", 4, 32, 69, 16, False, 128),
    ("oracle_w8_a4_s7_fixed", 8, 4, 7, 24, True, 16),
]


# recorded from the reference's own simulation code on the stand-in engine
# (tests/golden/make_golden.py; meta["side"] says so): name -> action stream
REF_FIXTURES = ["reference_w8_a32_s69", "reference_w4_a32_s69_breed", "reference_w4_a32_s69_shoot"]


def stream_actions(meta, n, t):
    """The fixture's action rows for step t, [n, 6] int32, or None where its
    stream is the simulator's own write_synthetic_actions."""
    stream = meta.get("stream", "synthetic")
    if stream == "synthetic":
        return None
    return STREAMS[stream](n, t)


def breed_heavy(n, step):
    """tests/test_parity_gpu.py's _breed_heavy: breed 1/2, forward 1/4, rotate 1/4."""
    import torch
    g = torch.Generator().manual_seed(1000 + step)
    r = torch.randint(0, 8, (n,), generator=g).numpy()
    a = np.zeros((n, 6), np.int32)
    a[r < 4, 5] = 1
    a[(r >= 4) & (r < 6), 0] = 1
    a[r == 6, 2] = 1
    a[r == 7, 3] = 1
    return a


def shoot_heavy(n, step):
    """shoot 1/2, forward 1/4, rotate left / right 1/8 each."""
    import torch
    g = torch.Generator().manual_seed(2000 + step)
    r = torch.randint(0, 8, (n,), generator=g).numpy()
    a = np.zeros((n, 6), np.int32)
    a[r < 4, 4] = 1
    a[(r >= 4) & (r < 6), 0] = 1
    a[r == 6, 2] = 1
    a[r == 7, 3] = 1
    return a


STREAMS = {"breed_heavy": breed_heavy, "shoot_heavy": shoot_heavy}


def load_fixture(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    arrays = {k: z[k] for k in z.files if k != "meta"}
    return meta, arrays


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def table_digests(get, species_count):
    """get(name, is_prev) -> numpy array in the oracle's dtypes."""
    out = {}
    for nm in NAMES:
        out[nm] = digest(get(nm, False))
        out["prev_" + nm] = digest(get(nm, True))
    out["species_count"] = digest(species_count)
    return out


def run_digests(sim, meta):
    """Drive the oracle through the fixture's call sequence."""
    def get(nm, prev):
        return sim.column(NAMES.index(nm), prev)
    log = [["init", sim.num_agents(), table_digests(get, sim.species_count())]]
    for t in range(meta["steps"]):
        a = stream_actions(meta, sim.num_agents(), t)
        if a is None:
            sim.write_synthetic_actions(meta["action_seed"], t, meta["write_hidden"])
        else:
            sim.column(NAMES.index("action"))[:] = a
        sim.step()
        log.append([f"step{t}", sim.num_agents(), table_digests(get, sim.species_count())])
        sim.shift_observations()
        log.append([f"shift{t}", sim.num_agents(), table_digests(get, sim.species_count())])
    return log


def run_digests_manager(mgr, meta):
    """The same call sequence through a SimManager (either exec mode); the depth
    digests are empty (not exported without fix_depth_alias) and skipped by the
    caller.  Returns (log, get)."""
    import torch
    acc = {"species": "species_tensor", "pos": "position_tensor", "health": "health_tensor",
           "surround": "surrounding_tensor", "reward": "reward_tensor",
           "action": "action_tensor", "stats": "stats_tensor",
           "hidden": "hidden_state_tensor", "semantic": "semantic_tensor"}

    def get(nm, prev):
        if nm == "depth":
            return np.zeros(0)
        a = getattr(mgr, acc[nm])(prev).to_torch().cpu().numpy()
        return a.view(np.int32) if nm == "health" else a

    def digests():
        return table_digests(get, mgr.species_count_tensor().to_torch().cpu().numpy())

    log = [["init", mgr.num_agents(), digests()]]
    for t in range(meta["steps"]):
        a = stream_actions(meta, mgr.num_agents(), t)
        if a is None:
            mgr.write_synthetic_actions(meta["action_seed"], t, meta["write_hidden"])
        else:
            v = mgr.action_tensor(False).to_torch()
            v.copy_(torch.from_numpy(a).to(v.device))
        mgr.step()
        log.append([f"step{t}", mgr.num_agents(), digests()])
        mgr.shift_observations()
        log.append([f"shift{t}", mgr.num_agents(), digests()])
    return log, get
