"""Sharded runs grow on their own: every rank but the last steps a ghost world
(shard_ghost=True), mbots_max_population counts it, and each rank leaves its
capacity when its own worlds need it -- results do not depend on the class a
world runs in, so the shards still equal one uncapped oracle.  CPU mode over
gloo (eight ranks), and two HIP shards on one device."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pyoracle as po
from test_sharding import _free_port, _rewards_by_world, _world_states

W, STEPS, CAP0 = 16, 12, 96


def _run(sim, caps=None):
    for t in range(STEPS):
        sim.write_synthetic_actions(1234, t, True)
        sim.step()
        if caps is not None:
            caps.append(sim.agent_capacity)
        sim.shift_observations()


def _shard_result(sim, offset, per):
    sc = sim.species_count_tensor().to_torch().cpu().numpy()
    rew = sim.reward_tensor(False).to_torch().cpu().numpy().ravel()
    return _world_states(sim, offset, per, True), _rewards_by_world(sc, rew, offset)


def _check_against_one(results):
    ref = po.OracleSim(W, 69, 32, cap=1024, num_threads=4)
    _run(ref)
    assert ref.overflow() == 0
    full_states = _world_states(ref, 0, W, False)
    full_rew = _rewards_by_world(ref.species_count(), ref.column(po.COL_REWARD).ravel(), 0)
    seen = set()
    for shard_states, shard_rew in results:
        for w, st in shard_states.items():
            seen.add(w)
            for k in st:   # (world_state returns the first n rows of each array)
                assert np.array_equal(st[k], full_states[w][k]), (w, k)
        for (w, s), r in shard_rew.items():
            assert np.array_equal(r.view(np.uint32), full_rew[(w, s)].view(np.uint32)), (w, s)
    assert seen == set(range(W))
    return ref


def _worker(rank, port, q, ws):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MBOTS_CPU_THREADS="1")
    import madrona_bots as mb
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    per = W // ws
    sim = mb.SimManager(0, per, 69, 32, exec_mode="cpu", world_offset=rank * per,
                        shard_ghost=rank < ws - 1, agent_capacity=CAP0, auto_grow=True)
    caps = []
    _run(sim, caps)
    out = [None] * ws
    dist.all_gather_object(out, (_shard_result(sim, rank * per, per), caps, sim.num_agents(), sim.overflow()))
    if rank == 0:
        q.put(out)
    dist.destroy_process_group()


def test_eight_gloo_ranks_with_ghosts_grow_on_their_own():
    ws = 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, q, ws)) for r in range(ws)]
    for p in procs:
        p.start()
    out = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = _check_against_one([o[0] for o in out])
    assert sum(o[2] for o in out) == ref.num_agents()
    for rank, (_, caps, _, dropped) in enumerate(out):
        assert caps[0] == CAP0 and caps[-1] == 128 and set(caps) == {CAP0, 128}, (rank, caps)
        assert dropped == 0, rank
    # seven ranks need more than 96 slots before their third step, rank 3 one step later
    assert [o[1].index(128) for o in out] == [2, 2, 2, 3, 2, 2, 2, 2]


@pytest.mark.gpu
def test_two_hip_shards_with_ghosts_equal_one():
    import madrona_bots as mb
    per = W // 2
    shards = [mb.SimManager(0, per, 69, 32, world_offset=r * per, shard_ghost=r == 0,
                            agent_capacity=CAP0, auto_grow=True) for r in range(2)]
    handles = [s._h for s in shards]
    for s in shards:
        _run(s)
    ref = _check_against_one([_shard_result(s, r * per, per) for r, s in enumerate(shards)])
    assert sum(s.num_agents() for s in shards) == ref.num_agents()
    for s, h in zip(shards, handles):
        assert s.agent_capacity == 128 and s._h is h
        assert s.overflow() == 0
