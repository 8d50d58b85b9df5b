"""Owed PrevAction (DESIGN.md "Owed PrevAction"): in the headline loop -- step,
shift, a whole-table action write, nobody reading PrevAction -- the shift
launches no kernel; the manager owes the column as (the last table's Action,
that step's src_of) and gathers it only when somebody asks.  Observably
exact: the HIP manager is driven side by side with the product's CPU mode
(bit-identical by contract) and every exported column, current and Prev,
must be equal bit for bit.

The method is tests/test_lazy_hidden.py's: 64 worlds of 32 agents, its shoot-
and breed-heavy action stream (actions random per row and step, so a wrong
permutation cannot match; rows are born, die and cross species boundaries
every step), and every lazy case asserts that the state was really entered
(schedule_info()["prev_action_lazy"]), so no case passes without it."""
import numpy as np
import pytest
import torch

from simpair import COLUMNS, bits
from test_lazy_hidden import MODES, Pair as _Pair, _stretch

pytestmark = pytest.mark.gpu

HIP = MODES[0] == "hip"


class Pair(_Pair):
    def owed(self):
        """whether the manager under test owes PrevAction right now (host
        state, no device call); the CPU mode never does"""
        return self.m[0].schedule_info()["prev_action_lazy"]

    def step_shift(self):
        """step and shift with no write after them: current Action stays the
        owed view"""
        before = self.m[1].num_agents()
        self.each(lambda m: (m.step(), m.shift_observations()))
        self.births += self.m[1].num_agents() != before

    def offsets(self):
        """[start, end) export rows of each species (no shard ghost)"""
        c = self.m[1].species_count_tensor().to_torch().sum(dim=0).cumsum(dim=0).tolist()
        return list(zip([0] + [int(v) for v in c[:-1]], [int(v) for v in c]))


def _owed_stretch(p, start_half, steps):
    _stretch(p, start_half, steps)
    assert p.owed() == HIP


def _finish(p, where):
    p.check(where)
    for _ in range(3):
        p.lazy_step()
    assert p.owed() == HIP, f"{where}: the loop did not return to the owed state"
    p.check(where + ", 3 steps on")
    assert p.births, "the action stream moved no rows"


@pytest.mark.parametrize("first", ["prev", "cur"])
@pytest.mark.parametrize("start_half", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 3, 8])
def test_stretch_then_read(steps, start_half, first):
    """a stretch on either table half, one more step and shift (Action is then
    the owed view too), and both columns read, either one first"""
    p = Pair()
    _owed_stretch(p, start_half, steps)
    p.step_shift()
    assert p.owed() == HIP
    for is_prev in ((True, False) if first == "prev" else (False, True)):
        p.check_column("action_tensor", is_prev, f"stretch {steps}, {first} first")
        assert not p.owed()
    p.write()
    _finish(p, f"stretch {steps} from half {start_half}, {first} first")


def _exit_prev_action(p):
    p.check_column("action_tensor", True, "exit")
    assert not p.owed()


def _exit_action(p):
    p.step_shift()
    assert p.owed() == HIP
    p.check_column("action_tensor", False, "exit")
    assert not p.owed()
    p.write()


def _exit_set_action(p):
    p.step_shift()
    assert p.owed() == HIP
    row = p.rows() // 3
    p.each(lambda m: m.set_action(row, 1, 0, 1, 0, 1, 1))
    assert not p.owed()
    p.check_column("action_tensor", False, "set_action")
    p.write()


def _exit_partial_view(p):
    """half the rows written through the Action view"""
    p.step_shift()
    assert p.owed() == HIP
    half = p.rows() // 2
    a = p.actions(half)

    def wr(m):
        m.action_tensor().to_torch()[:half] = a.to(m.device)
    p.each(wr)
    assert not p.owed()


def _exit_no_write(p):
    """nobody writes before the next step: K1 reads the owed view"""
    p.step_shift()
    assert p.owed() == HIP
    p.step_shift()
    p.check("no write")
    p.write()


def _exit_step(p):
    """a step with no shift, then every column (the new half's deferred
    PrevAction move has an owed source)"""
    p.each(lambda m: m.step())
    assert p.owed() == HIP
    p.check("step, no shift")
    assert not p.owed()
    p.each(lambda m: m.shift_observations())
    p.write()


def _exit_step_step(p):
    p.each(lambda m: (m.step(), m.step()))
    assert not p.owed()
    p.check("step, step")
    p.each(lambda m: m.shift_observations())
    p.write()


def _exit_obs_prev(p):
    o = p.each(lambda m: m.construct_obs(True).cpu().numpy())
    assert np.array_equal(bits(o[0]), bits(o[1])), "construct_obs(prev) differs"
    p.each(lambda m: m.step())
    o = p.each(lambda m: m.construct_obs(True).cpu().numpy())
    assert np.array_equal(bits(o[0]), bits(o[1])), "construct_obs(prev) after a step differs"
    p.each(lambda m: m.shift_observations())
    p.write()


def _exit_pack(p):
    r = p.each(lambda m: m.pack_learner().cpu().numpy())
    assert np.array_equal(r[0], r[1]), "pack_learner differs"
    assert not p.owed()


def _exit_step_pack(p):
    """the learner's records between step and shift"""
    p.each(lambda m: m.step())
    r = p.each(lambda m: m.pack_learner().cpu().numpy())
    assert np.array_equal(r[0], r[1]), "pack_learner after step differs"
    assert not p.owed()
    p.each(lambda m: m.shift_observations())
    p.write()


def _exit_slim(p):
    r = p.each(lambda m: m.pack_learner(slim=True).cpu().numpy())
    assert np.array_equal(r[0], r[1]), "slim learner records differ"
    p.each(lambda m: m.step())
    r = p.each(lambda m: m.pack_learner(slim=True).cpu().numpy())
    assert np.array_equal(r[0], r[1]), "slim learner records after step differ"
    p.each(lambda m: m.shift_observations())
    p.write()


def _exit_checkpoint(p):
    import madrona_bots as mb
    blobs = p.each(lambda m: m.save_checkpoint())
    assert not p.owed()
    worlds, seed, a = p.args
    p.m = [mb.SimManager(0, worlds, seed, a, exec_mode=mode, **p.kw) for mode in MODES]
    for m, b in zip(p.m, blobs):
        m.load_checkpoint(b)


def _exit_checkpoint_view(p):
    """saved while current Action is the owed view too"""
    p.step_shift()
    assert p.owed() == HIP
    _exit_checkpoint(p)
    p.write()


def _exit_reset(p):
    p.each(lambda m: m.reset_worlds([3, 17, 40, 63]))
    assert not p.owed()
    p.lazy_step()
    p.lazy_step()


def _exit_species_shifts(p):
    """the training loop's pattern: the views taken once after the step, a
    shift per species, each species' rows written through the view"""
    p.each(lambda m: m.step())
    views = p.each(lambda m: m.action_tensor().to_torch())
    assert not p.owed()
    for s, e in p.offsets():
        p.each(lambda m: m.shift_observations())
        a = p.actions(e - s)
        for m, v in zip(p.m, views):
            v[s:e] = a.to(m.device)


def _exit_double_shift(p):
    """a second shift copies the written Action over the owed column: dead"""
    p.each(lambda m: m.shift_observations())
    assert not p.owed()
    p.check_column("action_tensor", True, "double shift")


EXITS = {"prev_action": _exit_prev_action, "action": _exit_action, "set_action": _exit_set_action,
         "partial_view": _exit_partial_view, "no_write": _exit_no_write, "step": _exit_step,
         "step_step": _exit_step_step, "obs_prev": _exit_obs_prev, "pack": _exit_pack,
         "step_pack": _exit_step_pack, "slim": _exit_slim, "checkpoint": _exit_checkpoint,
         "checkpoint_view": _exit_checkpoint_view, "reset": _exit_reset,
         "species_shifts": _exit_species_shifts, "double_shift": _exit_double_shift}


@pytest.mark.parametrize("start_half", [0, 1])
@pytest.mark.parametrize("way", sorted(EXITS))
def test_every_way_out(way, start_half):
    p = Pair()
    _owed_stretch(p, start_half, 3)
    EXITS[way](p)
    _finish(p, f"exit {way}")


def test_capacity_grows_mid_stretch():
    """agent_capacity="auto" under a stream that breeds and never shoots: a
    world's 2 n + 32 passes 128 a few steps into the stretch"""
    p = Pair(agent_capacity="auto", probs=(0.4, 0.0, 0.2, 0.2, 0.0, 0.6))
    cap0 = p.m[0].agent_capacity
    _stretch(p, 0, 0)
    owed = 0
    while p.m[0].agent_capacity == cap0 and owed < 24:
        owed += p.owed()
        p.lazy_step()
    assert p.m[0].agent_capacity > cap0, "the stream did not outgrow the first capacity class"
    assert owed >= 2 or not HIP, "the capacity grew before a stretch was under way"
    p.lazy_step()
    _finish(p, "growth")


def test_shard_ghost():
    """the ghost's rows take part; a write of the exported rows only is a
    partial write_actions"""
    p = Pair(shard_ghost=True)
    _owed_stretch(p, 1, 3)
    p.step_shift()
    assert p.owed() == HIP
    n = p.m[1].num_agents()
    assert p.rows() > n
    a = p.actions(n)
    p.each(lambda m: m.write_actions(a.to(m.device)))
    assert not p.owed()
    _finish(p, "ghost")


def test_four_steps_in_flight():
    """2,048 worlds, four owed steps enqueued with no host read in between:
    each K3a writes its parity's src_of while the owed column still reads the
    other one"""
    p = Pair(worlds=2048)
    p.write(memory=True)
    p.eager_step()
    n0 = p.m[1].num_agents()
    for t in range(5):   # (the first makes HiddenState a view: a stretch of four)
        p.each(lambda m: (m.step(), m.shift_observations(), m.write_synthetic_actions(99, t)))
    assert p.owed() == HIP
    assert p.m[1].num_agents() != n0
    p.check("4 steps in flight")
    for t in range(3):
        p.each(lambda m: (m.step(), m.shift_observations(), m.write_synthetic_actions(99, 5 + t)))
    assert p.owed() == HIP
    p.check("3 steps in flight")


def test_graph_after_stretch():
    """a capture taken in the owed state: the gather is recorded once and the
    replays equal the CPU mode's eager steps; no graph step owes anything"""
    p = Pair()
    hip, cpu = p.m
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        _owed_stretch(p, 0, 3)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for t in (0, 1):
                hip.step(); hip.shift_observations(); hip.write_synthetic_actions(7, t)
            hip.join()
    assert not p.owed()
    for _ in range(3):
        g.replay()
        for t in (0, 1):
            cpu.step(); cpu.shift_observations(); cpu.write_synthetic_actions(7, t)
    p.check("graph replays")
    for _ in range(2):
        p.lazy_step()
        assert not p.owed()
    p.check("eager after the graph")


def test_memory_written_every_step():
    """a loop that writes memory every step never owes PrevAction (the shift
    gathers HiddenState anyway), and the columns are equal all the same"""
    p = Pair()
    p.write(memory=True)
    for _ in range(6):
        p.eager_step()
        assert not p.owed()
    p.check("memory every step")
    assert p.m[1].num_agents() != 64 * 32


def _op_step(p):
    p.each(lambda m: m.step())


def _op_shift(p):
    p.each(lambda m: m.shift_observations())


def _op_write_actions(p):
    p.write()


def _op_write_both(p):
    p.write(memory=True)


def _op_read_action(p):
    p.check_column("action_tensor", False, "fuzz")


def _op_read_prev_action(p):
    p.check_column("action_tensor", True, "fuzz")


def _op_read_prev_hidden(p):
    p.check_column("hidden_state_tensor", True, "fuzz")


def _op_set_action(p):
    row = p.rows() // 3
    p.each(lambda m: m.set_action(row, 0, 1, 0, 1, 1, 0))


def _op_partial_view(p):
    half = p.rows() // 2
    a = p.actions(half)

    def wr(m):
        m.action_tensor().to_torch()[:half] = a.to(m.device)
    p.each(wr)


def _op_obs_prev(p):
    o = p.each(lambda m: m.construct_obs(True).cpu().numpy())
    assert np.array_equal(bits(o[0]), bits(o[1])), "construct_obs(prev) differs"


def _op_pack(p):
    r = p.each(lambda m: m.pack_learner().cpu().numpy())
    assert np.array_equal(r[0], r[1]), "pack_learner differs"


def _op_slim(p):
    r = p.each(lambda m: m.pack_learner(slim=True).cpu().numpy())
    assert np.array_equal(r[0], r[1]), "slim learner records differ"


def _op_reset(p):
    p.each(lambda m: m.reset_worlds([3, 17, 40, 63]))


def _op_headline(p):
    p.lazy_step()


# (every sequence starts in the owed state and the headline's calls weigh most,
# so stretches form again; every reader, writer and odd call order cuts into
# them somewhere)
OPS = [(_op_headline, 6), (_op_step, 8), (_op_shift, 8), (_op_write_actions, 8), (_op_write_both, 1), (_op_read_action, 1),
       (_op_read_prev_action, 1), (_op_read_prev_hidden, 1), (_op_set_action, 1), (_op_partial_view, 1),
       (_op_obs_prev, 1), (_op_pack, 1), (_op_slim, 1), (_exit_checkpoint, 1), (_op_reset, 1)]


@pytest.mark.parametrize("seed", range(8))
def test_random_call_sequences(seed):
    """40 calls drawn at random -- steps without shifts, shifts without steps,
    readers and writers between any two -- with every column compared at the
    end and wherever a reader falls"""
    p = Pair(seed=90 + seed)
    _owed_stretch(p, seed & 1, 2)
    rng = np.random.default_rng(100 + seed)
    ops = [op for op, weight in OPS for _ in range(weight)]
    owed = 0
    for k in range(40):
        op = ops[rng.integers(len(ops))]
        was = p.owed()
        op(p)
        owed += was and p.owed()   # calls the state lived through
        if k % 20 == 19:
            p.check(f"seed {seed} call {k} ({op.__name__})")
    # (entered for certain at the start; how long it lasts is the draw's)
    print(f"seed {seed}: the owed state lived through {owed} of 40 calls")
    _finish(p, f"seed {seed}")


def _columns(m):
    out = {"n": m.num_agents(), "species_count": m.species_count_tensor().to_torch().cpu().numpy()}
    for name, _ in COLUMNS:
        for is_prev in (False, True):
            out[name, is_prev] = bits(getattr(m, name)(is_prev).to_torch().cpu().numpy())
    return out


@pytest.mark.parametrize("worlds", [2304, 16400])
def test_larger_world_counts(monkeypatch, worlds):
    """the value-wait schedule (2304 worlds) and the swapped one (16400, no
    multiple of the scan tile): a manager that owes PrevAction beside one
    created with MBOTS_LAZY_PREV_ACTION=0, six steps of the headline loop,
    every column bitwise equal; 2304 worlds also against the CPU mode"""
    import madrona_bots as mb
    lazy = mb.SimManager(0, worlds, 69, 32)
    monkeypatch.setenv("MBOTS_LAZY_PREV_ACTION", "0")   # read when a manager is created
    plain = mb.SimManager(0, worlds, 69, 32)
    monkeypatch.delenv("MBOTS_LAZY_PREV_ACTION")
    ms = [lazy, plain] + ([mb.SimManager(0, worlds, 69, 32, exec_mode="cpu")] if worlds == 2304 else [])
    assert lazy.schedule_info()["swap"] == (worlds > 8192)
    n0 = lazy.num_agents()
    owed = 0
    for t in range(6):
        for m in ms:
            m.step(); m.shift_observations(); m.write_synthetic_actions(31, t)
        owed += lazy.schedule_info()["prev_action_lazy"]
        assert not plain.schedule_info()["prev_action_lazy"]
    assert owed >= 4, "the loop did not owe PrevAction"
    assert plain.schedule_info()["hidden_lazy"]
    want = _columns(ms[0])
    assert want["n"] != n0, "no rows were born or died"
    for k, m in enumerate(ms[1:]):
        got = _columns(m)
        for key, v in want.items():
            assert np.array_equal(v, got[key]), f"{worlds} worlds: {key} differs from manager {k + 1}"
