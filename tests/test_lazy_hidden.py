"""Lazy HiddenState (DESIGN.md "Lazy HiddenState"): while nobody reads or
writes HiddenState, a step + shift + action write moves no HiddenState rows;
the manager carries a row map composed over the stretch instead and gathers
the column once, when somebody asks.  Observably exact: the HIP manager is
driven side by side with the product's CPU mode (bit-identical by contract)
and every exported column, current and Prev, must be equal bit for bit.

Memory is seeded with each row's identity (row * 16 + k + 1, exact in
float32), so a wrong permutation cannot pass by accident, and the action
stream shoots and breeds heavily: rows are born, die and cross species
boundaries every step.

Covered: stretches of 1, 2, 3 and 8 steps from both table halves (the gather
is never in place, whatever the parity), every way out of the state, four
steps in flight with no host read (the map's two buffers), a graph captured
after a stretch, a growing capacity, resets, and the shard ghost."""
import numpy as np
import pytest
import torch

from simpair import COLUMNS, bits

pytestmark = pytest.mark.gpu

MODES = ("hip", "cpu")   # the manager under test, and what it must equal
W, A = 64, 32


class Pair:
    def __init__(self, worlds=W, seed=69, probs=(0.5, 0.1, 0.3, 0.3, 0.6, 0.7), **kw):
        import madrona_bots as mb
        self.probs = torch.tensor(probs)
        self.args, self.kw = (worlds, seed, A), kw
        self.m = [mb.SimManager(0, worlds, seed, A, exec_mode=mode, **kw) for mode in MODES]
        self.gen = torch.Generator().manual_seed(4321)
        self.births = 0

    def each(self, fn):
        return [fn(m) for m in self.m]

    def rows(self):
        r = self.each(lambda m: m.num_rows())
        assert r[0] == r[1], f"num_rows {r}"
        return r[0]

    def actions(self, rows):
        """forward / turn half the time, shoot and breed most of the time"""
        return (torch.rand((rows, 6), generator=self.gen) < self.probs).to(torch.int32)

    def write(self, memory=False):
        rows = self.rows()
        a = self.actions(rows)
        mem = None
        if memory:   # the row's identity
            mem = (torch.arange(rows * 16, dtype=torch.float32) + 1.0).reshape(rows, 16)
        self.each(lambda m: m.write_actions(a.to(m.device), None if mem is None else mem.to(m.device)))

    def eager_step(self):
        """a step whose memory is written: never lazy"""
        self.each(lambda m: (m.step(), m.shift_observations()))
        self.write(memory=True)

    def lazy_step(self):
        """the headline loop's step: nobody touches HiddenState"""
        before = self.m[1].num_agents()
        self.each(lambda m: (m.step(), m.shift_observations()))
        self.births += self.m[1].num_agents() != before
        self.write()

    def lazy(self):
        """whether the manager under test owes HiddenState right now (host
        state, no device call); the CPU mode never does"""
        return self.m[0].schedule_info()["hidden_lazy"]

    def column(self, name, is_prev):
        return self.each(lambda m: getattr(m, name)(is_prev).to_torch().cpu().numpy())

    def check_column(self, name, is_prev, where):
        g, o = self.column(name, is_prev)
        assert g.shape == o.shape, f"{where}: {name}(prev={is_prev}) shape {g.shape} vs {o.shape}"
        gb, ob = bits(g), bits(o)
        bad = np.nonzero((gb != ob).reshape(len(gb), -1).any(axis=1))[0]
        assert not len(bad), (f"{where}: {name}(prev={is_prev}) {len(bad)} rows differ; first row {bad[0]}: "
                              f"{MODES[0]}={g[bad[0]]} {MODES[1]}={o[bad[0]]}")

    def check(self, where):
        n = self.each(lambda m: m.num_agents())
        assert n[0] == n[1], f"{where}: num_agents {n}"
        sc = self.each(lambda m: m.species_count_tensor().to_torch().cpu().numpy())
        assert np.array_equal(sc[0], sc[1]), f"{where}: species_count differs"
        for name, _ in COLUMNS:
            for is_prev in (False, True):
                self.check_column(name, is_prev, where)


def _stretch(p, start_half, steps):
    """the memory seeded, 1 + `start_half` eager steps (the stretch begins on
    either table half), one step that leaves the memory alone -- from its
    shift on HiddenState is a view, which the next shift can owe -- and then a
    lazy stretch of `steps` steps"""
    p.write(memory=True)
    for _ in range(1 + start_half):
        p.eager_step()
    p.lazy_step()
    assert not p.lazy()
    for _ in range(steps):
        p.lazy_step()
        assert p.lazy() == (MODES[0] == "hip")


def _finish(p, where):
    p.check(where)
    for _ in range(3):
        p.lazy_step()
    p.check(where + ", 3 steps on")
    assert p.births, "the action stream moved no rows"


@pytest.mark.parametrize("start_half", [0, 1])
@pytest.mark.parametrize("steps", [1, 2, 3, 8])
def test_stretch_then_read(steps, start_half):
    p = Pair()
    _stretch(p, start_half, steps)
    p.check_column("hidden_state_tensor", False, f"stretch {steps}")
    assert not p.lazy()
    p.check_column("hidden_state_tensor", True, f"stretch {steps}")
    _finish(p, f"stretch {steps} from half {start_half}")


@pytest.mark.parametrize("start_half", [0, 1])
def test_prev_read_first(start_half):
    """PrevHiddenState read before HiddenState, and between step and shift"""
    p = Pair()
    _stretch(p, start_half, 3)
    p.check_column("hidden_state_tensor", True, "prev first")
    assert not p.lazy()
    p.check_column("hidden_state_tensor", False, "prev first")
    p.lazy_step()
    p.lazy_step()
    p.each(lambda m: m.step())
    p.check_column("hidden_state_tensor", True, "prev after step")
    p.check_column("hidden_state_tensor", False, "prev after step")
    p.each(lambda m: m.shift_observations())
    p.write()
    _finish(p, "prev first")


def _exit_hidden(p):
    p.check_column("hidden_state_tensor", False, "exit")


def _exit_prev_hidden(p):
    p.check_column("hidden_state_tensor", True, "exit")


def _exit_partial_write(p):
    """half the rows written through the HiddenState view"""
    half = p.rows() // 2
    v = -(torch.arange(half * 16, dtype=torch.float32) + 1.0).reshape(half, 16)

    def wr(m):
        m.hidden_state_tensor().to_torch()[:half] = v.to(m.device)
    p.each(wr)


def _exit_full_write(p):
    rows = p.rows()
    mem = (torch.arange(rows * 16, dtype=torch.float32) * 0.5 + 3.0).reshape(rows, 16)
    p.each(lambda m: m.write_actions(None, mem.to(m.device)))


def _exit_step_step(p):
    p.each(lambda m: (m.step(), m.step()))
    p.check("step, step")
    p.each(lambda m: m.shift_observations())
    p.write()


def _exit_obs_pack(p):
    o = p.each(lambda m: m.construct_obs(True).cpu().numpy())
    assert np.array_equal(bits(o[0]), bits(o[1])), "construct_obs(prev) differs"
    r = p.each(lambda m: m.pack_learner().cpu().numpy())
    assert np.array_equal(r[0], r[1]), "pack_learner differs"


def _exit_step_pack(p):
    """the learner's records between step and shift"""
    p.each(lambda m: m.step())
    r = p.each(lambda m: m.pack_learner().cpu().numpy())
    assert np.array_equal(r[0], r[1]), "pack_learner after step differs"
    p.each(lambda m: m.shift_observations())
    p.write()


def _exit_checkpoint(p):
    import madrona_bots as mb
    blobs = p.each(lambda m: m.save_checkpoint())
    worlds, seed, a = p.args
    p.m = [mb.SimManager(0, worlds, seed, a, exec_mode=mode, **p.kw) for mode in MODES]
    for m, b in zip(p.m, blobs):
        m.load_checkpoint(b)


def _exit_reset(p):
    p.each(lambda m: m.reset_worlds([3, 17, 40, 63]))
    p.lazy_step()
    p.lazy_step()


def _exit_double_shift(p):
    p.each(lambda m: m.shift_observations())


EXITS = {"hidden": _exit_hidden, "prev_hidden": _exit_prev_hidden, "partial_write": _exit_partial_write,
         "full_write": _exit_full_write, "step_step": _exit_step_step, "obs_pack": _exit_obs_pack,
         "step_pack": _exit_step_pack, "checkpoint": _exit_checkpoint, "reset": _exit_reset,
         "double_shift": _exit_double_shift}


# (a whole memory write leaves PrevHiddenState owed; flags and a second shift
# touch nothing)
LEAVES = ("hidden", "prev_hidden", "partial_write", "step_step", "obs_pack", "step_pack", "checkpoint")


@pytest.mark.parametrize("start_half", [0, 1])
@pytest.mark.parametrize("way", sorted(EXITS))
def test_every_way_out(way, start_half):
    p = Pair()
    _stretch(p, start_half, 3)
    EXITS[way](p)
    if way in LEAVES:
        assert not p.lazy()
    _finish(p, f"exit {way}")


def test_full_write_then_steps_without_read():
    """memory written whole in the lazy state: PrevHiddenState stays owed, then
    dies at the next shift; nothing is read until the end"""
    p = Pair()
    _stretch(p, 0, 3)
    _exit_full_write(p)
    for _ in range(4):
        p.lazy_step()
    p.check("full write, 4 steps")


def test_capacity_grows_mid_stretch():
    """agent_capacity="auto" under a stream that breeds and never shoots: a
    world's 2 n + 32 passes 128 a few steps into the stretch"""
    p = Pair(agent_capacity="auto", probs=(0.4, 0.0, 0.2, 0.2, 0.0, 0.6))
    cap0 = p.m[0].agent_capacity
    _stretch(p, 0, 0)
    lazy = 0
    while p.m[0].agent_capacity == cap0 and lazy < 24:
        lazy += p.lazy()
        p.lazy_step()
    assert p.m[0].agent_capacity > cap0, "the stream did not outgrow the first capacity class"
    assert lazy >= 2 or MODES[0] != "hip", "the capacity grew before a stretch was under way"
    p.lazy_step()
    _finish(p, "growth")


def test_shard_ghost():
    """the ghost's rows take part; a memory write of the exported rows only is
    a partial write"""
    p = Pair(shard_ghost=True)
    _stretch(p, 1, 3)
    n = p.m[1].num_agents()
    assert p.rows() > n
    mem = (torch.arange(n * 16, dtype=torch.float32) + 0.25).reshape(n, 16)
    a = p.actions(n)
    p.each(lambda m: m.write_actions(a.to(m.device), mem.to(m.device)))
    _finish(p, "ghost")


def test_four_steps_in_flight():
    """2,048 worlds, four lazy steps enqueued with no host read in between:
    each K3a reads the last step's map while it writes its own, and the
    gather at the end must not be in place"""
    p = Pair(worlds=2048)
    p.write(memory=True)
    p.eager_step()
    n0 = p.m[1].num_agents()
    for t in range(5):   # (the first makes HiddenState a view: a stretch of four)
        p.each(lambda m: (m.step(), m.shift_observations(), m.write_synthetic_actions(99, t)))
    assert p.lazy() == (MODES[0] == "hip")
    assert p.m[1].num_agents() != n0
    p.check("4 steps in flight")
    for t in range(3):
        p.each(lambda m: (m.step(), m.shift_observations(), m.write_synthetic_actions(99, 5 + t)))
    p.check("3 steps in flight")


def test_graph_after_stretch():
    """a capture taken in the lazy state: the gather is recorded once and the
    replays equal the CPU mode's eager steps"""
    p = Pair()
    hip, cpu = p.m
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        _stretch(p, 0, 3)
        assert p.lazy()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for t in (0, 1):
                hip.step(); hip.shift_observations(); hip.write_synthetic_actions(7, t)
            hip.join()
    assert not p.lazy()
    for _ in range(3):
        g.replay()
        for t in (0, 1):
            cpu.step(); cpu.shift_observations(); cpu.write_synthetic_actions(7, t)
    p.check("graph replays")
    for _ in range(2):
        p.lazy_step()
    p.check("eager after the graph")


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


def _op_slim(p):
    r = p.each(lambda m: m.pack_learner(slim=True).cpu().numpy())
    assert np.array_equal(r[0], r[1]), "slim learner records differ"


# (the headline's calls weigh most, so stretches form; every reader, writer and
# odd call order cuts into them somewhere)
OPS = [(_op_step, 8), (_op_shift, 8), (_op_write_actions, 8), (_op_write_both, 1), (_exit_hidden, 1),
       (_exit_prev_hidden, 1), (_exit_partial_write, 1), (_exit_full_write, 1), (_exit_obs_pack, 1),
       (_op_read_action, 1), (_op_read_prev_action, 1), (_op_slim, 1), (_exit_checkpoint, 1), (_exit_reset, 1)]


@pytest.mark.parametrize("seed", range(8))
def test_random_call_sequences(seed):
    """60 calls drawn at random -- steps without shifts, shifts without steps,
    readers and writers between any two -- with every column compared at the
    end and wherever a reader falls"""
    p = Pair(seed=70 + seed)
    p.write(memory=True)
    rng = np.random.default_rng(seed)
    ops = [op for op, weight in OPS for _ in range(weight)]
    entered = 0
    for k in range(60):
        op = ops[rng.integers(len(ops))]
        op(p)
        entered += p.lazy()
        if k % 20 == 19:
            p.check(f"seed {seed} call {k} ({op.__name__})")
    assert entered or MODES[0] != "hip", "no call order reached the lazy state"
    _finish(p, f"seed {seed}")
