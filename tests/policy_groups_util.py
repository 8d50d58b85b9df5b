"""TEST INFRASTRUCTURE shared by the policy-group tests (DESIGN.md "Policy
groups"): the shapes at which the segment logic can go wrong, managers and
mixed-architecture nets per group built from the helpers of
tests/test_policy_cpu.py, the numpy statement of policy_segments(), and the
float64 restatement per group.  Not a product path."""
import numpy as np
import torch

import policy_ref as pr
import test_policy_cpu as tp

# shape: (worlds, agents per world), starts
SHAPES = {
    "A": ((3, 5), [0, 1, 2]),                     # every segment under one tile
    "B": ((40, 32), [0, 1, 17, 39]),              # groups of 1 / 16 / 22 / 1 worlds
    "C": ((40, 32), [0, 2, 100]),                 # a group with no local world
    "D": ((130, 8), list(range(0, 128, 2))),      # the largest table: 64 groups, 260 segments
}
# the architectures mixed across groups (cases of test_policy_cpu.GRID; the
# two world keys only give two different sets of weights per architecture)
SMALL, BIG = (16, 1, False, False), (128, 4, True, True)
CASES = [("3x5",) + SMALL, ("3x5",) + BIG, ("40x32",) + SMALL, ("40x32",) + BIG]


def make_sim(shape, exec_mode="cpu", starts=True, **kw):
    """tp.make_sim for a shape of SHAPES, with the shape's groups set."""
    import madrona_bots as mb
    (W, A), st = SHAPES[shape]
    sim = mb.SimManager(0, W, tp.SEED, A, exec_mode=exec_mode, **kw)
    for t in range(3):
        sim.write_synthetic_actions(4321, t, True)
        sim.step()
    if starts:
        sim.set_policy_groups(st)
    return sim


def make_group_nets(sim, n_groups, first=0):
    """nets[g]: four make_net() dicts, the architecture cycling through CASES
    from `first` (so neighbouring groups differ in H, depth, activations,
    memory head and memory_in)."""
    x85 = pr.inputs(sim, True)
    sets = {}
    for case in CASES:
        sets[case] = tp.make_nets(case, x85 if case[3] else np.ascontiguousarray(x85[:, :69]))
    return [sets[CASES[(first + g) % len(CASES)]] for g in range(n_groups)]


def set_group_nets(sim, nets, groups=None):
    """Upload nets[g] to group g (one PolicyNet object per distinct net)."""
    made = {}
    for g, four in enumerate(nets):
        if groups is not None and g not in groups:
            continue
        sim.set_policy([made.setdefault(id(n), pr.policy_net(n, sim.device)) for n in four], group=g)


def world_group(starts, gw):
    return np.searchsorted(np.asarray(starts), gw, side="right") - 1


def needed_groups(starts, lo, hi):
    """The groups that own a world of [lo, hi)."""
    return sorted(set(world_group(starts, np.arange(lo, hi)).tolist()))


def segments_numpy(sc, starts, world_offset=0):
    """policy_segments() from species_count_tensor(): int32 [G, 4, 2]."""
    sc = np.asarray(sc).astype(np.int64)
    W = sc.shape[0]
    first = [min(max(int(s) - world_offset, 0), W) for s in starts] + [W]
    out = np.zeros((len(starts), 4, 2), np.int32)
    base = 0
    for s in range(4):
        cum = np.concatenate([[0], np.cumsum(sc[:, s])])
        for g in range(len(starts)):
            out[g, s] = (base + cum[first[g]], base + cum[first[g + 1]])
        base += cum[W]
    return out


def reference(nets, sim, starts, world_offset=0):
    """tp.reference over a grouped table: float64 and torch-f32 logits, value
    and memory of every exported row through the net of its (group, species),
    and has_mem [N]: the row's net has a memory head."""
    sc = sim.species_count_tensor().to_torch().cpu().numpy()
    gw, sp, _ = pr.row_keys(sc, world_offset)
    x85 = pr.inputs(sim, True)
    n = len(gw)
    r64 = (np.zeros((n, 6)), np.zeros(n), np.zeros((n, 16)))
    r32 = (np.zeros((n, 6)), np.zeros(n), np.zeros((n, 16)))
    has_mem = np.zeros(n, bool)
    rg = world_group(starts, gw)
    wg = world_group(starts, world_offset + np.arange(sc.shape[0]))
    for g in np.unique(rg):
        rows = np.nonzero(rg == g)[0]
        sc_g = np.where((wg == g)[:, None], sc, 0)
        mi = nets[g][0]["memory_in"]
        x = x85[rows] if mi else np.ascontiguousarray(x85[rows, :69])
        a64, a32 = tp.reference(nets[g], x, sc_g)
        for dst, src in ((r64, a64), (r32, a32)):
            for d, s_ in zip(dst, src):
                d[rows] = s_
        has_mem[rows] = nets[g][0]["memory"] is not None
    return r64, r32, has_mem


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def assert_same_outputs(o_a, o_b, where):
    for k in ("action", "logp", "value"):
        a, b = bits(o_a[k]), bits(o_b[k])
        assert a.shape == b.shape, (where, k, a.shape, b.shape)
        bad = np.nonzero(a != b)[0]
        assert not len(bad), (where, k, len(bad), int(bad[0]), o_a[k][bad[0]].item(), o_b[k][bad[0]].item())


def by_world(m, off):
    """Every (global world, species)'s rows of the columns act() and step()
    touch, and every world's state: what two shards must share with one."""
    sc = m.species_count_tensor().to_torch().cpu().numpy()
    cols = {k: getattr(m, k)().to_torch().cpu().numpy()
            for k in ("reward_tensor", "action_tensor", "hidden_state_tensor", "position_tensor")}
    out, row = {}, 0
    for s in range(4):
        for w in range(sc.shape[0]):
            n = int(sc[w, s])
            out[(off + w, s)] = {k: v[row:row + n].copy() for k, v in cols.items()}
            row += n
    return out, {off + w: m.world_state(w) for w in range(sc.shape[0])}
