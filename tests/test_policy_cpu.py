"""CPU mode: the device actor (DESIGN.md "Device actor"; SimManager.set_policy
/ act) against the float64 restatement of tests/policy_ref.py -- its
activations, the forward pass, the sampled and the greedy actions, its
equivalence with the construct_obs -> net -> write_actions sequence, the draw
counter, the refusals and shards."""
import numpy as np
import pytest
import torch

import policy_ref as pr
from simpair import compare
import pyoracle

SEED = 77
WORLDS = {"3x5": (3, 5), "40x32": (40, 32)}     # under one tile / many tiles, species boundaries inside
                                                 # tiles, ragged last tiles
GRID = [(wk, H, depth, mi, mh) for wk in WORLDS for H in (16, 48, 128) for depth in (1, 4)
        for mi in (False, True) for mh in (False, True)]


def grid_id(c):
    return f"{c[0]}-H{c[1]}-d{c[2]}-{'min' if c[3] else 'nomin'}-{'mem' if c[4] else 'nomem'}"


def make_sim(case, exec_mode="cpu", **kw):
    """A manager a few steps into its run (observations, rewards and a
    non-zero HiddenState in place)."""
    import madrona_bots as mb
    W, A = WORLDS[case[0]]
    sim = mb.SimManager(0, W, SEED, A, exec_mode=exec_mode, **kw)
    for t in range(3):
        sim.write_synthetic_actions(4321, t, True)
        sim.step()
    return sim


def make_nets(case, x):
    """Four different random nets for a grid case; every activation code is
    used across the grid (and inside every depth-4 case)."""
    _, H, depth, mi, mh = case
    idx = GRID.index(case)
    rng = np.random.default_rng(1000 + idx)
    return [pr.calibrate_actor(pr.make_net(rng, H, depth, [(idx + s + l) % 6 for l in range(depth)], mi, mh,
                                           pr.in_scale(x)), x) for s in range(4)]


def reference(nets, x, sc):
    """float64 and torch-f32 forward of every row through its species' net."""
    _, sp, _ = pr.row_keys(sc)
    n = len(sp)
    z64, v64, m64 = np.zeros((n, 6)), np.zeros(n), np.zeros((n, 16))
    z32, v32, m32 = np.zeros((n, 6)), np.zeros(n), np.zeros((n, 16))
    for s in range(4):
        rows = np.nonzero(sp == s + 1)[0]
        if not len(rows):
            continue
        for (z, v, m), f in (((z64, v64, m64), pr.forward64), ((z32, v32, m32), pr.forward_torch32)):
            a, b, c = f(nets[s], x[rows])
            z[rows], v[rows] = a, b
            if c is not None:
                m[rows] = c
    return (z64, v64, m64), (z32, v32, m32)


def test_grid_uses_every_activation():
    used = set()
    for c in GRID:
        idx = GRID.index(c)
        used |= {(idx + s + l) % 6 for s in range(4) for l in range(c[2])}
    assert used == set(range(6))


# ---- 1. activations -------------------------------------------------------
def sweep():
    x = np.concatenate([np.linspace(-30.0, 30.0, 2_000_001), np.linspace(-1e-3, 1e-3, 100_001),
                        np.linspace(-0.5, 0.5, 200_001), np.array([0.0, -0.0, 1e-30, -1e-30, 1e-41, -1e-41])])
    return x.astype(np.float32)


def ulps(y, ref):
    a = np.maximum(np.abs(ref).astype(np.float32), np.float32(1.1754944e-38))
    return np.abs(y.astype(np.float64) - ref) / np.spacing(a).astype(np.float64)


def test_activation_sweep_within_4_ulp():
    """Each activation, exp on (-inf, 0] and log on [1, 7] within 4 ulp of
    float64 over ~2.3 M points (measured maxima are recorded in DESIGN.md)."""
    import madrona_bots as mb
    x = sweep()
    x64 = x.astype(np.float64)
    for code, name in pr.CODES.items():
        y = mb.policy_activation(name, torch.from_numpy(x)).numpy()
        e = ulps(y, pr.act64(code, x64))
        print(f"{name}: max {e.max():.3f} ulp at x = {x[e.argmax()]!r}")
        assert e.max() <= 4.0, (name, e.max(), x[e.argmax()])
    xe = np.concatenate([-np.abs(x), -np.linspace(30.0, 104.0, 400_001).astype(np.float32),
                         np.array([-np.inf], np.float32)])
    e = ulps(mb.policy_activation("exp", torch.from_numpy(xe)).numpy(), np.exp(xe.astype(np.float64)))
    print(f"exp: max {e.max():.3f} ulp at x = {xe[e.argmax()]!r}")
    assert e.max() <= 4.0
    xl = np.linspace(1.0, 7.0, 2_000_001).astype(np.float32)
    e = ulps(mb.policy_activation("log", torch.from_numpy(xl)).numpy(), np.log(xl.astype(np.float64)))
    print(f"log: max {e.max():.3f} ulp at x = {xl[e.argmax()]!r}")
    assert e.max() <= 4.0


# ---- 2. / 3. forward and sampled actions ------------------------------------
@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_forward_and_sampling_against_float64(case):
    """value, logp and the new HiddenState within tol = 8 x torch-f32's own
    largest error against float64; the sampled action equals the restatement's
    except where u lies within 4 tol of a CDF edge (at most 1 % of rows); every
    action is taken by >= 2 % of the draws (the 15-row case pools 40 draws of
    the same table, so that 2 % is not less than one row)."""
    sim = make_sim(case)
    x = pr.inputs(sim, case[3])
    nets = make_nets(case, x)
    sim.set_policy([pr.policy_net(n) for n in nets])
    sc = sim.species_count_tensor().to_torch().numpy()
    gw, sp, k = pr.row_keys(sc)
    (z64, v64, m64), (z32, v32, m32) = reference(nets, x, sc)
    hidden_before = sim.hidden_state_tensor().to_torch().numpy().copy()
    sim.policy_draw = 11
    o = sim.act()
    a, logp, value = (o[q].numpy()[:, 0] for q in ("action", "logp", "value"))
    lp64, lp32 = pr.logp64(z64), pr.logp64(z32)
    has_mem = case[4]
    err32 = max(np.abs(v32 - v64).max(), np.abs(lp32 - lp64).max(), np.abs(m32 - m64).max() if has_mem else 0.0)
    tol = 8.0 * err32
    a64, dist = pr.sample64(z64, pr.uniforms(SEED, 11, gw, sp, k))
    rows = np.arange(len(a))
    e_v = np.abs(value - v64).max()
    e_lp = np.abs(logp - lp64[rows, a]).max()
    hid = sim.hidden_state_tensor().to_torch().numpy()
    e_m = np.abs(hid - m64).max() if has_mem else 0.0
    print(f"tol {tol:.3g} (torch f32 {err32:.3g}); value {e_v:.3g} logp {e_lp:.3g} memory {e_m:.3g}")
    assert tol > 0 and e_v <= tol and e_lp <= tol and e_m <= tol
    if not has_mem:
        assert np.array_equal(hid.view(np.uint32), hidden_before.view(np.uint32))
    exempt = dist <= 4.0 * tol
    assert exempt.mean() <= 0.01
    assert np.array_equal(a[~exempt], a64[~exempt])
    onehot = sim.action_tensor().to_torch().numpy()
    assert np.array_equal(onehot, (np.arange(6)[None, :] == a[:, None]).astype(np.int32))
    # no saturated softmax: it would hide a sampling bug
    acts = [a]
    if len(a) < 300:
        acts += [sim.act(write=False)["action"].numpy()[:, 0] for _ in range(39)]
    share = np.bincount(np.concatenate(acts), minlength=6) / sum(len(q) for q in acts)
    assert share.min() >= 0.02, share


# ---- 4. greedy ------------------------------------------------------------
def test_greedy_is_first_argmax_with_a_crafted_tie():
    case = ("40x32", 48, 1, False, False)
    sim = make_sim(case)
    x = pr.inputs(sim, False)
    nets = make_nets(case, x)
    for n in nets:   # actor rows 1 and 4 duplicate row 3: wherever that logit is the largest, 1 wins
        w, b = n["actor"][1]
        w[1], w[4], b[1], b[4] = w[3], w[3], b[3], b[3]
    sim.set_policy([pr.policy_net(n) for n in nets])
    (z64, _, _), _ = reference(nets, x, sim.species_count_tensor().to_torch().numpy())
    a = sim.act(greedy=True)["action"].numpy()[:, 0]
    assert not np.isin(a, (3, 4)).any() and (a == 1).sum() > 10
    clear = np.sort(z64, axis=1)
    clear = (clear[:, -1] - clear[:, -2] > 1e-4) | (z64.argmax(axis=1) == 1)
    assert clear.mean() > 0.9 and np.array_equal(a[clear], z64.argmax(axis=1)[clear])
    b = sim.act(greedy=True)["action"].numpy()[:, 0]
    assert np.array_equal(a, b)       # greedy does not depend on the draw


# ---- 5. equivalence with construct_obs -> net -> write_actions -------------------
class _AsOracle:
    """A manager behind the oracle's reading surface, for simpair.compare."""
    COLS = {pyoracle.COL_SPECIES: "species_tensor", pyoracle.COL_POS: "position_tensor",
            pyoracle.COL_HEALTH: "health_tensor", pyoracle.COL_SURROUND: "surrounding_tensor",
            pyoracle.COL_REWARD: "reward_tensor", pyoracle.COL_ACTION: "action_tensor",
            pyoracle.COL_STATS: "stats_tensor", pyoracle.COL_HIDDEN: "hidden_state_tensor",
            pyoracle.COL_SEMANTIC: "semantic_tensor"}

    def __init__(self, m):
        self.m = m

    def num_agents(self):
        return self.m.num_agents()

    def species_count(self):
        return self.m.species_count_tensor().to_torch().cpu().numpy()

    def column(self, cid, is_prev=False):
        return getattr(self.m, self.COLS[cid])(is_prev).to_torch().cpu().numpy()


def run_equivalence(exec_mode, pattern, case=("40x32", 48, 4, True, True)):
    a, b = make_sim(case, exec_mode), make_sim(case, exec_mode)
    nets = make_nets(case, pr.inputs(a, case[3]))
    a.set_policy([pr.policy_net(n, a.device) for n in nets])
    for t in range(6):
        if pattern == "reset" and t == 2:
            a.reset_worlds([1, 7])
            b.reset_worlds([1, 7])
        if pattern == "grow" and t == 3:
            a.grow_capacity(256)
            b.grow_capacity(256)
        before = (a.action_tensor().to_torch().clone(), a.hidden_state_tensor().to_torch().clone())
        o = a.act(write=False)
        assert torch.equal(before[0], a.action_tensor().to_torch())
        assert torch.equal(before[1].view(torch.int32), a.hidden_state_tensor().to_torch().view(torch.int32))
        a.policy_draw = t
        o2 = a.act()
        assert a.policy_draw == t + 1
        act, mem = a.action_tensor().to_torch().clone(), a.hidden_state_tensor().to_torch().clone()
        assert torch.equal(act, (torch.arange(6, device=act.device)[None, :] == o2["action"]).to(torch.int32))
        b.write_actions(act, mem)
        for m in (a, b):
            m.step()
            if pattern == "shift":
                m.shift_observations()
            elif pattern == "shift4":
                for _ in range(4):
                    m.shift_observations()
        errs = compare(a, _AsOracle(b), f"{pattern} step {t}")
        assert not errs, errs[:4]


@pytest.mark.parametrize("pattern", ["plain", "shift", "shift4", "reset", "grow"])
def test_act_equals_three_call_sequence(pattern):
    run_equivalence("cpu", pattern)


# ---- 6. draw counter and misuse ---------------------------------------------
def test_draw_counter_and_misuse():
    import madrona_bots as mb
    nn = torch.nn
    case = ("40x32", 16, 1, False, False)
    sim = make_sim(case)
    nets = [pr.policy_net(n) for n in make_nets(case, pr.inputs(sim, False))]
    with pytest.raises(RuntimeError, match="no policy net"):
        sim.act()
    sim.set_policy(nets[0], species=1)
    sim.set_policy(nets[1], species=2)
    sim.set_policy(nets[2], species=3)
    with pytest.raises(RuntimeError, match="species 4 has no policy net"):
        sim.act()
    sim.set_policy(nets[3], species=4)
    assert sim.policy_draw == 0
    first = sim.act(write=False)
    second = sim.act(write=False)
    assert sim.policy_draw == 2
    assert not torch.equal(first["action"], second["action"])
    assert torch.equal(first["value"], second["value"])
    sim.policy_draw = 0
    again = sim.act(write=False)
    assert all(torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)) for k in first)
    # widths
    def stack(h_in=69, H=16, n_act=6):
        return (nn.Sequential(nn.Linear(h_in, H), nn.Tanh()), nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, n_act)),
                nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1)))
    mb.PolicyNet.from_torch(*stack())
    for kw, msg in ((dict(H=24), "multiple of 16"), (dict(H=144), "multiple of 16"), (dict(h_in=70), r"\[16, 69\]"),
                    (dict(n_act=5), "6 outputs")):
        with pytest.raises(ValueError, match=msg):
            mb.PolicyNet.from_torch(*stack(**kw))
    f, a, c = stack()
    with pytest.raises(ValueError, match=r"feature\[1\] \(GELU\)"):
        mb.PolicyNet.from_torch(nn.Sequential(f[0], nn.GELU()), a, c)
    with pytest.raises(ValueError, match=r"feature\[1\] \(GRU\)"):
        mb.PolicyNet.from_torch(nn.Sequential(f[0], nn.GRU(16, 16)), a, c)
    with pytest.raises(ValueError, match="one at most"):
        mb.PolicyNet.from_torch(nn.Sequential(f[0], nn.Tanh(), nn.ReLU()), a, c)
    with pytest.raises(ValueError, match="LeakyReLU"):
        mb.PolicyNet.from_torch(nn.Sequential(f[0], nn.LeakyReLU(0.2)), a, c)
    with pytest.raises(ValueError, match="memory"):
        mb.PolicyNet.from_torch(f, a, c, memory=nn.Sequential(nn.Linear(16, 8), nn.Tanh()))
    # the library checks for itself: a hand-made net of a bad width
    w = torch.zeros
    bad = mb.PolicyNet([(w(16, 69), None, 0)], [(w(16, 16), None, 0), (w(6, 16), None, 0)],
                       [(w(16, 16), None, 0), (w(2, 16), None, 0)])
    with pytest.raises(RuntimeError, match="critic"):
        sim.set_policy(bad, species=1)
    assert torch.equal(sim.act(write=False)["value"], sim.act(write=False)["value"])   # the old net is in place


def test_reference_shaped_stack_loads_unchanged():
    """The reference's feature stack -- Linear(69, 128), Linear(128, 128), Tanh,
    Linear(128, 128), ReLU -- maps to trunk codes 0, 3, 1."""
    import madrona_bots as mb
    nn = torch.nn
    torch.manual_seed(3)
    feature = nn.Sequential(nn.Linear(69, 128), nn.Linear(128, 128), nn.Tanh(), nn.Linear(128, 128), nn.ReLU())
    actor = nn.Sequential(nn.Linear(128, 128), nn.ReLU(True), nn.Linear(128, 6))
    critic = nn.Sequential(nn.Linear(128, 128), nn.ReLU(True), nn.Linear(128, 1))
    net = mb.PolicyNet.from_torch(feature, actor, critic)
    assert [c for _, _, c in net.trunk] == [0, 3, 1]
    sim = make_sim(("3x5", 128, 4, False, False))
    with torch.no_grad():
        feature[0].weight.mul_(0.01)
    sim.set_policy(net)
    o = sim.act()
    with torch.no_grad():
        h = feature(sim.construct_obs())
        v = critic(h)
        lp = torch.log_softmax(actor(h), dim=1).gather(1, o["action"].long())
    assert torch.allclose(o["value"], v, atol=1e-4, rtol=1e-4) and torch.allclose(o["logp"], lp, atol=1e-4, rtol=1e-4)


# ---- 7. shards --------------------------------------------------------------
def test_two_shards_under_act_equal_one_manager():
    import madrona_bots as mb
    W, A = 8, 16
    whole = mb.SimManager(0, W, SEED, A, exec_mode="cpu")
    shards = [mb.SimManager(0, W // 2, SEED, A, exec_mode="cpu", world_offset=0, shard_ghost=True),
              mb.SimManager(0, W // 2, SEED, A, exec_mode="cpu", world_offset=W // 2)]
    case = ("40x32", 48, 4, True, True)
    nets = make_nets(case, np.abs(np.random.default_rng(0).normal(0, 30, (64, 85))).astype(np.float32))
    for m in [whole] + shards:
        m.set_policy([pr.policy_net(n) for n in nets])
    taken = np.zeros(6)
    for t in range(6):
        for m in [whole] + shards:
            o = m.act()
            m.step()
        taken += np.bincount(o["action"].numpy().ravel(), minlength=6)
    assert (taken > 0).sum() >= 3

    def by_world(m, off):
        sc = m.species_count_tensor().to_torch().numpy()
        cols = {k: getattr(m, k)().to_torch().numpy() for k in ("reward_tensor", "action_tensor", "hidden_state_tensor",
                                                                "position_tensor")}
        out, row = {}, 0
        for s in range(4):
            for w in range(sc.shape[0]):
                n = int(sc[w, s])
                out[(off + w, s)] = {k: v[row:row + n].copy() for k, v in cols.items()}
                row += n
        states = {off + w: m.world_state(w) for w in range(sc.shape[0])}
        return out, states
    full, full_states = by_world(whole, 0)
    for m, off in zip(shards, (0, W // 2)):
        part, states = by_world(m, off)
        for key, cols in part.items():
            for k, v in cols.items():
                assert np.array_equal(v.view(np.uint32), full[key][k].view(np.uint32)), (key, k)
        for w, st in states.items():
            for k in st:
                assert np.array_equal(np.asarray(st[k]), np.asarray(full_states[w][k])), (w, k)
