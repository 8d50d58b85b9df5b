"""Exact-geometry scenes (tests/scenes.py) in front of the sensor and the K1
finder pass: the same scene is written into the product and the oracle with
set_world_state, and every exported column must stay bitwise equal while the
scene is rendered (a step in which nothing moves), shot at (every finder slot
shows in the stats and health columns), bred in (newborns land on their
parents, inside the crowds) and then evolves under the synthetic stream.

Variants (the launcher's thresholds, csrc/mbots_kernels.hip launch_sensor and
mbots_manager.cpp: K1 finder mode up to 2048 worlds and 256 slots, the split
sensor up to 4096 worlds, mixed classes above 128 slots outside the K1 finder
mode unless MBOTS_MIXED=0):
  A  W = 64,   cap 128 / 256   K1 finder + split-4 sensor
  B  W = 2100, cap 128         split-4 sensor with its own finder
  C  W = 4100, cap 128         one wave per world, 4 worlds per block
  D  W = 2100, cap 256         mixed: the 128-slot kernel + the 256 list kernel
  E  W = 16,   cap 512         64-bit keys: the list kernel (mixed) or 2 worlds per block (MBOTS_MIXED=0)
  F  W = 8,    cap 1024        the list kernel (mixed) or 1 world per block (MBOTS_MIXED=0)
D runs 116 agents per world, not 48: the setter cannot change a population,
and only worlds that breed past 128 agents in step 3 reach the list kernel
while the others stay in the 128-slot one (measured with the oracle: 12 of the
64 scene worlds end above 128 agents, 52 at or below; the test asserts at
least 8 on either side).

Scene (w * stride + offset) % 32 goes into world w of the first and the last
64 worlds (32 and 32 in the large-W variants B, C, D, where each injection is
a checkpoint round trip of the whole manager).  stride = 32 / W where W < 32
(else 1), so the 8 or 16 worlds of the CPU legs and of E and F hold every
family in every case and the offset selects the headings: every kernel sees
every family at n = cap.

Time, measured on an 8-core host with the oracle alone (its seven steps on
8 threads, then building the injected scenes, which is numpy and cached per
(scene, population)): the CPU legs (W = 8, 48 agents, one thread) 0.05 s +
0.2 s; A at n = 128 0.3 s + 1.7 s, at n = 256 1.1 s + 4.1 s, at n = 65 0.1 s +
1.3 s; B 1.8 s + 1.0 s; C 3.6 s + 1.0 s; D (16 threads on the 8 cores) 6.1 s +
1.9 s; E 1.0 s + 1.0 s; F 1.9 s + 0.9 s.  B, C and D inject 32 + 32 worlds to
stay under about 10 s.
"""
import functools
import warnings

import numpy as np
import pytest

import pyoracle as po
import scene_ref
import scenes
from simpair import compare

S = len(scenes.SCENES)


@functools.lru_cache(maxsize=None)
def scene_for(idx, n, seed):
    name, fam, fn = scenes.SCENES[idx % S]
    pos, rot, food = fn(n, np.random.default_rng([seed, idx, n]))
    scenes.check_scene(n, pos, rot, food)
    return pos, rot, food


def _state_equal(g, o):
    return (np.array_equal(g["position"].view(np.int32), o["xy"].view(np.int32)) and
            np.array_equal(g["rotation_wz"].view(np.int32), o["rot"].view(np.int32)) and
            np.array_equal(g["species"], o["species"]) and np.array_equal(g["health"], o["health"]) and
            np.array_equal(g["food"], o["food"]))


def _set_actions(mgr, orc, col):
    a = mgr.action_tensor(False).to_torch()
    a.zero_()
    o = orc.column(po.COL_ACTION)
    o[:] = 0
    if col is not None:
        a[:, col] = 1
        o[:, col] = 1


def _blame(mgr, orc, scene_of):
    """names of the scenes (or "world <w>") whose rows differ in a column"""
    counts, offs = orc.world_counts()
    rows = orc.sensor_index()
    world_of_row = np.zeros(len(rows), np.int64)
    for w in range(len(counts)):
        world_of_row[rows[offs[w]:offs[w] + counts[w]]] = w
    out = {}
    for name, cid in (("semantic_tensor", po.COL_SEMANTIC), ("stats_tensor", po.COL_STATS),
                      ("health_tensor", po.COL_HEALTH), ("position_tensor", po.COL_POS)):
        g = getattr(mgr, name)(False).to_torch().cpu().numpy()
        o = orc.column(cid)
        if g.shape != o.shape:
            continue
        bad = np.nonzero((np.ascontiguousarray(g).view(np.uint8).reshape(len(g), -1) !=
                          np.ascontiguousarray(o).view(np.uint8).reshape(len(o), -1)).any(axis=1))[0]
        for w in np.unique(world_of_row[bad])[:12]:
            out.setdefault(scene_of.get(int(w), f"world {int(w)}"), set()).add(name.split("_")[0])
    return {k: sorted(v) for k, v in out.items()}


def _check(mgr, orc, where, depth_fixed, scene_of=None):
    errs = compare(mgr, orc, where, depth_fixed=depth_fixed)
    assert not errs, "; ".join(errs[:4]) + f" -- scenes: {_blame(mgr, orc, scene_of or {})}"


def run_protocol(mgr, orc, W, depth_fixed, seed=5, offset=0, n_inject=64):
    """The protocol of the module docstring; returns {family: semantic rows
    of its scene worlds after the render step}."""
    for t in range(2):
        for s in (mgr, orc):
            s.write_synthetic_actions(1234, t, True)
            s.step()
            s.shift_observations()
    worlds = sorted(set(range(min(n_inject, W))) | set(range(max(0, W - n_inject), W)))
    fam_of, scene_of = {}, {}
    stride = max(1, S // W)
    idx_of = {w: (w * stride + offset) % S for w in worlds}
    for w in worlds:
        n = len(orc.world_state(w)["xy"])
        name, fam, _ = scenes.SCENES[idx_of[w]]
        pos, rot, food = scene_for(idx_of[w], n, seed + w // S)
        mgr.set_world_state(w, pos, rot, food)
        orc.set_world_state(w, pos, rot, food)
        fam_of[w] = fam
        scene_of[w] = name
    for w in worlds:
        g, o = mgr.world_state(w), orc.world_state(w)
        assert _state_equal(g, o), f"world {w}: world_state differs after set_world_state"
        assert np.array_equal(o["xy"], scene_for(idx_of[w], len(o["xy"]), seed + w // S)[0])
    _check(mgr, orc, "after injection", depth_fixed)
    # 1: nothing moves -- the sensor renders exactly the injected geometry
    _set_actions(mgr, orc, None)
    mgr.step(); orc.step()
    _check(mgr, orc, "render step", depth_fixed, scene_of)
    counts, offs = orc.world_counts()
    rows = orc.sensor_index()
    sem = orc.column(po.COL_SEMANTIC)
    seen = {}
    for w in worlds:
        seen.setdefault(fam_of[w], []).append(sem[rows[offs[w]:offs[w] + counts[w]]].copy())
    for s in (mgr, orc):
        s.shift_observations()
    _check(mgr, orc, "render shift", depth_fixed, scene_of)
    # 2: every agent shoots, 3: every agent breeds, 4-5: the scene evolves
    for t, col in ((2, 4), (3, 5), (4, "syn"), (5, "syn")):
        if col == "syn":
            for s in (mgr, orc):
                s.write_synthetic_actions(1234, t, True)
        else:
            _set_actions(mgr, orc, col)
        mgr.step(); orc.step()
        _check(mgr, orc, f"step {t}", depth_fixed, scene_of)
        for s in (mgr, orc):
            s.shift_observations()
        _check(mgr, orc, f"shift {t}", depth_fixed, scene_of)
    return {f: np.concatenate(v) for f, v in seen.items()}


def assert_not_trivial(seen):
    """per family: some ray sees an agent, one food, one a wall, and in the
    family that is about misses (cameras at and beyond the walls: the only
    place a ray sees nothing at all) a -1"""
    assert set(seen) == {f for f, _ in scenes.FAMILIES}
    for fam, sem in seen.items():
        assert ((sem >= 1) & (sem <= 4)).any(), f"{fam}: no ray sees an agent"
        assert (sem == 6).any(), f"{fam}: no ray sees food"
        assert (sem == 5).any(), f"{fam}: no ray sees a wall"
    assert (seen["walls"] == -1).any(), "walls: no ray misses"


# ---- the catalogue's own float32 placement checks -------------------------------
@pytest.mark.parametrize("n", [4, 9, 65, 127, 128, 256])
def test_catalogue_scenes_are_reachable_states(n):
    """every scene, at every population the variants use, is a state both
    setters accept (solve() has asserted each threshold relation in float32
    while building it)"""
    for idx in range(S):
        pos, rot, food = scene_for(idx, n, 5)
        assert len(pos) == n
        if n >= 65:
            assert len(food) >= 1, scenes.SCENES[idx][0]


def test_catalogue_places_both_sides_of_each_threshold():
    """the solver finds float32 neighbours strictly below and strictly above
    each restated threshold at every heading, and exact equality at least at
    heading (1, 0), where f is a plain difference"""
    for k in scenes.HEADINGS:
        h = scenes.head_of(k)
        cam = (np.float32(40.0), np.float32(40.0))
        for T in (scenes.INSIDE_NEAR, scenes.TOUCH, scenes.CIRCLE_FAR, scenes.FAR_CULL):
            for sgn in (1.0, -1.0):
                for lt in (0.0, 0.92, scenes.wedge_reject_l(float(T), 0.92)):
                    lo = scenes.solve(cam, h, sgn * float(T), lt, scenes.q_absf, T, "lt")
                    hi = scenes.solve(cam, h, sgn * float(T), lt, scenes.q_absf, T, "gt")
                    assert lo is not None and hi is not None
                    f_lo = abs(float(scenes.fl(cam[0], cam[1], h[0], h[1], *lo)[0]))
                    f_hi = abs(float(scenes.fl(cam[0], cam[1], h[0], h[1], *hi)[0]))
                    # within a few float32 steps of the camera's coordinates (ulp(40) = 3.8e-6)
                    assert f_lo < float(T) < f_hi and f_hi - f_lo < 4e-5
        for T in (scenes.FOOD_FAR, scenes.FAR_CULL):
            pts = scenes.three_sides((50, 40), h, float(T), 0.0, scenes.q_absf, T, move="cam")
            assert len(pts) >= 2
        # the wedge (the kernel's own expression and the family's |l| - |f|) and
        # pixel tangency: float32 neighbours on both sides of each line
        for wk in (scenes.WK_DISC, scenes.WK_FOOD):
            for fa in (0.2, 1.0, 5.0, 8.0):
                for sl in (1.0, -1.0):
                    q = scenes.q_wedge(wk)
                    lt = sl * scenes.wedge_reject_l(fa, wk)
                    kept = scenes.solve(cam, h, fa, lt, q, 0.0, "lt")
                    gone = scenes.solve(cam, h, fa, lt, q, 0.0, "gt")
                    assert kept is not None and gone is not None
                    assert float(q(*scenes.fl(cam[0], cam[1], h[0], h[1], *gone))) > 0.0   # rejected in float32
                    assert len(scenes.three_sides(cam, h, -fa, lt, scenes.q_lmf, np.float32(abs(lt) - fa))) >= 2
        for pix in scenes.TANGENT_PIXELS:
            u = float(scenes.ray_u(pix))
            for f in (2.0, 6.0, 30.0):
                f = -f if 24 <= pix < 32 else f
                for sd in (1.0, -1.0):
                    lt = u * f + sd * 0.92 * np.sqrt(1 + u * u)
                    if scenes.solve(cam, h, f, lt) is not None:
                        assert len(scenes.three_sides(cam, h, f, lt, scenes.q_tangent(u, sd), 0.0)) >= 2
    for T in (scenes.CIRCLE_FAR, scenes.FAR_CULL):
        assert scenes.solve((np.float32(40.0), np.float32(40.0)), scenes.head_of(0), float(T), 0.0,
                            scenes.q_absf, T, "eq") is not None
    # the queue family fills the world's food to the cap and packs its crowd
    pos, rot, food = scene_for(16, 128, 5)
    assert scenes.SCENES[16][1] == "queue" and len(food) == 30
    d = np.hypot(*(pos[:8] - pos[:8].mean(0)).T)
    assert d.max() <= 2.0
    # the ties family puts coincident agents into the last slots
    pos, rot, food = scene_for(12, 300, 5)
    assert scenes.SCENES[12][1] == "ties"
    assert (pos[-1] == pos[-2]).all() and np.bincount(food[:, 0]).max() == 5


# ---- round trips: set_world_state(world_state()) is the identity ------------------
def _roundtrip(make, world_state_args):
    a, b = make(), make()
    for t in range(4):
        for s in (a, b):
            s.write_synthetic_actions(1234, t, True)
            s.step()
            s.shift_observations()
    before = [b.world_state(w) for w in range(4)]
    for w in range(4):
        b.set_world_state(w, *world_state_args(before[w]))
    for w in range(4):
        now = b.world_state(w)
        for k in before[w]:
            assert np.array_equal(before[w][k], now[k]), (w, k)
    for t in range(4, 9):
        for s in (a, b):
            s.write_synthetic_actions(1234, t, True)
            s.step()
            s.shift_observations()
    return a, b


def _mgr_args(ws):
    return ws["position"], ws["rotation_wz"], ws["food"]


def test_oracle_set_world_state_roundtrip_and_validation():
    a, b = _roundtrip(lambda: po.OracleSim(4, 69, 32), lambda ws: (ws["xy"], ws["rot"], ws["food"]))
    sa, sb = a.snapshot(), b.snapshot()
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint8), sb[k].view(np.uint8)), k
    args = _assert_rejections(b, lambda w: (lambda ws: (ws["xy"], ws["rot"], ws["food"]))(b.world_state(w)),
                              ValueError)
    _assert_accepts_edges(b, *args)


def _assert_rejections(sim, args_of, exc):
    """every condition of include/mbots.h is refused and changes nothing"""
    pos, rot, food = [np.array(x) for x in args_of(0)]
    ref = sim.world_state(0)

    def bad(p=pos, r=rot, f=food):
        with pytest.raises(exc):
            sim.set_world_state(0, p, r, f)
        now = sim.world_state(0)
        for k in ref:
            assert np.array_equal(ref[k], now[k]), k

    bad(p=pos[:-1], r=rot[:-1])                                    # another population
    for v in (np.nan, np.inf, -0.5, 127.5):
        p = pos.copy(); p[1, 0] = v
        bad(p=p)
    p = pos.copy(); p[0, 1] = 95.5
    bad(p=p)
    r = rot.copy(); r[2] = (1.0, 0.04)                             # |w^2 + z^2 - 1| = 1.6e-3
    bad(r=r)
    r = rot.copy(); r[2, 0] = np.nan
    bad(r=r)
    bad(f=np.array([[0, 1, 1, 0]] * 6, np.int32))                  # 6 in one chunk
    bad(f=np.array([[c, (c % 8) * 16, (c // 8) * 16, 0] for c in range(31)], np.int32))   # 31 in the world
    bad(f=np.array([[0, 16, 1, 0]], np.int32))                     # x outside chunk 0
    bad(f=np.array([[0, 1, -1, 0]], np.int32))
    bad(f=np.array([[48, 1, 1, 0]], np.int32))
    bad(f=np.array([[0, 1, 1, 1 << 22]], np.int32))
    return pos, rot, food


def _assert_accepts_edges(sim, pos, rot, food):
    """the closed ends of the ranges are inside"""
    r = rot.copy(); r[2] = (1.0, 0.02)                             # 4e-4: inside the tolerance
    p = pos.copy(); p[0] = (0.0, 95.0); p[1] = (127.0, 0.0)
    f = np.array([[0, 15, 15, (1 << 22) - 1]] * 5 + [[47, 127, 95, 0]], np.int32)
    sim.set_world_state(0, p, r, f)
    now = sim.world_state(0)
    assert np.array_equal(now["food"], f)


def test_cpu_mode_set_world_state_roundtrip_and_validation(tmp_path):
    import madrona_bots as mb
    a, b = _roundtrip(lambda: mb.SimManager(0, 4, 69, 32, exec_mode="cpu"), _mgr_args)
    orc = po.OracleSim(4, 69, 32)
    for t in range(9):
        orc.write_synthetic_actions(1234, t, True)
        orc.step()
        orc.shift_observations()
    for m in (a, b):
        assert not compare(m, orc, "cpu round trip")
    args = _assert_rejections(b, lambda w: _mgr_args(b.world_state(w)), RuntimeError)
    assert not compare(b, orc, "after the refused calls")
    path = str(tmp_path / "worlds.npz")          # dump_worlds output can be fed back
    a.dump_worlds(path, range(4))
    c = mb.SimManager(0, 4, 69, 32, exec_mode="cpu")
    for t in range(9):                           # (same populations: the same run)
        c.write_synthetic_actions(1234, t, True)
        c.step()
        c.shift_observations()
    c.set_world_state(1, *scene_for(16, len(c.world_state(1)["position"]), 5))
    c.load_worlds(path)
    for w in range(4):
        for k, v in a.world_state(w).items():
            assert np.array_equal(v, c.world_state(w)[k]), (w, k)
    _assert_accepts_edges(b, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("W,cap", [(4, 128), (2100, 256)])
def test_hip_set_world_state_roundtrip_and_validation(W, cap):
    """(2100 worlds at 256 slots: outside the K1 finder mode, mixed classes)"""
    import madrona_bots as mb
    a, b = _roundtrip(lambda: mb.SimManager(0, W, 69, 32, agent_capacity=cap), _mgr_args)
    orc = po.OracleSim(W, 69, 32, cap=cap, num_threads=8)
    for t in range(9):
        orc.write_synthetic_actions(1234, t, True)
        orc.step()
        orc.shift_observations()
    for m in (a, b):
        errs = compare(m, orc, "hip round trip")
        assert not errs, errs[:3]
    args = _assert_rejections(b, lambda w: _mgr_args(b.world_state(w)), RuntimeError)
    errs = compare(b, orc, "after the refused calls")
    assert not errs, errs[:3]
    _assert_accepts_edges(b, *args)


@pytest.mark.gpu
def test_hip_set_world_state_refused_under_capture():
    """a host-side write cannot be recorded into a graph: refused while the
    manager's stream is captured, with the state (and the capture) intact"""
    import madrona_bots as mb
    import torch
    mgr = mb.SimManager(0, 64, 69, 32)
    orc = po.OracleSim(64, 69, 32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for sim in (mgr, orc):
            sim.write_synthetic_actions(1234, 0)
            sim.step(); sim.shift_observations()
            sim.write_synthetic_actions(1234, 1)
        torch.cuda.synchronize()
        args = _mgr_args(mgr.world_state(0))
        with torch.cuda.graph(g, stream=s):
            mgr.step(); mgr.shift_observations(); mgr.write_synthetic_actions(1234, 2)
            with pytest.raises(RuntimeError, match="captured into a graph"):
                mgr.set_world_state(0, *args)
            mgr.step(); mgr.shift_observations(); mgr.write_synthetic_actions(1234, 3)
            mgr.join()
    g.replay()
    for t in (2, 3):
        orc.step(); orc.shift_observations(); orc.write_synthetic_actions(1234, t)
    errs = compare(mgr, orc, "after the replay")
    assert not errs, errs[:3]
    assert _state_equal(mgr.world_state(0), orc.world_state(0))


# ---- the CPU leg: catalogue, both setters and the protocol without a GPU -----------
@pytest.mark.parametrize("offset,fixd", [(0, False), (1, True), (2, False), (3, True)])
def test_scenes_cpu_mode(offset, fixd):
    """W = 8: every family in each case, with offsets 0..3 every scene of the
    catalogue once"""
    import madrona_bots as mb
    mgr = mb.SimManager(0, 8, 69, 48, exec_mode="cpu", fix_depth_alias=fixd)
    orc = po.OracleSim(8, 69, 48)
    seen = run_protocol(mgr, orc, 8, fixd, offset=offset)
    assert_not_trivial(seen)


# ---- the GPU variants ------------------------------------------------------------------
def _gpu_case(monkeypatch, W, cap, A, fixd, mixed_env, offset, n_inject, expect, threads=8):
    import madrona_bots as mb
    if mixed_env is not None:
        monkeypatch.setenv("MBOTS_MIXED", mixed_env)
    mgr = mb.SimManager(0, W, 69, A, agent_capacity=cap, fix_depth_alias=fixd)
    info = mgr.schedule_info()
    for k, v in expect.items():
        assert info[k] == v, (k, info)
    orc = po.OracleSim(W, 69, A, cap=cap, num_threads=threads)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", mb.CapacityWarning)   # n = cap: births are dropped on both sides
        seen = run_protocol(mgr, orc, W, fixd, offset=offset, n_inject=n_inject)
    assert mgr.overflow() == orc.overflow()
    assert_not_trivial(seen)
    return mgr, orc


K1 = dict(k1_finder=True, mixed_classes=False)
A_CASES = [(128, 128, False), (128, 128, True), (128, 127, True), (128, 65, False), (128, 9, True),
           (128, 4, False), (256, 256, False), (256, 256, True), (256, 255, False), (256, 65, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("cap,A,fixd", A_CASES, ids=[f"A-k1finder-split4-cap{c}-n{a}-{'depth' if d else 'alias'}"
                                                     for c, a, d in A_CASES])
def test_scenes_variant_a(monkeypatch, cap, A, fixd):
    _gpu_case(monkeypatch, 64, cap, A, fixd, None, 0, 64, K1)


@pytest.mark.gpu
def test_scenes_variant_b_split4_own_finder(monkeypatch):
    _gpu_case(monkeypatch, 2100, 128, 48, False, None, 0, 32, dict(k1_finder=False, mixed_classes=False))


@pytest.mark.gpu
@pytest.mark.parametrize("fixd", [False, True], ids=["C-wave-per-world-alias", "C-wave-per-world-depth"])
def test_scenes_variant_c(monkeypatch, fixd):
    _gpu_case(monkeypatch, 4100, 128, 48, fixd, None, 0, 32, dict(k1_finder=False, mixed_classes=False))


@pytest.mark.gpu
def test_scenes_variant_d_mixed_128_and_256_list(monkeypatch):
    mgr, orc = _gpu_case(monkeypatch, 2100, 256, 116, False, None, 0, 32,
                         dict(k1_finder=False, mixed_classes=True), threads=16)
    counts, _ = orc.world_counts()
    injected = np.r_[counts[:32], counts[-32:]]
    # scene worlds on both sides of the 128 line: both kernels rendered scenes
    assert (injected > 128).sum() >= 8 and (injected <= 128).sum() >= 8, injected


E_CASES = [(512, "1", 0), (512, "0", 1), (511, "0", 0), (65, "1", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("A,mixed,offset", E_CASES,
                         ids=[f"E-cap512-n{a}-{'list512' if m == '1' else '2-worlds-per-block'}-scenes{o}"
                              for a, m, o in E_CASES])
def test_scenes_variant_e(monkeypatch, A, mixed, offset):
    _gpu_case(monkeypatch, 16, 512, A, False, mixed, offset, 64, dict(k1_finder=False, mixed_classes=mixed == "1"))


F_CASES = [(1024, "1", 0), (1024, "0", 1), (1024, "1", 2), (1024, "0", 3), (1023, "0", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("A,mixed,offset", F_CASES,
                         ids=[f"F-cap1024-n{a}-{'list1024' if m == '1' else '1-world-per-block'}-scenes{o}"
                              for a, m, o in F_CASES])
def test_scenes_variant_f(monkeypatch, A, mixed, offset):
    _gpu_case(monkeypatch, 8, 1024, A, False, mixed, offset, 64, dict(k1_finder=False, mixed_classes=mixed == "1"))


# ---- float64: the oracle composites the crowded scenes correctly ----------------------------
REF_FAMILIES = [f for f, _ in scenes.FAMILIES if f not in scenes.BOUNDARY_FAMILIES]


@pytest.mark.parametrize("family", REF_FAMILIES)
def test_oracle_matches_float64_renderer(family):
    """The oracle's post-step world_state of each scene of the family (four
    headings, 40 agents), rendered in float64: the semantic class of every ray
    not skipped for being on a decision boundary is the oracle's.  At most
    10 % of the family's rays may be skipped."""
    idxs = [i for i, s in enumerate(scenes.SCENES) if s[1] == family]
    orc = po.OracleSim(len(idxs), 69, 40)
    for t in range(2):
        orc.write_synthetic_actions(1234, t, True)
        orc.step()
        orc.shift_observations()
    for w, idx in enumerate(idxs):
        n = len(orc.world_state(w)["xy"])
        orc.set_world_state(w, *scene_for(idx, n, 5))
    orc.column(po.COL_ACTION)[:] = 0
    orc.step()
    counts, offs = orc.world_counts()
    rows = orc.sensor_index()
    sem = orc.column(po.COL_SEMANTIC)
    total = checked = 0
    for w, idx in enumerate(idxs):
        ws = orc.world_state(w)
        want, skip = scene_ref.render_scene(ws["xy"], ws["rot"], ws["species"], ws["food"])
        got = sem[rows[offs[w]:offs[w] + counts[w]]].astype(np.int64)
        ok = ~skip
        bad = np.argwhere(ok & (want != got))
        assert len(bad) == 0, (scenes.SCENES[idx][0], bad[:5], want[ok & (want != got)][:5],
                               got[ok & (want != got)][:5])
        total += skip.size
        checked += int(ok.sum())
    print(f"{family}: {checked} of {total} rays checked")
    assert checked >= 0.9 * total, (family, checked, total)
