"""CPU: the oracle reproduces the committed golden vectors, and the boundary
shapes match what the reference's own files pin (tests/golden/make_golden.py)."""
import json
import os

import numpy as np
import pytest

import pyoracle as po
from golden_util import FIXTURES, NAMES, REF_FIXTURES, load_fixture, run_digests, run_digests_manager

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", [f[0] for f in FIXTURES])
def test_oracle_reproduces_golden(name):
    meta, arrays = load_fixture(name)
    sim = po.OracleSim(meta["worlds"], meta["seed"], meta["agents"], cap=meta["cap"],
                       reward_fixed=meta["reward_fixed"])
    log = run_digests(sim, meta)
    for (tag, n, dg), (tag2, n2, dg2) in zip(meta["log"], log):
        assert tag == tag2 and n == n2, (tag, n, n2)
        bad = [k for k in dg if dg[k] != dg2[k]]
        assert not bad, f"{name} {tag}: columns differ: {bad}"


def _same_log(name, want, got, skip=()):
    assert len(want) == len(got)
    for (tag, n, dg), (tag2, n2, dg2) in zip(want, got):
        assert tag == tag2 and n == n2, (name, tag, n, n2)
        bad = [k for k in dg if dg[k] != dg2[k] and not any(s in k for s in skip)]
        assert not bad, f"{name} {tag}: columns differ from the reference's recorded output: {bad}"


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_oracle_reproduces_reference_output(name):
    """reference_*.npz hold what the reference's own simulation code computed
    on the stand-in engine (meta["side"]); the oracle alone, replaying the run,
    must give the same digests after every step and shift and the same final
    tables -- also where that library cannot be built."""
    meta, arrays = load_fixture(name)
    assert meta["side"].startswith("the reference's sim.cpp")
    sim = po.OracleSim(meta["worlds"], meta["seed"], meta["agents"], cap=meta["cap"])
    _same_log(name, meta["log"], run_digests(sim, meta))
    assert sim.overflow() == 0
    for i, nm in enumerate(NAMES):
        for prev in (False, True):
            want = arrays[("prev_" if prev else "") + nm]
            assert np.array_equal(sim.column(i, prev).view(np.uint8), want.view(np.uint8)), (nm, prev)
    assert np.array_equal(sim.species_count(), arrays["species_count"])
    # the reference's own SpeciesCount is the one before the respawns (B.5)
    assert np.array_equal(np.maximum(arrays["species_count_before_respawn"], meta["agents"] // 4),
                          arrays["species_count"])


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_cpu_mode_reproduces_reference_output(name):
    """The product's host path (exec_mode="cpu") against the same records."""
    import madrona_bots as mb
    meta, arrays = load_fixture(name)
    mgr = mb.SimManager(0, meta["worlds"], meta["seed"], meta["agents"], exec_mode="cpu",
                        agent_capacity=meta["cap"])
    log, get = run_digests_manager(mgr, meta)
    _same_log(name, meta["log"], log, skip=("depth",))
    for nm in NAMES:
        if nm != "depth":
            assert np.array_equal(get(nm, False).view(np.uint8), arrays[nm].view(np.uint8)), nm
    assert mgr.overflow() == 0


def test_reference_boundary_shapes():
    ref = json.load(open(os.path.join(HERE, "golden", "reference_shapes.json")))
    # learn/env.py:19 obs = depth 32 + health 1 + position 2 + semantic 32 + surrounding 2
    assert ref["obs_dim"] == [32 + 1 + 2 + 32 + 2]
    assert ref["action_dim"] == [6]
    sim = po.OracleSim(2, 69, 32)
    widths = {c: sim.column(c).shape[1] for c in range(10)}
    assert widths[po.COL_DEPTH] + widths[po.COL_HEALTH] + widths[po.COL_POS] + \
        widths[po.COL_SEMANTIC] + widths[po.COL_SURROUND] == ref["obs_dim"][0]
    assert widths[po.COL_ACTION] == ref["action_dim"][0]
    # sensor objects: food the +-1 cube; agents the agent mesh's cross-section
    # in the rays' plane (z = 0 of the mesh: the camera sits at the agent's
    # centre), radii 0.910-0.921 -> the spec's disc of radius 0.92, which the
    # near sphere 1.1 (mgr.cpp:133) clears, so a camera never sees its own body
    ext = ref["mesh_abs_extent"]
    assert 1.0 <= ext["agent_render.obj"] <= 1.2 and ext["cube_render.obj"] == 1.0
    lo, hi = ref["agent_section_z0_radii"]
    assert lo <= 0.92 and abs(hi - 0.92) < 1e-3 and hi < 1.1


def test_golden_final_tables_consistent():
    meta, arrays = load_fixture("oracle_w4_a32_s69")
    sc = arrays["species_count"]
    assert sc.sum() == arrays["species"].shape[0]
    assert (np.diff(arrays["species"].ravel()) >= 0).all()
