"""The trajectory window in CPU mode (include/mbots.h "Trajectory window";
SimManager.trajectory_window): links are identities, the sweeps equal a numpy
float32 restatement bitwise, resets cut lifelines, and nothing the caller does
between steps -- shifts, Prev views, a capacity growth, chained windows, a
second compute -- changes a bit.  4 worlds of 8 agents, windows of 7 to 12
tables, under a breed- and shoot-heavy action stream chosen (seed and length,
tests/traj_util.py) so that the window holds births, deaths and survivors,
which every scenario asserts.  The chained-window, second-compute, shard and
error bodies are tests/traj_util.py's: tests/test_traj_gpu.py runs them on the
device."""
import numpy as np
import pytest
import torch

import traj_util as tu


@pytest.fixture(scope="module")
def plain():
    """The plain run, with and without values: (manager, window) each."""
    return {v: tu.scenario_plain(tu.cpu, v) for v in (False, True)}


@pytest.fixture(scope="module")
def plain_result(plain):
    """Its results at the second parameter set, as numpy copies."""
    return {v: tu.to_numpy(plain[v][1].compute(*tu.PARAMS[1])) for v in (False, True)}


def _expected_worlds(mgr):
    """Each row's world from species_count_tensor alone: species-major, per
    species world-major."""
    c = mgr.species_count_tensor().to_torch().cpu().numpy()
    out = []
    for s in range(4):
        for w in range(c.shape[0]):
            out += [w] * int(c[w, s])
    return np.asarray(out, np.int32)


def test_links_are_identity_without_src_of():
    """HiddenState travels with its agent through the species sort: after each
    push every row writes row + 1 into its column 0 (no shift_observations), so
    after the next step the column names each row's previous row, 0 for a new
    agent.  link must say the same, next must be its exact inverse, and world
    must agree with species_count_tensor and agent_offset_for_world."""
    mgr = tu.cpu()
    stamps, worlds, offsets = [], [], []

    def after_push(m, t):
        h = m.hidden_state_tensor(False).to_torch()
        stamps.append(h[:, 0].numpy().copy())
        worlds.append(_expected_worlds(m))
        offsets.append([m.agent_offset_for_world(w) for w in range(tu.W)])
        h[:, 0] = torch.arange(1, h.shape[0] + 1, dtype=torch.float32)

    win = tu.run_window(mgr, after_push=after_push)
    res = tu.to_numpy(win.compute(1.0))
    tu.assert_scenario(res)
    n = len(res["rows"])
    assert n == tu.STEPS + 1 == win.num_tables
    for t in range(n):
        assert res["rows"][t] == len(stamps[t])
        if t:
            assert np.array_equal(res["link"][t], stamps[t].astype(np.int32) - 1), t
        assert np.array_equal(res["world"][t], worlds[t]), t
        per_world = np.bincount(res["world"][t], minlength=tu.W)
        assert [int(per_world[:w].sum()) for w in range(tu.W)] == offsets[t], t
    for t in range(n - 1):
        nxt, link = res["next"][t], res["link"][t + 1]
        alive = np.nonzero(nxt >= 0)[0]
        assert np.array_equal(link[nxt[alive]], alive), t                  # next then link: back home
        came = np.nonzero(link >= 0)[0]
        assert np.array_equal(nxt[link[came]], came), t                    # link then next: too
        assert len(alive) == len(came) == len(np.unique(link[came])), t    # one successor each


@pytest.mark.parametrize("with_values", [False, True])
@pytest.mark.parametrize("params", tu.PARAMS)
def test_sweep_equals_the_numpy_restatement(plain, params, with_values):
    mgr, win = plain[with_values]
    out = win.compute(*params)
    res = tu.to_numpy(out)
    tu.assert_scenario(res)
    marks = [np.zeros(tu.W, np.int32)] * len(res["rows"])   # an unarmed manager has no resets
    tu.check_against_restatement(res, marks, *params)
    assert (np.concatenate(res["end"][:-1]) != 2).all() and (res["end"][-1] == 3).all()
    if not with_values:
        assert all(not v.any() for v in res["value"])
    for t0 in (0, 3):
        life = win.lifelines(t0).cpu().numpy()
        assert life.dtype == np.int64
        assert np.array_equal(life, tu.lifelines_ref(res["next"], res["rows"], t0))


def test_plain_discounted_return(plain_result):
    """value None and lambda 1: ret is the discounted sum of the rewards after
    the row, along its lifeline (float32, summed from the back as the sweep does)."""
    mgr, win = tu.scenario_plain(tu.cpu, False, steps=6)
    res = tu.to_numpy(win.compute(0.99, 1.0, 0.0))
    life = tu.lifelines_ref(res["next"], res["rows"])
    g = np.float32(0.99)
    for j in range(res["rows"][0]):
        acc = np.float32(0.0)
        rows = [r for r in life[:, j] if r >= 0]
        for t in range(len(rows) - 1, 0, -1):
            acc = np.float32(res["reward"][t][rows[t]] + np.float32(g * acc))
        assert np.float32(res["ret"][0][j]).tobytes() == acc.tobytes(), j


@pytest.mark.parametrize("mode", ["flag", "length"])
def test_resets_cut_lifelines(mode, plain_result):
    mgr, win, marks = tu.scenario_reset(tu.cpu, mode)
    res = tu.to_numpy(win.compute(*tu.PARAMS[1]))
    if mode == "flag":
        tu.assert_scenario(res, marks)
    else:   # every world is reset inside the window: nobody can live through it
        births, deaths, survivors = tu.scenario_facts(res, marks)
        assert births >= 1 and deaths >= 1 and survivors == 0
    tu.check_against_restatement(res, marks, *tu.PARAMS[1])
    n = len(res["rows"])
    reset_tables = [t for t in range(n) if marks[t].any()]
    if mode == "flag":
        assert reset_tables == [tu.RESET_STEP + 1] and list(np.nonzero(marks[tu.RESET_STEP + 1])[0]) == [tu.RESET_WORLD]
    else:   # every world at once: when its age reaches the length, and the step that resets counts as 1
        assert reset_tables == [tu.EPISODE_LENGTH + 1, 2 * tu.EPISODE_LENGTH + 1]
        assert all(marks[t].all() for t in reset_tables)
    for t in range(n - 1):
        cut = marks[t + 1][res["world"][t]] != 0
        assert np.array_equal(res["end"][t] == 2, cut), t          # every row of a reset world, no other
        new = marks[t + 1][res["world"][t + 1]] != 0
        assert (res["link"][t + 1][new] == -1).all(), t
        assert (res["adv"][t][cut] == 0).all()
    if mode == "flag":
        # an agent of a world that is not reset dies in the step that resets another
        t = tu.RESET_STEP
        died = res["world"][t][res["end"][t] == 1]
        assert tu.OTHER_WORLD in died and tu.RESET_WORLD not in died
        # up to the reset the run is the plain one
        ref = plain_result[True]
        for k in ("link", "reward", "world"):
            for u in range(t + 1):
                assert np.array_equal(tu.bits(res[k][u]), tu.bits(ref[k][u]))


def test_shift_and_prev_views_change_nothing(plain_result):
    def before(m, t):
        m.shift_observations()
        for name in ("hidden_state_tensor", "action_tensor", "reward_tensor", "position_tensor", "semantic_tensor"):
            getattr(m, name)(True).to_torch()
    mgr, win = tu.scenario_plain(tu.cpu, True, before_step=before)
    res = tu.to_numpy(win.compute(*tu.PARAMS[1]))
    tu.assert_scenario(res)
    tu.assert_same(res, plain_result[True])


def test_auto_growth_mid_window_changes_nothing():
    a, wa, cap0 = tu.scenario_growth(tu.cpu, "auto")
    b, wb, _ = tu.scenario_growth(tu.cpu, 256)
    assert cap0 == 128 and a.agent_capacity == 256 and a.overflow() == b.overflow() == 0
    ra, rb = tu.to_numpy(wa.compute(*tu.PARAMS[1])), tu.to_numpy(wb.compute(*tu.PARAMS[1]))
    tu.assert_scenario(ra)
    tu.assert_same(ra, rb)


def test_chained_windows_keep_every_transition():
    tu.chained_windows_keep_every_transition(tu.cpu)


def test_compute_twice_gives_the_same_bits(plain, plain_result):
    mgr, win = plain[True]
    tu.compute_twice_gives_the_same_bits(win, plain_result[True])


def test_two_shards_equal_one_manager():
    tu.two_shards_equal_one_manager(tu.cpu)


def test_errors_and_emptying():
    tu.errors_and_emptying(tu.cpu)


def test_a_window_arms_nothing():
    """Opening and pushing leaves the step schedule as it was (no reset pass)."""
    mgr, win = tu.scenario_plain(tu.cpu, False, steps=2)
    info = mgr.schedule_info()
    assert not info["episodes_armed"] and info["steps"] == 2
