"""bench.py --dump-outputs: the dump of the exported columns after the bench's
own loop (here on the CPU execution mode, bit-identical to the HIP path) is
float32 / float64 .npy files, samples the same rows of every column, and is
identical from run to run."""
import os

import numpy as np

import bench

COLS = ["species", "position", "health", "surrounding", "reward", "action", "stats", "hidden_state",
        "semantic"]


def _run(path, worlds=8, steps=6):
    import madrona_bots as mb
    m = mb.SimManager(0, worlds, bench.SEED, bench.AGENTS_PER_WORLD, exec_mode="cpu")
    m.write_synthetic_actions(bench.ACTION_SEED, 0)
    for t in range(steps):
        m.step()
        m.shift_observations()
        m.write_synthetic_actions(bench.ACTION_SEED, t + 1)
    names = bench.dump_outputs(m, str(path))
    full = {c: getattr(m, c + "_tensor")(False).to_torch().numpy().copy() for c in COLS}
    return m.num_agents(), names, {n: np.load(os.path.join(path, n + ".npy")) for n in names}, full


def test_dump_outputs_sampled_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROWS", 100)   # 8 worlds hold > 100 agents: the sampled path
    n, names, a, full = _run(tmp_path / "a")
    _, _, b, _ = _run(tmp_path / "b")
    assert n > 100
    assert set(names) == {"num_agents", "rows", "species_count"} | {p + c for c in COLS for p in ("", "prev_")}
    rows = a["rows"].astype(np.int64)
    assert len(rows) == 100 and len(set(rows)) == 100 and (np.diff(rows) > 0).all() and rows[-1] < n
    assert a["num_agents"][0] == n and a["species_count"].sum() == n
    for k in names:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    for c in COLS:
        want = full[c].view(np.int32) if c == "health" else full[c]
        assert a[c].shape == (100,) + want.shape[1:], c
        assert np.array_equal(a[c], want[rows].astype(a[c].dtype)), c
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES


def test_dump_outputs_whole_table_when_small(tmp_path):
    n, _, a, full = _run(tmp_path / "s", worlds=2, steps=2)
    assert np.array_equal(a["rows"], np.arange(n))
    assert np.array_equal(a["position"], full["position"])
