"""CPU: the trajectory window of the C ABI from a C99 host
(tests/c_host/traj_host.c, built here with gcc -std=c99 -pedantic -Werror
against include/mbots.h and libmbots.so) gives the same view bytes as the same
calls through madrona_bots (MBOTS_EXEC_CPU), and meets the refusals the host
program checks itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")
HORIZON = 6


def _fnv1a(chunks):
    h = 1469598103934665603
    for b in chunks:
        for x in b:
            h ^= x
            h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _chunks(win, res):
    n = len(res["rows"])
    order = ("link", "next", "end", "world", "reward", "value", "adv", "ret")   # enum mbots_traj_view_id
    return [np.ascontiguousarray(res[k][t].numpy()).tobytes()
            for t in range(n) for k in order if not (k == "next" and t == n - 1)]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_traj_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "traj_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "traj_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    m = mb.SimManager(0, 4, 15, 8, exec_mode="cpu", world_offset=3)
    win = m.trajectory_window(HORIZON, 256)
    m.set_episode_length(3)

    def push(step):
        win.push(0.25 * torch.arange(m.num_agents(), dtype=torch.float32) - float(step))
    chunks, ends = [], []
    push(0)
    for s in range(2 * (HORIZON - 1)):
        m.write_synthetic_actions(1234, s, False)
        m.step()
        push(s + 1)
        if s + 2 == HORIZON:
            res = win.compute(0.99, 0.95, -1.0)
            chunks += _chunks(win, res)
            ends += [e.numpy().copy() for e in res["end"]]
            win.clear(keep_last=True)
            m.grow_capacity(256)
    res = win.compute(0.99, 0.95, -1.0)
    chunks += _chunks(win, res)
    ends += [e.numpy().copy() for e in res["end"]]
    # (what the calls did, so the digest is not of a run in which they did nothing)
    assert win.num_tables == HORIZON and (res["world"][0] >= 3).all()
    assert any((e == 2).any() for e in ends) and any((e == 0).any() for e in ends)
    assert out[:2] == ["agents", str(m.num_agents())]
    assert int(out[3], 16) == _fnv1a(chunks)
