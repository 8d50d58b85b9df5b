"""CPU: the trajectory window's sequences, batches and gathers of the C ABI from
a C99 host (tests/c_host/seq_host.c, built here with gcc -std=c99 -pedantic
-Werror against include/mbots.h and libmbots.so) give the same bytes as the
same calls through madrona_bots (MBOTS_EXEC_CPU), and meet the refusals the
host program checks itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_traj_c_host import HORIZON, LIBDIR, ROOT, _fnv1a

MAX_ROWS = 256


def _chunks(win):
    res = win.compute(0.99, 0.95, -1.0)
    S = win.sequences()
    n = len(res["rows"])
    out = [np.ascontiguousarray(win.view(what, t).numpy()).tobytes()
           for t in range(n) for what in (win.SEQ_ID, win.SEQ_POS)]
    b = win.batch()
    assert tuple(b) == ("rows", "t0", "len", "end", "obs", "reward", "value", "adv", "ret", "action_in", "hidden0")
    out += [np.ascontiguousarray(v.numpy()).tobytes() for v in b.values()]
    own = [torch.stack([torch.full((r,), float(t)), torch.arange(r, dtype=torch.float32)], 1).contiguous()
           for t, r in enumerate(res["rows"])]
    out.append(np.ascontiguousarray(win.gather(own).numpy()).tobytes())
    return out, S, b


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_seq_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "seq_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "seq_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    m = mb.SimManager(0, 4, 15, 8, exec_mode="cpu", world_offset=3)
    win = m.trajectory_window(HORIZON, MAX_ROWS, record_obs=True, record_state=True)
    m.set_episode_length(3)

    def push(step):
        win.push(0.25 * torch.arange(m.num_agents(), dtype=torch.float32) - float(step))
    chunks, counts, batches = [], [], []
    push(0)
    for s in range(2 * (HORIZON - 1)):
        m.write_synthetic_actions(1234, s, True)
        m.step()
        push(s + 1)
        if s + 2 == HORIZON:
            c, S, b = _chunks(win)
            chunks += c
            counts.append(S)
            batches.append(b)
            win.clear(keep_last=True)
            m.grow_capacity(256)
    c, S, b = _chunks(win)
    chunks += c
    counts.append(S)
    batches.append(b)
    # (what the calls did, so the digest is not of a run in which they did nothing)
    assert all((x["end"].numpy() == 2).any() and (x["len"].numpy() > 1).any() and x["obs"].numpy().any()
               and x["action_in"].numpy().any() for x in batches)
    assert batches[1]["hidden0"].numpy().any()
    assert out[:2] == ["agents", str(m.num_agents())]
    assert out[2:5] == ["sequences", str(counts[0]), str(counts[1])]
    assert int(out[6], 16) == _fnv1a(chunks)
