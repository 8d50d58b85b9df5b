"""CPU: the episode entry points of the C ABI from a C99 host
(tests/c_host/reset_host.c, built here with gcc -std=c99 -pedantic -Werror
against include/mbots.h and libmbots.so) give the same exported bytes as the
same calls through madrona_bots (MBOTS_EXEC_CPU)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")


def _fnv1a(chunks):
    h = 1469598103934665603
    for b in chunks:
        for x in b:
            h ^= x
            h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _views(m):
    get = [m.reset_tensor, m.episode_tensor, m.episode_step_tensor, m.action_tensor, m.reward_tensor,
           m.position_tensor, lambda: m.position_tensor(True), m.health_tensor, m.semantic_tensor,
           lambda: m.semantic_tensor(True), m.stats_tensor, m.species_count_tensor]
    return [np.ascontiguousarray(g().to_torch().numpy()).tobytes() for g in get]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_reset_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "reset_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "reset_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    W, T = 6, 12
    out = subprocess.run([str(exe), str(W), str(T)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    m = mb.SimManager(0, W, 69, 32, exec_mode="cpu", world_offset=1)
    m.reset_worlds([])
    assert not m.schedule_info()["episodes_armed"]
    m.set_episode_length(5)
    for t in range(T):
        if t == 2:
            m.reset_worlds([1, 1000])
        if t == 4:
            m.reset_worlds([0, 2], [5, 0])
        if t == 7:
            m.reset_tensor().to_torch()[3] = 9 + 2
        m.step()
        m.shift_observations()
        m.write_synthetic_actions(1234, t, True)
    # (what the calls did, so the digest is not of a run in which they did nothing)
    assert m.episode_tensor().to_torch().reshape(-1).tolist() == [2, 1, 2, 9, 2, 2]
    assert m.episode_step_tensor().to_torch().reshape(-1).tolist() == [5, 3, 2, 5, 2, 2]
    assert out[:2] == ["agents", str(m.num_agents())]
    assert int(out[3], 16) == _fnv1a(_views(m))
