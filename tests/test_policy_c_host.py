"""CPU: the device actor of the C ABI from a C99 host
(tests/c_host/policy_host.c, built here with gcc -std=c99 -pedantic -Werror
against include/mbots.h and libmbots.so) gives the same outputs and the same
Action / HiddenState bytes as the same calls through madrona_bots
(MBOTS_EXEC_CPU), and meets the refusals the host program checks itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")
H = 16


class _Lcg:
    def __init__(self):
        self.x = 12345

    def fill(self, shape, div):
        n = int(np.prod(shape))
        out = np.empty(n, np.float32)
        for i in range(n):
            self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = np.float32(((self.x >> 16) % 2001) - 1000) / np.float32(div)
        return torch.from_numpy(out.reshape(shape))

    def layer(self, n_in, n_out, act, div):
        w = self.fill((n_out, n_in), div)
        return (w, self.fill((n_out,), 4096.0), act)


def _fnv1a(h, *arrays):
    for a in arrays:
        for x in np.ascontiguousarray(a).tobytes():
            h ^= x
            h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_policy_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "policy_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "policy_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    g = _Lcg()
    nets = []
    for s in range(4):
        mem = bool(s & 1)
        trunk = [g.layer(85 if mem else 69, H, 3, 262144.0), g.layer(H, H, s + 2, 2048.0)]
        actor = [g.layer(H, H, 0, 2048.0), g.layer(H, 6, 0, 1024.0)]
        critic = [g.layer(H, H, 0, 2048.0), g.layer(H, 1, 0, 2048.0)]
        nets.append(mb.PolicyNet(trunk, actor, critic, g.layer(H, 16, 0, 2048.0) if mem else None, mem))
    m = mb.SimManager(0, 6, 21, 12, exec_mode="cpu", world_offset=5)
    m.set_policy(nets)
    d = 1469598103934665603

    def digest(d, o):
        return _fnv1a(d, o["action"].numpy(), o["logp"].numpy(), o["value"].numpy(),
                      m.action_tensor().to_torch().numpy(), m.hidden_state_tensor().to_torch().numpy())
    shares = np.zeros(6)
    for t in range(4):
        o = m.act(greedy=t == 2)
        shares += np.bincount(o["action"].numpy().ravel(), minlength=6)
        d = digest(d, o)
        m.step()
    assert m.policy_draw == 4
    assert (shares > 0).sum() >= 4          # (the run is not one in which every agent does the same)
    d = digest(d, m.act(write=False))
    w, b, a = nets[0].actor[1]
    nets[0].actor[1] = (g.fill((6, H), 512.0), b, a)
    m.policy_draw = 5                        # (the host program's two repeats advanced the counter to 5)
    m.set_policy(nets[0], species=1)
    d = digest(d, m.act())
    assert out[:2] == ["agents", str(m.num_agents())]
    assert int(out[3], 16) == d
