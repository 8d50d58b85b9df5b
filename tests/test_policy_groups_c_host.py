"""CPU: the policy groups of the C ABI from a C99 host
(tests/c_host/policy_groups_host.c, built here with gcc -std=c99 -pedantic
-Werror against include/mbots.h and libmbots.so): the five entry points give
the same segments, the same outputs and the same Action / HiddenState bytes as
the same calls through madrona_bots (MBOTS_EXEC_CPU), on a shard whose ghost
world is a group of its own, and meet the refusals the host program checks
itself."""
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")
STARTS = [0, 7, 9, 11]


class _Lcg:
    def __init__(self):
        self.x = 777

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


def test_policy_groups_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "policy_groups_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "policy_groups_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    lcg = _Lcg()
    nets = []
    for g in range(4):
        four = []
        for s in range(4):
            big = bool(g & 1)
            H = 32 if big else 16
            trunk = [lcg.layer(85 if big else 69, H, 3, 262144.0)]
            if not big:
                trunk.append(lcg.layer(H, H, s + 2, 2048.0))
            actor = [lcg.layer(H, H, 0, 2048.0), lcg.layer(H, 6, 0, 1024.0)]
            critic = [lcg.layer(H, H, 0, 2048.0), lcg.layer(H, 1, 0, 2048.0)]
            four.append(mb.PolicyNet(trunk, actor, critic, lcg.layer(H, 16, 0, 2048.0) if big else None, big))
        nets.append(four)
    m = mb.SimManager(0, 6, 21, 12, exec_mode="cpu", world_offset=5, shard_ghost=True)
    m.set_policy_groups(STARTS)
    for g in range(4):
        m.set_policy(nets[g], group=g)
    d = 1469598103934665603

    def digest(d, o):
        return _fnv1a(d, o["action"].numpy(), o["logp"].numpy(), o["value"].numpy(),
                      m.action_tensor().to_torch().numpy(), m.hidden_state_tensor().to_torch().numpy())
    shares = np.zeros(6)
    for t in range(4):
        seg = m.policy_segments().numpy()
        assert seg.dtype == np.int32 and seg.shape == (4, 4, 2)
        d = _fnv1a(d, seg)
        o = m.act(greedy=t == 2)
        shares += np.bincount(o["action"].numpy().ravel(), minlength=6)
        d = digest(d, o)
        m.step()
    assert (shares > 0).sum() >= 4          # (the run is not one in which every agent does the same)
    m.set_policy(nets[2][0], species=1)      # no group: every group
    d = digest(d, m.act())
    m.clear_policy(species=3, group=2)
    m.set_policy_groups(STARTS)
    m.set_policy(nets[2][2], species=3, group=2)
    d = digest(d, m.act(write=False))
    assert out[:2] == ["agents", str(m.num_agents())]
    assert int(out[3], 16) == d
