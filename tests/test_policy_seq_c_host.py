"""CPU: the handle-free sequence calls of the C ABI from a C99 host
(tests/c_host/policy_seq_host.c, built here with gcc -std=c99 -pedantic
-Werror against include/mbots.h and libmbots.so, and run as its own program)
give the same bytes as PolicyNet.evaluate_sequences and backward() on the same
net, sequences and upstream gradients, and meet the refusals the host program
checks itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_policy_c_host import ROOT, LIBDIR, _Lcg, _fnv1a

H, L, B = 32, 4, 70


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_policy_seq_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "policy_seq_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "policy_seq_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    g = _Lcg()

    def layer(n_in, n_out, act, div):
        w, b, a = g.layer(n_in, n_out, act, div)
        return (w.requires_grad_(), b.requires_grad_(), a)
    trunk = [layer(85, H, 3, 16384.0), layer(H, H, 4, 2048.0)]
    actor = [layer(H, H, 0, 2048.0), layer(H, 6, 0, 1024.0)]
    critic = [layer(H, H, 0, 2048.0), layer(H, 1, 0, 2048.0)]
    memory = layer(H, 16, 0, 512.0)
    net = mb.PolicyNet(trunk, actor, critic, memory, True)
    obs, hidden0 = g.fill((L, B, 69), 8.0), g.fill((B, 16), 1000.0)
    gs = [g.fill((L, B), 65536.0) for _ in range(3)]

    def ints(n, mod):
        out = np.empty(n, np.int32)
        for i in range(n):
            g.x = (g.x * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = (g.x >> 16) % mod
        return out
    action, length = ints(L * B, 6).reshape(L, B), ints(B, L + 1)
    res = net.evaluate_sequences(obs, torch.from_numpy(action), torch.from_numpy(length), hidden0, return_hidden=True)
    sum((q * o).sum() for q, o in zip(gs, res[:3])).backward()
    d = _fnv1a(1469598103934665603, *[o.detach().numpy() for o in res])
    d = _fnv1a(d, *[p.grad.numpy() for w, b, _ in trunk + actor + critic + [memory] for p in (w, b)])
    assert out[:2] == ["sequences", str(B)]
    assert int(out[3], 16) == d
