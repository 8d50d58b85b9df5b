"""CPU: the grouped sequence calls of the C ABI from a C99 host
(tests/c_host/policy_seq_groups_host.c, built here with gcc -std=c99 -pedantic
-Werror against include/mbots.h and libmbots.so, and run as its own program)
give the same bytes as madrona_bots.sequence_segments,
evaluate_sequences_groups and backward() on the same nets, sequences and
upstream gradients, and meet the refusals the host program checks itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_policy_c_host import ROOT, LIBDIR, _Lcg, _fnv1a

GROUPS, L, B = 2, 3, 300


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_policy_seq_groups_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "policy_seq_groups_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_host", "policy_seq_groups_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    g = _Lcg()

    def layer(n_in, n_out, act, div):
        w, b, a = g.layer(n_in, n_out, act, div)
        return (w.requires_grad_(), b.requires_grad_(), a)
    nets, layers = [], []
    for e in range(4 * GROUPS):
        if e == 2:
            nets.append(None)
            continue
        H, T = (32 if e >= 4 else 16), 1 + (e & 1)
        trunk = [layer(H if l else 85, H, 1 + (e + l) % 5, 2048.0 if l else 16384.0) for l in range(T)]
        actor = [layer(H, H, 0, 2048.0), layer(H, 6, 0, 1024.0)]
        critic = [layer(H, H, 0, 2048.0), layer(H, 1, 0, 2048.0)]
        memory = layer(H, 16, 0, 512.0)
        nets.append(mb.PolicyNet(trunk, actor, critic, memory, True))
        layers.append(trunk + actor + critic + [memory])
    obs, hidden0 = g.fill((L, B, 69), 8.0), g.fill((B, 16), 1000.0)
    gs = [g.fill((L, B), 65536.0) for _ in range(3)]

    def ints(n, mod):
        out = np.empty(n, np.int32)
        for i in range(n):
            g.x = (g.x * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = (g.x >> 16) % mod
        return out
    action, length = ints(L * B, 6).reshape(L, B), ints(B, L + 1)
    net_id = ints(B, 4 * GROUPS + 2) - 1
    order, seg = mb.sequence_segments(torch.from_numpy(net_id), GROUPS)
    res = mb.evaluate_sequences_groups([nets[:4], nets[4:]], obs, torch.from_numpy(action), torch.from_numpy(length),
                                       hidden0, order, seg, return_hidden=True)
    sum((q * o).sum() for q, o in zip(gs, res[:3])).backward()
    d = _fnv1a(1469598103934665603, order.numpy(), seg.numpy(), *[o.detach().numpy() for o in res])
    d = _fnv1a(d, *[p.grad.numpy() for net in layers for w, b, _ in net for p in (w, b)])
    assert out[:2] == ["sequences", str(B)]
    assert int(out[3], 16) == d
