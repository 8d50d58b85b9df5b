"""CPU: the gated memory head of the C ABI from a C99 host
(tests/c_host/policy_gate_host.c, built here with gcc -std=c99 -pedantic
-Werror against include/mbots.h and libmbots.so, and run as its own program)
gives the same bytes as SimManager.act() and PolicyNet.evaluate_sequences +
backward() on the same gated net, and meets the refusals the host program
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
def test_policy_gate_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "policy_gate_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "policy_gate_host.c"),
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
    gate = layer(H, 16, 0, 256.0)
    net = mb.PolicyNet(trunk, actor, critic, memory, True, gate)
    obs, hidden0 = g.fill((L, B, 69), 8.0), g.fill((B, 16), 1000.0)
    gs = [g.fill((L, B), 65536.0) for _ in range(3)]

    def ints(n, mod):
        out = np.empty(n, np.int32)
        for i in range(n):
            g.x = (g.x * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = (g.x >> 16) % mod
        return out
    action, length = ints(L * B, 6).reshape(L, B), ints(B, L + 1)

    # act(): the gated net for every species
    m = mb.SimManager(0, 6, 21, 12, exec_mode="cpu")
    m.set_policy([net] * 4)
    da = 1469598103934665603
    moved = False
    for t in range(3):
        before = m.hidden_state_tensor().to_torch().numpy().copy()
        o = m.act()
        after = m.hidden_state_tensor().to_torch().numpy()
        moved |= bool((after != before).any())
        da = _fnv1a(da, o["action"].numpy(), o["logp"].numpy(), o["value"].numpy(),
                    m.action_tensor().to_torch().numpy(), after)
        n = m.num_agents()
        m.step()
    assert moved
    assert out[:2] == ["agents", str(n)]
    assert int(out[3], 16) == da

    res = net.evaluate_sequences(obs, torch.from_numpy(action), torch.from_numpy(length), hidden0, return_hidden=True)
    sum((q * o).sum() for q, o in zip(gs, res[:3])).backward()
    d = _fnv1a(1469598103934665603, *[o.detach().numpy() for o in res])
    d = _fnv1a(d, *[p.grad.numpy() for w, b, _ in trunk + actor + critic + [memory, gate] for p in (w, b)])
    assert out[4:6] == ["sequences", str(B)]
    assert int(out[7], 16) == d
