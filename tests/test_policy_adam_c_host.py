"""CPU: the device learner step of the C ABI from a C99 host
(tests/c_host/policy_adam_host.c, built here with gcc -std=c99 -pedantic -Werror
against include/mbots.h and libmbots.so): mbots_policy_group_rows,
mbots_policy_a2c_loss and two mbots_policy_adam steps on the host path meet the
refusals the program checks and leave, checksum for checksum, what
madrona_bots.a2c_loss_groups and madrona_bots.PolicyAdam leave on the same
numbers."""
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")
N = 600


class Lcg:
    """The program's sequence: x' = 1664525 x + 1013904223 (mod 2^32), x >> 16."""

    def __init__(self, seed=97531):
        self.x = seed

    def next(self, n):
        out = np.empty(n, np.int64)
        for i in range(n):
            self.x = (self.x * 1664525 + 1013904223) & 0xFFFFFFFF
            out[i] = self.x >> 16
        return out

    def fill(self, n, div):
        return ((self.next(n) % 2001 - 1000).astype(np.float32) / np.float32(div)).astype(np.float32)


def fnv(*arrays):
    h = 14695981039346656037
    for a in arrays:
        for b in np.ascontiguousarray(a).tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return f"{h:016x}"


def test_policy_adam_c_host(tmp_path):
    import madrona_bots as mb
    exe = tmp_path / "policy_adam_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_host", "policy_adam_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = run.stdout.split()
    assert out[-1] == "ok" and out[0:-1:2] == ["gradients", "loss", "param", "m", "v", "state"]
    theirs = dict(zip(out[0:-1:2], out[1::2]))

    lcg = Lcg()
    t = torch.from_numpy
    cols = [t(lcg.fill(N, d)) for d in (100.0, 50.0, 1000.0, 200.0, 50.0)]
    lcg.next(3 * N)                                                           # (the garbage in the outputs)
    end = t((lcg.next(N) % 4).astype(np.int32))
    segments = torch.tensor([[[0, 257], [257, 257], [257, 258], [258, 300]],
                             [[310, 400], [400, 400], [400, 600], [600, 600]]], dtype=torch.int32)
    rows = mb.policy_group_rows(segments, torch.zeros(2, dtype=torch.int64))
    assert rows.tolist() == [300, 290]
    g_logp, g_value, g_entropy, loss = mb.a2c_loss_groups(*cols, end, segments, rows, 0.5, 0.01)
    assert fnv(g_logp.numpy(), g_value.numpy(), g_entropy.numpy()) == theirs["gradients"]
    assert fnv(loss.numpy()) == theirs["loss"]

    nets = []
    for _ in range(2):
        ps = []
        for shape in ((16, 69), (16,), (16, 16), (16,), (6, 16), (6,), (16, 16), (16,), (1, 16), (1,)):
            n = int(np.prod(shape))
            p = t(lcg.fill(n, 1000.0).reshape(shape)).requires_grad_()
            p.grad = t(lcg.fill(n, 100.0).reshape(shape))
            ps.append(p)
        layers = [(ps[2 * i], ps[2 * i + 1], 3 if i == 0 else 0) for i in range(5)]
        nets.append(mb.PolicyNet(layers[:1], layers[1:3], layers[3:5]))
    opt = mb.PolicyAdam(nets, lr=1e-3)
    assert opt.groups == 2 and len(opt.params) == 20
    opt.step(rows)
    opt.step(torch.tensor([300, 0]))
    sd = opt.state_dict()
    cut = lambda flat: [flat.numpy()[o:o + p.numel()] for o, p in zip(opt.offsets, opt.params)]
    assert fnv(*[p.detach().numpy() for p in opt.params]) == theirs["param"]
    assert fnv(*cut(sd["m"])) == theirs["m"] and fnv(*cut(sd["v"])) == theirs["v"]
    assert sd["state"][:, 0].tolist() == [2, 1] and fnv(sd["state"].numpy()) == theirs["state"]
