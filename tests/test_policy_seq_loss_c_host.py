"""CPU: the recurrent update of the C ABI from a C99 host
(tests/c_host/policy_seq_loss_host.c, built here with gcc -std=c99 -pedantic
-Werror against include/mbots.h and libmbots.so): mbots_policy_seq_group_rows,
mbots_policy_seq_a2c_loss and two mbots_policy_adam_clip steps on the host path
meet the refusals the program checks and print, bit for bit, what the numpy
restatement (tests/policy_seq_loss_ref.py) leaves on the same numbers."""
import os
import subprocess

import numpy as np

import policy_adam_ref as ar
import policy_seq_loss_ref as sr
from test_policy_adam_c_host import Lcg, fnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")
G, L, B, LAST = 2, 3, 300, 4
SIZES = (5, 1024, 2049)
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0)


def test_policy_seq_loss_c_host(tmp_path):
    exe = tmp_path / "policy_seq_loss_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_host", "policy_seq_loss_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = run.stdout.split()
    assert out[-1] == "ok"
    assert [out[i] for i in (0, 3, 6, 8, 11, 13, 15, 17)] == ["rows", "loss", "gradients", "grad_norm", "param", "m",
                                                             "v", "state"]

    lcg = Lcg(24680)
    net_id = lcg.next(B) % 10
    length, t0, end = lcg.next(B) % (L + 1), lcg.next(B) % 6, lcg.next(B) % 4
    cols = [lcg.fill(L * B, d).reshape(L, B) for d in (100.0, 50.0, 1000.0, 200.0, 50.0)]
    lcg.next(3 * L * B)                                                       # (the garbage in the outputs)
    # mbots_policy_seq_order: the columns of key 0 .. 7 in ascending key, stable; the rest behind them
    order = np.concatenate([np.nonzero(net_id == k)[0] for k in range(4 * G)]).astype(np.int32)
    hi = np.cumsum([(net_id == k).sum() for k in range(4 * G)])
    segments = np.stack([hi - [(net_id == k).sum() for k in range(4 * G)], hi], axis=1).reshape(G, 4, 2)
    rows = sr.group_rows(L, length, t0, end, order, segments, LAST)
    assert [int(x) for x in out[1:3]] == rows.tolist() and rows.min() > 0
    g_logp, g_value, g_entropy, loss, _ = sr.seq_loss_f32(*cols, length, t0, end, order, segments, rows, LAST)
    assert out[4:6] == [f"{int(x):016x}" for x in loss.view(np.uint64)]
    assert out[7] == fnv(g_logp, g_value, g_entropy)

    tensors = []
    for g in range(G):
        for n in SIZES:
            p, grad = lcg.fill(n, 1000.0), lcg.fill(n, 100.0)
            tensors.append((p, grad, np.zeros(n, np.float32), np.zeros(n, np.float32), g))
    state = ar.adam_state(G)
    norms = sr.adam_clip_f32(tensors, state, rows.tolist(), **HYPER)
    assert out[9:11] == [f"{int(x):08x}" for x in norms.view(np.uint32)] and norms.min() > HYPER["max_norm"]
    sr.adam_clip_f32(tensors, state, [int(rows[0]), 0], **HYPER)
    assert out[12] == fnv(*[t[0] for t in tensors])
    assert out[14] == fnv(*[t[2] for t in tensors]) and out[16] == fnv(*[t[3] for t in tensors])
    st = np.array([[t, np.float32(a).view(np.uint32), np.float32(b).view(np.uint32)] for t, a, b in state], np.uint32)
    assert st[:, 0].tolist() == [2, 1] and out[18] == fnv(st)
