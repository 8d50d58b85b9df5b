"""CPU: PPO on the device of the C ABI from a C99 host
(tests/c_host/policy_ppo_host.c, built here with gcc -std=c99 -pedantic -Werror
against include/mbots.h and libmbots.so): mbots_policy_adv_moments,
mbots_policy_ppo_loss, mbots_policy_ppo_gate and the sequence twins on the host
path meet the refusals the program checks and print, bit for bit, what the
numpy restatement (tests/policy_ppo_ref.py) leaves on the same numbers."""
import os
import subprocess

import numpy as np

import policy_ppo_ref as pr
from test_policy_adam_c_host import Lcg, fnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")
G, N, L, B, LAST = 2, 9000, 3, 2000, 4
HYPER = dict(clip=0.2, value_clip=0.5, value_coef=0.5, entropy_coef=0.01)
SEGMENTS = np.array([[[3, 4100], [4100, 4100], [4100, 4103], [4103, 4500]],
                     [[4510, 4766], [4766, 8000], [8000, 8001], [8001, 8950]]], np.int32)


def hex64(a):
    return [f"{int(x):016x}" for x in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)]


def columns(lcg, n):
    logp, value, entropy = lcg.fill(n, 500.0), lcg.fill(n, 200.0), lcg.fill(n, 1000.0)
    old_logp = (logp + lcg.fill(n, 4000.0)).astype(np.float32)
    old_value = (value + lcg.fill(n, 1000.0)).astype(np.float32)
    adv, ret = lcg.fill(n, 300.0), lcg.fill(n, 200.0)
    lcg.next(3 * n)                                                           # (the garbage in the outputs)
    return [logp, value, entropy, old_logp, old_value, adv, ret]


def test_policy_ppo_c_host(tmp_path):
    exe = tmp_path / "policy_ppo_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_host", "policy_ppo_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = run.stdout.split()
    assert out[-1] == "ok"
    names = {0: "workspace", 3: "moments", 10: "stats", 23: "gradients", 25: "gate", 30: "rows", 33: "moments",
             40: "stats", 53: "gradients"}
    assert all(out[i] == name for i, name in names.items()), out

    lcg = Lcg(13579)
    cols = columns(lcg, N)
    end = (lcg.next(N) % 4).astype(np.int32)
    rows = np.array([4497, 4440], np.int64)
    assert rows.tolist() == (SEGMENTS[:, :, 1] - SEGMENTS[:, :, 0]).sum(axis=1).tolist()
    chunks = -(-N // pr.CHUNK)
    assert int(out[1]) >= G * 4 * chunks * 6 * 8 and int(out[2]) >= G * 4 * -(-B // pr.SEQ_CHUNK) * 6 * 8
    moments = pr.moments_rows(cols[5], end, SEGMENTS)
    assert out[4:10] == hex64(moments)
    g_logp, g_value, g_entropy, stats, _ = pr.loss_rows(cols, end, SEGMENTS, rows, moments=moments, **HYPER)
    assert out[11:23] == hex64(stats) and (stats != 0).all()
    assert out[24] == fnv(g_logp, g_value, g_entropy)
    first = pr.gate(rows, rows, stats, 0.5 * (stats[0, 4] + stats[1, 4]))
    assert sorted(first.tolist())[0] == 0 and first.max() > 0                 # one group closed
    assert [int(x) for x in out[26:30]] == first.tolist() + pr.gate(first, rows, stats, 1e30).tolist()
    assert out[28:30] == out[26:28]                                            # and it stayed closed

    net_id = lcg.next(B) % 10
    length, t0, send = ((lcg.next(B) % m).astype(np.int32) for m in (L + 1, 6, 4))
    i = np.arange(B)
    net_id[(net_id >= 2) & (net_id < 8) & (i % 7 != 0)] = 1
    assert (net_id == 1).sum() > pr.SEQ_CHUNK
    cols = [c.reshape(L, B) for c in columns(lcg, L * B)]
    # mbots_policy_seq_order: the columns of key 0 .. 7 in ascending key, stable; the rest behind them
    order = np.concatenate([np.nonzero(net_id == k)[0] for k in range(4 * G)] +
                           [np.nonzero(net_id >= 4 * G)[0]]).astype(np.int32)
    count = np.array([(net_id == k).sum() for k in range(4 * G)])
    hi = np.cumsum(count)
    segments = np.stack([hi - count, hi], axis=1).reshape(G, 4, 2).astype(np.int32)
    kept = pr.seq_kept(length, t0, send, LAST, L)
    seq_rows = np.array([kept[order[segments[g, 0, 0]:segments[g, 3, 1]]].sum() for g in range(G)], np.int64)
    assert [int(x) for x in out[31:33]] == seq_rows.tolist() and seq_rows.min() > 0
    moments = pr.moments_seq(cols[5], length, t0, send, order, segments, LAST)
    assert out[34:40] == hex64(moments)
    g_logp, g_value, g_entropy, stats = pr.loss_seq(cols, length, t0, send, order, segments, seq_rows, LAST,
                                                    moments=moments, **HYPER)
    assert out[41:53] == hex64(stats) and (stats != 0).all()
    assert out[54] == fnv(g_logp, g_value, g_entropy)
