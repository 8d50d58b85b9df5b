"""CPU: the rasteriser of the C ABI from a C99 host
(tests/c_host/render_host.c, built here with gcc -std=c99 -pedantic -Werror
against include/mbots.h and libmbots.so): the NULL-list form with fewer images
than worlds, the palette call and the status codes are checked by the host
program itself; its digest of a 2-world render equals the digest of the same
render through madrona_bots (MBOTS_EXEC_CPU)."""
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


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no C compiler")
def test_render_c_host_matches_python_surface(tmp_path):
    exe = tmp_path / "render_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c_host", "render_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    import madrona_bots as mb
    m = mb.SimManager(0, 3, 15, 24, exec_mode="cpu", shard_ghost=True)
    for s in range(6):
        m.write_synthetic_actions(1234, s, True)
        m.step()
    r = m.render_worlds([0, 1], 4, rgb=True, cls=True, slot=True)
    # (what the render shows, so the digest is not of two empty floors)
    assert {0, 1, 2}.issubset(np.unique(r["cls"].numpy()).tolist()) and (r["slot"].numpy() >= 0).any()
    chunks = [np.ascontiguousarray(r[k].numpy()).tobytes() for k in ("cls", "slot", "rgb")]
    chunks.append(np.ascontiguousarray(mb.RENDER_PALETTE).tobytes())
    assert out[0] == "digest" and int(out[1], 16) == _fnv1a(chunks)
