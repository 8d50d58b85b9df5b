"""CPU: the grouped evaluate of the C ABI from a C99 host
(tests/c_host/policy_eval_groups_host.c, built here with gcc -std=c99 -pedantic
-Werror against include/mbots.h and libmbots.so): mbots_policy_groups_workspace,
mbots_policy_eval_groups and mbots_policy_grad_groups on the host path meet the
refusals the program checks -- a workspace that is too small, a NULL `out`, bad
segments -- and give, byte for byte, what the per-net calls give on each
segment's rows, with an n_trunk == 0 entry among the nets."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "madrona-bots_amd", "madrona_bots")


def test_policy_eval_groups_c_host(tmp_path):
    exe = tmp_path / "policy_eval_groups_host"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1",
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_host", "policy_eval_groups_host.c"),
                    "-L", LIBDIR, "-lmbots", "-Wl,-rpath," + LIBDIR, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    out = run.stdout.split()
    assert out[:5] == ["ok", "rows", "400", "segments", "8"] and int(out[6]) > 0
