"""CPU: harness/a2c_recurrent.py and harness/a2c_recurrent_groups.py with
--device-update --exec-mode cpu run as command lines, print finite losses, and
print the same losses in a second run with 4 OpenMP threads as in a first with
1: the update's sums run in a fixed order.  (The processes are the subject: the
thread count is read when the library loads.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "madrona-bots_amd", "harness")
CASES = {
    "recurrent": ["a2c_recurrent.py", "--worlds", "16", "--iters", "2", "--hidden", "32", "--gated"],
    "recurrent_groups": ["a2c_recurrent_groups.py", "--worlds", "16", "--groups", "2", "--iters", "2", "--hidden", "32",
                         "16", "--max-grad-norm", "0.5", "--weight-decay", "0.01"],
}


def run(args, threads):
    env = dict(os.environ, OMP_NUM_THREADS=str(threads))
    out = subprocess.run([sys.executable, os.path.join(HARNESS, args[0]), *args[1:], "--device-update", "--exec-mode",
                          "cpu"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    return [json.loads(line)["loss"] for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_update_runs_and_is_deterministic(name):
    first, four = run(CASES[name], 1), run(CASES[name], 4)       # two runs, and two thread counts
    assert len(first) == 2 and all(x == x and abs(x) < 1e6 for it in first for x in it)
    assert first[0] != first[1]                          # the second update saw other nets
    assert first == four


def test_options_need_device_update():
    out = subprocess.run([sys.executable, os.path.join(HARNESS, "a2c_recurrent_groups.py"), "--max-grad-norm", "1.0",
                          "--exec-mode", "cpu"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode != 0 and "need --device-update" in out.stderr
