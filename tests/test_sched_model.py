"""CPU: the step's cross-queue ordering rules (csrc/mbots_sched.hpp) checked
for every call order by a stand-alone program (tests/c_host/sched_model.cpp),
built here with g++ and the address and undefined-behaviour sanitizers and run
directly.

The program runs the rules over a symbolic executor (vector clocks per queue)
and checks every access of a buffer two queues share against the accesses
before it: every sequence of 4 calls out of its 13 (step with the host ahead
or behind, shift with and without the prev-sensor move, the sensor-row and
prev-sensor reads, an action write, a switch of the caller's stream, join, the
idle reset, begin / end capture, replay) from five starting points (fresh, two
steps, a captured pair of steps, that replayed, an odd capture), in the four
schedules, armed and not: 357 170 sequences; and 400 fixed-seed random runs of
60 calls that start five epochs short of the wrap.  It prints the per-step
edge table and asserts it, and shows that it sees the two seeded faults.
About six seconds with the sanitizers on."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no C++ compiler")
def test_sched_model(tmp_path):
    exe = tmp_path / "sched_model"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "madrona-bots_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_host", "sched_model.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "depth 4: 357170 sequences" in r.stdout
    assert "runs crossed the epoch wrap" in r.stdout
    # the seeded faults are seen
    assert "seeded single ObsrowOut: hazard: K1 writes ObsrowOut[0] beside the sensor after: step, step" in r.stdout
    assert "seeded equality waits, no join: hang: the equality wait" in r.stdout
    assert r.stdout.rstrip().endswith("ok")
