"""CPU: the manager's deferred-column rules (csrc/mbots_defer.hpp) checked
exhaustively against an eager table by a stand-alone program
(tests/c_host/defer_model.cpp), built here with g++ and the address and
undefined-behaviour sanitizers and run directly.

The program runs every sequence of 4 calls out of its 21 (step, shift, the
reads, the writes, the device actor's uses, the packs, save, load) from six
starting points and for the four combinations of owed PrevAction on/off and
prev-sensor-by-sensor: 4 667 544 sequences; every sequence of 3 calls with
"step / shift while capturing" added: 292 008 sequences; and 12 000 fixed-seed
random sequences of 40 calls.  About six seconds with the sanitizers on; depth 5
would be two minutes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no C++ compiler")
def test_defer_model(tmp_path):
    exe = tmp_path / "defer_model"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "madrona-bots_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_host", "defer_model.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "depth 4: 4667544 sequences" in r.stdout
    assert "capture depth 3: 292008 sequences" in r.stdout
