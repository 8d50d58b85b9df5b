#!/usr/bin/env python3
"""More seeds of tests/test_parity_gpu.py::test_random_call_sequences on the
GPU (random step / shift / action-write / column-read / construct_obs /
checkpoint hand-over sequences against the oracle; seeds % 4 == 0 at 4100
worlds, the others at 21+ worlds in K1-finder mode):
    python scripts/fuzz_calls.py [--episodes | --window] [--cpu] FIRST_SEED END_SEED [WORLDS]
(WORLDS: every seed at that world count, e.g. 16400 for the swapped schedule)
--episodes runs test_random_call_sequences_episodes instead: the same
sequences with reset_worlds, flag writes through reset_tensor(),
set_episode_length, grow_capacity and set_world_state among the operations;
--window runs tests/test_window_sequences.py::run_window_sequence: those
operations with a trajectory window pushed behind every step and renders
queued, against the oracle-side reference (20 + seed worlds unless WORLDS);
--cpu (with --episodes or --window) runs them in CPU mode, which needs no
device.  Both print what each seed did."""
import sys, os, time
sys.path[:0] = ["madrona-bots_amd", "oracle", "tests"]
import test_parity_gpu as t
args = [a for a in sys.argv[1:] if not a.startswith("--")]
episodes, window, cpu = "--episodes" in sys.argv, "--window" in sys.argv, "--cpu" in sys.argv
lo, hi = int(args[0]), int(args[1])
W = int(args[2]) if len(args) > 2 else None
t0 = time.time()
for s in range(lo, hi):
    if window:
        import test_window_sequences as tw
        info = tw.run_window_sequence(s, W, exec_mode="cpu" if cpu else "hip")
        print("seed", s, "worlds", W or 20 + s, "ok", info, round(time.time() - t0, 1), flush=True)
    elif episodes:
        info = t.run_episode_sequence(s, W, exec_mode="cpu" if cpu else "hip")
        print("seed", s, "ok", info, round(time.time() - t0, 1), flush=True)
    else:
        t.test_random_call_sequences(s, W)
        print("seed", s, "ok", round(time.time() - t0, 1), flush=True)
