#!/usr/bin/env python3
"""What the trajectory window costs on one GPU: nothing while a manager has
none, one small launch per step for the push, and three launches plus one host
synchronisation for a compute over the window.

At --worlds worlds (65536) and a horizon of --horizon tables (16) on bench.py's
headline loop (step, shift_observations, write_synthetic_actions), --reps
alternating repeats per variant in one process, each timed with device events
around --steps steps after --warmup warm-up steps (the end event after
mbots_join, so the sensor's stream is inside the span):

  1. with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1
     --steps 100 --warmup 20 of that tree and of this one, alternating, each in a
     process of its own.  A manager without a window must sit inside the parent's
     own run-to-run spread: |mean(branch) - mean(parent)| <= max(parent) -
     min(parent) of ms_per_step ("no_window_within_parent_spread").
  2. the loop with a push (value = a device array of N f32) after every step,
     the window chained with clear(keep_last=True) whenever it is full, against
     the plain loop: the push in us per step and in percent.
  3. one compute(0.99, 0.95) over a full window: host wall time from the call to
     the device being idle (its own synchronisation and its three launches).

Writes every time and the means to --out (JSON)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd"))

SEED, A, ACTION_SEED = 69, 32, 1234   # bench.py's


def bench_ms(tree):
    """ms_per_step of `python bench.py --gpus 1 --steps 100 --warmup 20` in `tree`."""
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "100",
                          "--warmup", "20"], cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part 1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_window_cost.json"))
    args = ap.parse_args()
    W, T = args.worlds, args.horizon
    res = {"worlds": W, "horizon": T, "steps": args.steps, "warmup": args.warmup, "reps": args.reps}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    if args.parent:
        par, br = [], []
        for _ in range(args.reps):
            par.append(bench_ms(os.path.abspath(args.parent)))
            br.append(bench_ms(ROOT))
        spread = max(par) - min(par)
        res["bench_no_window"] = {
            "command": "bench.py --gpus 1 --steps 100 --warmup 20", "parent_ms_per_step": par,
            "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par), "branch_mean_ms": statistics.mean(br),
            "parent_spread_ms": spread,
            "no_window_within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}
        save()

    import torch
    import madrona_bots as mb
    res["device"] = torch.cuda.get_device_name(0)
    max_rows = W * 2 * A   # (the synthetic stream keeps a world near its initial population)

    def loop(m, t0, steps, win=None, value=None):
        for t in range(t0, t0 + steps):
            m.step()
            if win is not None:
                if win.num_tables == T:
                    win.clear(keep_last=True)
                win.push(value)
            m.shift_observations()
            m.write_synthetic_actions(ACTION_SEED, t + 1)

    def timed_loop(m, t0, steps, win=None, value=None):
        """ms per step of `steps` iterations: device events, the sensor's stream joined"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.join()
        a.record()
        loop(m, t0, steps, win, value)
        m.join()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps

    # 2. a push per step against the plain loop; 3. a compute over the full window
    plain, pushed, compute_ms, rows_seen = [], [], [], []
    for _ in range(args.reps):
        for with_window, into in ((False, plain), (True, pushed)):
            m = mb.SimManager(0, W, SEED, A)
            win = value = None
            if with_window:
                win = m.trajectory_window(T, max_rows)
                value = torch.rand(max_rows, dtype=torch.float32, device=m.device)
                win.push(value)
            m.write_synthetic_actions(ACTION_SEED, 0)
            loop(m, 0, args.warmup, win, value)
            into.append(timed_loop(m, args.warmup, args.steps, win, value))
            if with_window:
                t = args.warmup + args.steps
                while win.num_tables < T:
                    loop(m, t, 1, win, value)
                    t += 1
                win.compute(0.99, 0.95)   # (warm: the three kernels' code objects)
                for _ in range(3):
                    torch.cuda.synchronize()
                    h0 = time.perf_counter()
                    out = win.compute(0.99, 0.95)
                    torch.cuda.synchronize()
                    compute_ms.append((time.perf_counter() - h0) * 1e3)
                rows_seen.append(max(out["rows"]))
                win.close()
            del m
    mp, mw = statistics.mean(plain), statistics.mean(pushed)
    res["push_per_step"] = {"plain_ms_per_step": plain, "pushed_ms_per_step": pushed, "plain_mean_ms": mp,
                            "pushed_mean_ms": mw, "overhead_us_per_step": (mw - mp) * 1e3,
                            "overhead_percent": (mw - mp) / mp * 100.0, "plain_spread_ms": max(plain) - min(plain)}
    res["compute"] = {"tables": T, "largest_table_rows": rows_seen, "wall_ms": compute_ms,
                      "mean_ms": statistics.mean(compute_ms),
                      "note": "host wall time of compute(0.99, 0.95) until the device is idle, the window full"}
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
