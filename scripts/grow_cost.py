#!/usr/bin/env python3
"""What a capacity growth costs on one GPU, and what the per-step check costs.

At --worlds worlds (65536), 128 -> 256 slots, after 5 warm-up steps, three
repetitions of each in one process, interleaved, timed with time.perf_counter
around a device synchronise on both sides:

  (a) the checkpoint hand-over SimManager(agent_capacity="auto") used to make:
      save_checkpoint, a new manager at 256, load_checkpoint;
  (b) grow_capacity(256) on an identical manager (mbots_grow_capacity: the
      device-side move inside the same handle).

Then bench.py's headline loop (step, shift_observations,
write_synthetic_actions) with the library's automatic capacity off and on:
the per-step cost of mbots_step's population check.  Writes every time, the
medians and the checkpoint blob's size to --out (JSON)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd"))

import torch  # noqa: E402

import madrona_bots as mb  # noqa: E402

SEED, A, ACTION_SEED = 69, 32, 1234   # bench.py's


def warmed(W, steps, **kw):
    m = mb.SimManager(0, W, SEED, A, **kw)
    m.write_synthetic_actions(ACTION_SEED, 0)
    for t in range(steps):
        m.step()
        m.shift_observations()
        m.write_synthetic_actions(ACTION_SEED, t + 1)
    torch.cuda.synchronize()
    return m


def hand_over(m, W, cap):
    """(seconds in all, {part: seconds}, blob bytes, the new manager)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    blob = m.save_checkpoint()
    t1 = time.perf_counter()
    n = mb.SimManager(0, W, SEED, A, agent_capacity=cap)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    n.load_checkpoint(blob)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return t3 - t0, {"save_checkpoint": t1 - t0, "new_manager": t2 - t1, "load_checkpoint": t3 - t2}, blob.size, n


def in_place(m, cap):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.grow_capacity(cap)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def digest(m):
    """A cheap equality check of the two paths' results (not timed)."""
    return (m.num_agents(), float(m.position_tensor().to_torch().double().sum()),
            int(m.semantic_tensor().to_torch().long().sum()))


def headline(W, warmup, steps, auto):
    m = warmed(W, warmup, auto_grow=auto)
    t0 = time.perf_counter()
    for t in range(warmup, warmup + steps):
        m.step()
        m.shift_observations()
        m.write_synthetic_actions(ACTION_SEED, t + 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, m.agent_capacity


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grow_capacity_cost.json"))
    args = ap.parse_args()
    W = args.worlds
    res = {"worlds": W, "from_capacity": 128, "to_capacity": 256, "warmup_steps": 5,
           "device": torch.cuda.get_device_name(0), "hand_over_s": [], "hand_over_parts_s": [],
           "grow_capacity_s": [], "results_equal": []}
    for _ in range(args.reps):
        m = warmed(W, 5)
        s, parts, nbytes, n = hand_over(m, W, 256)
        res["hand_over_s"].append(s)
        res["hand_over_parts_s"].append(parts)
        res["checkpoint_blob_bytes"] = int(nbytes)
        want = digest(n)
        del m, n
        m = warmed(W, 5)
        res["grow_capacity_s"].append(in_place(m, 256))
        res["results_equal"].append(digest(m) == want)
        del m
    res["hand_over_median_s"] = statistics.median(res["hand_over_s"])
    res["grow_capacity_median_s"] = statistics.median(res["grow_capacity_s"])
    off, on, caps = [], [], set()
    for _ in range(args.reps):
        ms, _ = headline(W, args.warmup, args.steps, False)
        off.append(ms)
        ms, cap = headline(W, args.warmup, args.steps, True)
        on.append(ms)
        caps.add(cap)
    res["headline_loop"] = {"steps": args.steps, "warmup": args.warmup, "auto_off_ms_per_step": off,
                            "auto_on_ms_per_step": on, "auto_off_median_ms": statistics.median(off),
                            "auto_on_median_ms": statistics.median(on),
                            "auto_on_final_capacities": sorted(caps)}
    res["headline_loop"]["auto_on_over_off"] = res["headline_loop"]["auto_on_median_ms"] / \
        res["headline_loop"]["auto_off_median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
