#!/usr/bin/env python3
"""What episodes cost on one GPU: nothing while a manager is unarmed, one small
kernel per step once it is armed, and one init's worth of stores for a step that
resets every world.

At --worlds worlds (65536) on bench.py's headline loop (step,
shift_observations, write_synthetic_actions), --reps alternating repeats per
variant in one process, each timed with device events around --steps steps after
--warmup warm-up steps (the end event after mbots_join, so the sensor's stream is
inside the span):

  1. with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1
     --steps 100 --warmup 20 of that tree and of this one, alternating, each in a
     process of its own.  The unarmed path must sit inside the parent's own
     run-to-run spread: |mean(branch) - mean(parent)| <= max(parent) - min(parent)
     of ms_per_step ("unarmed_within_parent_spread").
  2. the loop on an armed manager with no reset pending against an unarmed one:
     the reset pass's early-exit path, in us per step and in percent.
  3. one step that resets every world (mbots_reset_worlds of all of them, then
     step) against an ordinary step of the same manager, and building a new
     manager of that size.

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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part 1)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reset_cost.json"))
    args = ap.parse_args()
    W = args.worlds
    res = {"worlds": W, "steps": args.steps, "warmup": args.warmup, "reps": args.reps}

    if args.parent:
        par, br = [], []
        for _ in range(args.reps):
            par.append(bench_ms(os.path.abspath(args.parent)))
            br.append(bench_ms(ROOT))
        spread = max(par) - min(par)
        res["bench_unarmed"] = {
            "command": "bench.py --gpus 1 --steps 100 --warmup 20", "parent_ms_per_step": par,
            "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par), "branch_mean_ms": statistics.mean(br),
            "parent_spread_ms": spread,
            "unarmed_within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}

    import torch
    import madrona_bots as mb
    res["device"] = torch.cuda.get_device_name(0)

    def loop(m, t0, steps):
        for t in range(t0, t0 + steps):
            m.step()
            m.shift_observations()
            m.write_synthetic_actions(ACTION_SEED, t + 1)

    def timed_loop(m, t0, steps):
        """ms per step of `steps` iterations: device events, the sensor's stream joined"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.join()
        a.record()
        loop(m, t0, steps)
        m.join()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps

    # 2. armed, nothing pending, against unarmed
    unarmed, armed = [], []
    for _ in range(args.reps):
        for arm, into in ((False, unarmed), (True, armed)):
            m = mb.SimManager(0, W, SEED, A)
            if arm:
                m.reset_tensor()
            assert m.schedule_info()["episodes_armed"] == arm
            m.write_synthetic_actions(ACTION_SEED, 0)
            loop(m, 0, args.warmup)
            into.append(timed_loop(m, args.warmup, args.steps))
            del m
    mu, ma = statistics.mean(unarmed), statistics.mean(armed)
    res["armed_idle"] = {"unarmed_ms_per_step": unarmed, "armed_ms_per_step": armed, "unarmed_mean_ms": mu,
                         "armed_mean_ms": ma, "overhead_us_per_step": (ma - mu) * 1e3,
                         "overhead_percent": (ma - mu) / mu * 100.0,
                         "unarmed_spread_ms": max(unarmed) - min(unarmed)}

    # 3. a step that resets every world against an ordinary one; a new manager
    every = list(range(W))
    plain, reset_all, build = [], [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        m = mb.SimManager(0, W, SEED, A)
        torch.cuda.synchronize()
        build.append((time.perf_counter() - h0) * 1e3)
        m.reset_tensor()
        m.write_synthetic_actions(ACTION_SEED, 0)
        loop(m, 0, args.warmup)
        t = args.warmup
        for _ in range(4):   # alternating single steps
            plain.append(timed_loop(m, t, 1))
            m.reset_worlds(every)   # (the list's upload is outside the span: the flags are set)
            torch.cuda.synchronize()
            reset_all.append(timed_loop(m, t + 1, 1))
            t += 2
        assert int(m.episode_tensor().to_torch().min()) == 4
        del m
    res["reset_every_world"] = {"ordinary_step_ms": plain, "reset_step_ms": reset_all,
                                "ordinary_mean_ms": statistics.mean(plain), "reset_mean_ms": statistics.mean(reset_all),
                                "extra_us": (statistics.mean(reset_all) - statistics.mean(plain)) * 1e3,
                                "new_manager_ms": build, "new_manager_mean_ms": statistics.mean(build),
                                "note": "a step = step + shift_observations + write_synthetic_actions; the reset "
                                        "step runs on 32 agents per world, the ordinary one on the run's population"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
