#!/usr/bin/env python3
"""What the trajectory window's sequences cost on one GPU (include/mbots.h
"Sequences for a recurrent learner"), in the manner of scripts/traj_cost.py:
--worlds worlds (65536), a horizon of --horizon tables (16), bench.py's headline
loop (step, shift_observations, write_synthetic_actions), --reps alternating
repeats per variant, device events around --steps steps after --warmup.

  a. with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1
     --steps 100 --warmup 20 of that tree and of this one, alternating, each in a
     process of its own.  A manager without a window must sit inside the parent's
     own run-to-run spread: |mean(branch) - mean(parent)| <= max(parent) -
     min(parent) ("no_window_within_parent_spread").
  b. with --parent: the loop with a flagless push per step, this tree's library
     against the parent's, alternating, each in a process of its own; the same
     rule ("flagless_push_within_parent_spread").
  c. a push with record_obs and record_state, in us per step over the plain
     loop, beside what a learner does today to keep the same information:
     construct_obs() plus clones of the memory and action views each step.
  d. sequences() and batch(0, 65536) with obs over a full window: host wall
     time from the call to the device being idle; the obs kernel's bytes (from
     the shapes: the index read, the records of the rows that exist, the
     [L, B, 69] f32 written) over its device time as a share of --hbm-peak; and
     the torch-side equivalent for the same sequences beside it -- lifelines()
     of their start table plus one index gather per table from kept f32
     [N_t, 69] tensors.

The memory comparison is arithmetic, from the shapes.  Parts that were not run
say "not measured".  Writes every time and the means to --out (JSON)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, A, ACTION_SEED = 69, 32, 1234   # bench.py's
NOT = "not measured"


def bench_ms(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "100",
                          "--warmup", "20"], cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def child_push_ms(tree, args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-push", os.path.abspath(tree),
                          "--worlds", str(args.worlds), "--horizon", str(args.horizon), "--steps", str(args.steps),
                          "--warmup", str(args.warmup)], check=True, capture_output=True, text=True, timeout=600).stdout
    return float(out.split()[-1])


def within(par, br):
    spread = max(par) - min(par)
    return {"parent_ms_per_step": par, "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par),
            "branch_mean_ms": statistics.mean(br), "parent_spread_ms": spread,
            "within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--hbm-peak", type=float, default=8.0e12, help="bytes per second (MI355X: 8 TB/s)")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (parts a, b)")
    ap.add_argument("--child-push", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_sequences_cost.json"))
    args = ap.parse_args()
    W, T = args.worlds, args.horizon
    tree = args.child_push or ROOT
    sys.path.insert(0, os.path.join(tree, "madrona-bots_amd"))
    max_rows = W * 2 * A   # (the synthetic stream keeps a world near its initial population)

    def loop(m, t0, steps, win=None, value=None, keep=None):
        for t in range(t0, t0 + steps):
            m.step()
            if win is not None:
                if win.num_tables == T:
                    win.clear(keep_last=True)
                win.push(value)
            if keep is not None:
                keep(m)
            m.shift_observations()
            m.write_synthetic_actions(ACTION_SEED, t + 1)

    def timed_loop(torch, m, t0, steps, **kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        m.join()
        a.record()
        loop(m, t0, steps, **kw)
        m.join()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps

    if args.child_push:   # part b's process: the flagless push loop of `tree`
        import torch
        import madrona_bots as mb
        m = mb.SimManager(0, W, SEED, A)
        win = m.trajectory_window(T, max_rows)
        value = torch.rand(max_rows, dtype=torch.float32, device=m.device)
        win.push(value)
        m.write_synthetic_actions(ACTION_SEED, 0)
        loop(m, 0, args.warmup, win, value)
        print("ms_per_step", timed_loop(torch, m, args.warmup, args.steps, win=win, value=value))
        return

    res = {"worlds": W, "horizon": T, "steps": args.steps, "warmup": args.warmup, "reps": args.reps,
           "bench_no_window": NOT, "flagless_push": NOT}
    rec_bytes = 64
    res["memory_per_row_slot"] = {
        "window_all_flags_bytes": 32 + rec_bytes + 65 + 8, "learner_today_bytes": 276 + 64,
        "note": "window: 32 (flagless) + 64 (record) + 65 (HiddenState, action mask) + 8 (SEQ_ID, SEQ_POS); "
                "learner: one [69] f32 row + 16 f32 of memory"}

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
        res["bench_no_window"] = dict(within(par, br), command="bench.py --gpus 1 --steps 100 --warmup 20")
        res["bench_no_window"]["no_window_within_parent_spread"] = res["bench_no_window"].pop("within_parent_spread")
        save()
        par, br = [], []
        for _ in range(args.reps):
            par.append(child_push_ms(args.parent, args))
            br.append(child_push_ms(ROOT, args))
        res["flagless_push"] = within(par, br)
        res["flagless_push"]["flagless_push_within_parent_spread"] = res["flagless_push"].pop("within_parent_spread")
        save()

    import torch
    import madrona_bots as mb
    res["device"] = torch.cuda.get_device_name(0)

    # c. the recording push against the plain loop and against the learner's own copies
    def keep_today(m):
        m._kept = (m.construct_obs(), m.hidden_state_tensor().to_torch().clone(),
                   m.action_tensor().to_torch().clone())

    plain, recorded, today, obs_only, state_only = [], [], [], [], []
    flags = {"recorded": dict(record_obs=True, record_state=True), "obs_only": dict(record_obs=True),
             "state_only": dict(record_state=True)}
    for _ in range(args.reps):
        for variant, into in (("plain", plain), ("recorded", recorded), ("today", today), ("obs_only", obs_only),
                              ("state_only", state_only)):
            m = mb.SimManager(0, W, SEED, A)
            win = value = None
            if variant in flags:
                win = m.trajectory_window(T, max_rows, **flags[variant])
                value = torch.rand(max_rows, dtype=torch.float32, device=m.device)
                win.push(value)
            kw = dict(win=win, value=value, keep=keep_today if variant == "today" else None)
            m.write_synthetic_actions(ACTION_SEED, 0)
            loop(m, 0, args.warmup, **kw)
            into.append(timed_loop(torch, m, args.warmup, args.steps, **kw))
            if win is not None:
                win.close()
            del m
    mp = statistics.mean(plain)
    res["recording_push"] = {
        "plain_ms_per_step": plain, "recorded_ms_per_step": recorded, "learner_today_ms_per_step": today,
        "plain_spread_ms": max(plain) - min(plain),
        "recorded_overhead_us_per_step": (statistics.mean(recorded) - mp) * 1e3,
        "learner_today_overhead_us_per_step": (statistics.mean(today) - mp) * 1e3,
        "record_obs_only_ms_per_step": obs_only, "record_state_only_ms_per_step": state_only,
        "record_obs_only_overhead_us_per_step": (statistics.mean(obs_only) - mp) * 1e3,
        "record_state_only_overhead_us_per_step": (statistics.mean(state_only) - mp) * 1e3,
        "note": "recorded: push with record_obs | record_state (window chained with clear(keep_last)); learner "
                "today: construct_obs() plus clones of the memory and action views each step"}
    save()

    # d. sequences() and batch() with obs over a full window, and the torch-side equivalent
    m = mb.SimManager(0, W, SEED, A)
    win = m.trajectory_window(T, max_rows, record_obs=True, record_state=True)
    kept = []
    m.write_synthetic_actions(ACTION_SEED, 0)
    win.push()
    kept.append(m.construct_obs())
    for t in range(T - 1):
        m.step()
        win.push()
        kept.append(m.construct_obs())
        m.shift_observations()
        m.write_synthetic_actions(ACTION_SEED, t + 1)
    out = win.compute(0.99, 0.95)
    L = len(out["rows"])

    def wall(fn, n=3):
        fn()   # (warm)
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - h0) * 1e3)
        return ts, r

    def device_ms(fn, n=5):
        fn()
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return ts

    seq_ms, S = wall(win.sequences)
    B = min(args.batch, S)
    bufs = {k: torch.empty(s, dtype=d, device=m.device) for k, (s, d) in
            {"rows": ((L, B), torch.int32), "t0": ((B,), torch.int32), "len": ((B,), torch.int32),
             "obs": ((L, B, 69), torch.float32)}.items()}
    batch_ms, _ = wall(lambda: win.batch(0, B, out=bufs))
    index_only = {k: bufs[k] for k in ("rows", "t0", "len")}
    with_obs = device_ms(lambda: win.batch(0, B, out=bufs))
    without = device_ms(lambda: win.batch(0, B, out=index_only))
    obs_ms = statistics.mean(with_obs) - statistics.mean(without)
    present = int(bufs["len"].sum().item())
    obs_bytes = L * B * 4 + B * 4 + present * rec_bytes + L * B * 69 * 4

    def torch_side():
        t0 = bufs["t0"]
        first = int(t0.min().item())
        assert int(t0.max().item()) == first   # (the first B sequences all start in one table here)
        life = win.lifelines(first)[:, :B]
        o = torch.zeros((L, B, 69), dtype=torch.float32, device=m.device)
        for k in range(life.shape[0]):
            alive = life[k] >= 0
            o[k, alive] = kept[first + k][life[k][alive]]
        return o

    torch_ms, o = wall(torch_side)
    same = bool((o.view(torch.int32) == bufs["obs"].view(torch.int32)).all().item())
    res["sequences_and_batch"] = {
        "tables": L, "sequences": S, "batch": B, "rows_in_batch": present,
        "sequences_wall_ms": seq_ms, "sequences_mean_ms": statistics.mean(seq_ms),
        "batch_rows_t0_len_obs_wall_ms": batch_ms, "batch_mean_ms": statistics.mean(batch_ms),
        "batch_device_ms": with_obs, "batch_index_only_device_ms": without,
        "obs_kernel_ms": obs_ms, "obs_kernel_bytes": obs_bytes,
        "obs_kernel_share_of_hbm_peak": obs_bytes / (obs_ms * 1e-3) / args.hbm_peak if obs_ms > 0 else NOT,
        "hbm_peak_bytes_per_s": args.hbm_peak,
        "torch_side_wall_ms": torch_ms, "torch_side_mean_ms": statistics.mean(torch_ms),
        "torch_side_equals_batch": same,
        "note": "wall: host time from the call to the device being idle; obs_kernel_ms: device time of the "
                "batch with obs minus the batch without; torch side: lifelines() of the start table plus one "
                "index gather per table from kept f32 [N_t, 69] tensors"}
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
