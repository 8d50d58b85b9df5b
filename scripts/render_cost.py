#!/usr/bin/env python3
"""What a render_worlds call costs on one GPU, beside the least time its output
bytes could take.

Three cases, each on a manager stepped --steps times on bench.py's synthetic
action stream first (so the worlds hold births, food and agents of every
health), rendering into preallocated outputs with the NULL world list (nothing
uploaded):

  1. 64 worlds at scale 8, all three outputs (a person's frames);
  2. every world of a 4096-world manager at scale 1, cls only (a critic's maps);
  3. every world of a 65536-world manager at scale 1, cls only.

A case is warmed up with --warmup calls; then --runs measurements, each the
device-event time around --inner back-to-back calls divided by --inner (the
stream is idle before the first event, so a measurement is kernel time plus the
launch gaps between the calls); the figure is the median.  floor_us is the
output bytes over the HBM peak bench.py uses (HBM_PEAK_GBS): the kernel also
reads the worlds' state, a few percent of what it writes at scale 1 and far
less above.  Writes --out (JSON)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd"))

SEED, A, ACTION_SEED = 69, 32, 1234   # bench.py's

CASES = (("frames_64_worlds_scale_8_all_outputs", 64, 8, ("rgb", "cls", "slot")),
         ("maps_4096_worlds_scale_1_cls", 4096, 1, ("cls",)),
         ("maps_65536_worlds_scale_1_cls", 65536, 1, ("cls",)))
BYTES = {"rgb": 3, "cls": 1, "slot": 2}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_cost.json"))
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")

    import torch
    import madrona_bots as mb
    from bench import HBM_PEAK_GBS
    if not torch.cuda.is_available():
        raise SystemExit("render_cost.py measures on a GPU: none is present")
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS, "steps_before": args.steps,
           "warmup": args.warmup, "runs": args.runs, "calls_per_run": args.inner, "cases": {}}
    for name, W, scale, keys in CASES:
        m = mb.SimManager(0, W, SEED, A)
        for t in range(args.steps):
            m.write_synthetic_actions(ACTION_SEED, t)
            m.step()
        H, Wp = 96 * scale, 128 * scale
        shape = {"rgb": (W, H, Wp, 3), "cls": (W, H, Wp), "slot": (W, H, Wp)}
        dtype = {"rgb": torch.uint8, "cls": torch.uint8, "slot": torch.int16}
        out = {k: torch.empty(shape[k], dtype=dtype[k], device=m.device) for k in keys}
        nbytes = sum(W * H * Wp * BYTES[k] for k in keys)
        for _ in range(args.warmup):
            m.render_worlds(None, scale, out=out)
        times = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.inner):
                m.render_worlds(None, scale, out=out)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / args.inner)
        med = statistics.median(times)
        floor = nbytes / (HBM_PEAK_GBS * 1e9) * 1e6
        res["cases"][name] = {"manager_worlds": W, "images": W, "scale": scale, "outputs": list(keys),
                              "agents": m.num_agents(), "output_bytes": nbytes, "us_per_call": times,
                              "median_us": med, "min_us": min(times), "max_us": max(times),
                              "floor_us": floor, "ratio_to_floor": med / floor,
                              "achieved_write_gbs": nbytes / (med * 1e-6) / 1e9}
        del out, m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {q: v[q] for q in ("median_us", "floor_us", "ratio_to_floor")}
                      for k, v in res["cases"].items()}))


if __name__ == "__main__":
    main()
