#!/usr/bin/env python3
"""What policy groups cost on one GPU (include/mbots.h "Acting on the device",
DESIGN.md "Policy groups"), in the manner of scripts/policy_cost.py: --worlds
worlds (65536) a few steps into bench.py's headline run, reference-sized nets
(H = 128, a trunk of three Linear layers with codes 0, 3, 1, the actor and
critic heads), different random weights per (group, species).

  a. with --parent DIR (a built checkout of the parent commit), alternating,
     each in a process of its own, --reps times:
       - bench.py --gpus 1 --steps 100 --warmup 20 (a manager without a policy);
       - act() with one group, device events around --calls calls.
     Each branch mean must sit inside the parent's own run-to-run spread:
     |mean(branch) - mean(parent)| <= max(parent) - min(parent).
  b. in one process, alternating, --reps times: act() with one group, with
     --groups (32) groups of the same architecture, and with --groups groups of
     mixed architectures (every other group H = 64, two trunk layers, a memory
     head and memory_in); and act() of one manager of worlds / groups worlds,
     what a user pays per universe with one manager per universe.

Parts that were not run say "not measured".  Writes every time, the means and
the spreads to --out (JSON)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, A, ACTION_SEED = 69, 32, 1234   # bench.py's
NOT = "not measured"
H = 128


def bench_ms(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "100",
                          "--warmup", "20", "--no-cpu-baseline", "--no-secondary"], cwd=tree, check=True,
                         capture_output=True, text=True, timeout=600).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def summary(xs):
    return {"runs": xs, "mean": statistics.mean(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs)}


def make_models(torch, n, device, small=False):
    """n (feature, actor, critic, memory) stacks of random weights."""
    nn = torch.nn
    out = []
    for _ in range(n):
        if small:
            h = 64
            feature = nn.Sequential(nn.Linear(85, h), nn.Tanh(), nn.Linear(h, h), nn.ReLU())
            memory = nn.Sequential(nn.Linear(h, 16), nn.Tanh())
        else:
            h = H
            feature = nn.Sequential(nn.Linear(69, h), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, h), nn.ReLU())
            memory = None
        actor = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 6))
        critic = nn.Sequential(nn.Linear(h, h), nn.ReLU(), nn.Linear(h, 1))
        with torch.no_grad():
            feature[0].weight.mul_(0.02)   # (unnormalised inputs: bytes up to 255)
        out.append(tuple(None if x is None else x.to(device).requires_grad_(False)
                         for x in (feature, actor, critic, memory)))
    return out


def make_manager(mb, torch, worlds, groups=1, mixed=False):
    m = mb.SimManager(0, worlds, SEED, A)
    for t in range(4):
        m.write_synthetic_actions(ACTION_SEED, t)
        m.step()
        m.shift_observations()
    if groups > 1:
        m.set_policy_groups(list(range(0, worlds, worlds // groups))[:groups])
    for g in range(groups):
        small = mixed and g % 2 == 1
        nets = [mb.PolicyNet.from_torch(f, a, c, memory=mem, memory_in=small)
                for f, a, c, mem in make_models(torch, 4, m.device, small)]
        if groups > 1:
            m.set_policy(nets, group=g)
        else:
            m.set_policy(nets)
    n = m.num_agents()
    out = {k: torch.empty((n, 1), dtype=d, device=m.device)
           for k, d in (("action", torch.int32), ("logp", torch.float32), ("value", torch.float32))}
    return m, out


def device_ms(torch, fn, calls):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def worker_one_group(args):
    """act() with one group in the tree --tree: one JSON line of the times."""
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "madrona-bots_amd"))
    import torch
    import madrona_bots as mb
    torch.manual_seed(0)
    m, out = make_manager(mb, torch, args.worlds)
    for _ in range(3):   # warm-up
        device_ms(torch, lambda: m.act(out=out), args.calls)
    print(json.dumps({"ms": [device_ms(torch, lambda: m.act(out=out), args.calls) for _ in range(args.reps)],
                      "rows": m.num_agents()}))


def one_group_ms(tree, args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--worlds",
                          str(args.worlds), "--reps", str(args.reps), "--calls", str(args.calls)], check=True,
                         capture_output=True, text=True, timeout=600).stdout
    return statistics.mean(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["ms"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_groups_cost.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker_one_group(args)
    res = {"worlds": args.worlds, "groups": args.groups, "reps": args.reps, "calls": args.calls,
           "bench_no_policy": NOT, "act_one_group_vs_parent": NOT}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    if args.parent:
        parent = os.path.abspath(args.parent)
        for key, fn, unit in (("bench_no_policy", bench_ms, "ms_per_step"),
                              ("act_one_group_vs_parent", lambda tree: one_group_ms(tree, args), "device_ms_per_call")):
            par, br = [], []
            for _ in range(args.reps):
                par.append(fn(parent))
                br.append(fn(ROOT))
            p, b = summary(par), summary(br)
            res[key] = {"unit": unit, "parent": p, "branch": b,
                        "within_parent_spread": abs(b["mean"] - p["mean"]) <= p["spread"]}
            save()

    sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd"))
    import torch
    import madrona_bots as mb
    res["device"] = torch.cuda.get_device_name(0)
    torch.manual_seed(0)
    G = args.groups
    cases = {"one_group": make_manager(mb, torch, args.worlds),
             "groups_same_architecture": make_manager(mb, torch, args.worlds, G),
             "groups_mixed_architectures": make_manager(mb, torch, args.worlds, G, mixed=True),
             "one_manager_per_universe": make_manager(mb, torch, args.worlds // G)}
    rows = cases["one_group"][0].num_agents()
    res["rows"] = rows
    # from the code: one ragged tile more per segment at most
    res["tile_share_bound"] = 4 * G / (rows / 64)
    times = {k: [] for k in cases}
    for k, (m, out) in cases.items():   # warm-up
        for _ in range(3):
            device_ms(torch, lambda: m.act(out=out), args.calls)
    for _ in range(args.reps):
        for k, (m, out) in cases.items():
            times[k].append(device_ms(torch, lambda: m.act(out=out), args.calls))
    res["act_device_ms_per_call"] = {k: summary(v) for k, v in times.items()}
    one = statistics.mean(times["one_group"])
    res["groups_same_over_one_group"] = statistics.mean(times["groups_same_architecture"]) / one
    res["groups_mixed_over_one_group"] = statistics.mean(times["groups_mixed_architectures"]) / one
    res["universes_in_one_manager_over_one_manager_each"] = \
        statistics.mean(times["groups_same_architecture"]) / (G * statistics.mean(times["one_manager_per_universe"]))
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
