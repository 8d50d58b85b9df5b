#!/usr/bin/env python3
"""What the learner's half of policy groups costs on one GPU (include/mbots.h
"Every group's nets in one call"), in the manner of scripts/policy_grad_cost.py:
--worlds worlds (65536) a few steps into bench.py's headline run, one table of
about 2.15 M rows, reference-sized nets (H = 128, a trunk of three Linear
layers, the actor and critic heads) with different random weights per (group,
species), every row evaluated through its net on act()'s actions, the loss
sum(g * output), one backward().

  bench. with --parent DIR (a built checkout of the parent commit): bench.py
     --gpus 1 --steps 100 --warmup 20 of that tree and of this one, alternating,
     each in a process of its own: a manager that never calls the new code
     must sit inside the parent's own run-to-run spread.
  a. --groups groups (32) of worlds / groups worlds each, 4 x groups nets: the
     per-net loop of harness/a2c_groups.py -- policy_segments().tolist(), one
     PolicyNet.evaluate per (group, species), one backward() -- against one
     evaluate_groups + backward(), alternating, --reps runs of --calls calls.
  b. one group: the four evaluate calls against one evaluate_groups.

Per call: wall ms (until the device is idle), device ms (events around the
calls), host ms (until the last launch is enqueued; the loop's includes its
.tolist() wait), and the peak device memory a call adds over what is allocated
before it (the cached workspaces are allocated by the warm call and reported
apart).  Writes every time, the means and the two verdicts to --out (JSON)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from policy_cost import bench_ms, SEED, A, ACTION_SEED, NOT, H   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part bench)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_eval_groups_cost.json"))
    args = ap.parse_args()
    res = {"worlds": args.worlds, "groups": args.groups, "reps": args.reps, "calls": args.calls, "bench_unused": NOT}

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
        res["bench_unused"] = {
            "command": "bench.py --gpus 1 --steps 100 --warmup 20", "parent_ms_per_step": par,
            "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par), "branch_mean_ms": statistics.mean(br),
            "parent_spread_ms": spread,
            "within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}
        save()

    sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd"))
    import torch
    import madrona_bots as mb
    nn = torch.nn
    res["device"] = torch.cuda.get_device_name(0)
    m = mb.SimManager(0, args.worlds, SEED, A)
    for t in range(4):
        m.write_synthetic_actions(ACTION_SEED, t)
        m.step()
        m.shift_observations()
    obs = m.construct_obs().clone()
    n = m.num_agents()
    g = [torch.randn(n, device=m.device) / n for _ in range(3)]
    res["rows"] = n

    def make_nets(groups, seed):
        torch.manual_seed(seed)
        nets, params = [], []
        for _ in range(groups):
            four = []
            for _ in range(4):
                feature = nn.Sequential(nn.Linear(69, H), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, H), nn.ReLU())
                actor = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 6))
                critic = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1))
                with torch.no_grad():
                    feature[0].weight.mul_(0.02)   # (unnormalised inputs: bytes up to 255)
                mods = [x.to(m.device) for x in (feature, actor, critic)]
                four.append(mb.PolicyNet.from_torch(*mods))
                params += [p for mod in mods for p in mod.parameters()]
            nets.append(four)
        return nets, params

    def measure(groups, seed):
        starts = [u * args.worlds // groups for u in range(groups)]
        m.set_policy_groups(starts if groups > 1 else None)
        nets, params = make_nets(groups, seed)
        for u in range(groups):
            m.set_policy(nets[u], group=u)
        action = m.act(write=False)["action"].clone()
        seg = torch.empty((groups, 4, 2), dtype=torch.int32, device=m.device)

        def loop():
            loss = 0.0
            for four, sg in zip(nets, m.policy_segments(out=seg).tolist()):
                for net, (lo, hi) in zip(four, sg):
                    if hi > lo:
                        out = net.evaluate(obs[lo:hi], action[lo:hi])
                        loss = loss + sum((q[lo:hi] * o).sum() for q, o in zip(g, out))
            loss.backward()

        def grouped():
            out = mb.evaluate_groups(nets, obs, action, m.policy_segments(out=seg))
            sum((q * o).sum() for q, o in zip(g, out)).backward()

        def run(fn):
            for p in params:
                p.grad = None
            fn()

        def timed(fn):
            run(fn)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            a.record()
            for _ in range(args.calls):
                run(fn)
            b.record()
            host = (time.perf_counter() - h0) * 1e3 / args.calls
            b.synchronize()
            wall = (time.perf_counter() - h0) * 1e3 / args.calls
            return wall, a.elapsed_time(b) / args.calls, host

        def peak_mb(fn):
            run(fn)
            for p in params:
                p.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            run(fn)
            torch.cuda.synchronize()
            return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

        out = {"nets": 4 * groups, "segment_rows_min_max": None}
        lens = (m.policy_segments()[..., 1] - m.policy_segments()[..., 0]).flatten().tolist()
        out["segment_rows_min_max"] = [min(lens), max(lens)]
        times = {"loop": [], "grouped": []}
        for _ in range(args.reps):
            times["loop"].append(timed(loop))
            times["grouped"].append(timed(grouped))
        for name, fn in (("loop", loop), ("grouped", grouped)):
            wall, dev, host = zip(*times[name])
            out[name] = {"wall_ms_per_call": list(wall), "device_ms_per_call": list(dev), "host_ms_per_call": list(host),
                         "mean_wall_ms": statistics.mean(wall), "mean_device_ms": statistics.mean(dev),
                         "mean_host_ms": statistics.mean(host), "wall_spread_ms": max(wall) - min(wall),
                         "peak_extra_mb": peak_mb(fn)}
        out["workspaces_mb"] = sorted(w.numel() / 2 ** 20 for w in mb._workspaces.values())
        gain = out["loop"]["mean_wall_ms"] - out["grouped"]["mean_wall_ms"]
        out["grouped_wall_minus_loop_ms"] = -gain
        out["loop_wall_spread_ms"] = out["loop"]["wall_spread_ms"]
        del nets, params
        return out

    a = measure(args.groups, 0)
    a["done_grouped_wall_below_loop_by_more_than_its_spread"] = \
        -a["grouped_wall_minus_loop_ms"] > a["loop_wall_spread_ms"]
    a["done_grouped_host_lower"] = a["grouped"]["mean_host_ms"] < a["loop"]["mean_host_ms"]
    res["a_groups"] = a
    save()
    mb._workspaces.clear()
    torch.cuda.empty_cache()
    b = measure(1, 1)
    b["done_grouped_within_loop_spread"] = b["grouped_wall_minus_loop_ms"] <= b["loop_wall_spread_ms"]
    res["b_one_group"] = b
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
