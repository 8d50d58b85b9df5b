#!/usr/bin/env python3
"""What the recurrent learner's half of policy groups costs on one GPU
(include/mbots.h "Every group's recurrent nets in one call"), in the manner of
scripts/policy_eval_groups_cost.py: --worlds worlds (65536) a few steps into
bench.py's headline run, reference-sized recurrent nets (H = 128, a trunk of
three Linear layers, the actor and critic heads, a memory head, memory_in) with
different random weights per (group, species), acting through a window of
--horizon tables (16); the batch is --batch sequences (65536) of that window,
every k-th of its sequences so that every net has columns, scattered through
the batch as the window hands them out; the loss sum(g * output), one
backward().

  bench. with --parent DIR (a built checkout of the parent commit): bench.py
     --gpus 1 --steps 100 --warmup 20 of that tree and of this one, alternating,
     each in a process of its own: a manager that never calls the new code
     must sit inside the parent's own run-to-run spread.
  a. --groups groups (32) of worlds / groups worlds each, 4 x groups nets: the
     per-net loop -- per net torch.nonzero(net_id == e), index_select of obs,
     action, len, hidden0 and the g_*, one PolicyNet.evaluate_sequences, then
     one backward() -- against sequence_segments + one
     evaluate_sequences_groups + backward(), alternating, --reps runs of
     --calls calls.
  b. one group: the four evaluate_sequences calls against the grouped call.

Per call: wall ms (until the device is idle), device ms (events around the
calls), host ms (until the last launch is enqueued; the loop's includes its
nonzero waits), and the peak device memory a call adds over what is allocated
before it (the cached workspaces are allocated by the warm call and reported
apart).  Writes every time, the means and the verdicts to --out (JSON)."""
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
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part bench)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_seq_groups_cost.json"))
    args = ap.parse_args()
    res = {"worlds": args.worlds, "groups": args.groups, "horizon": args.horizon, "reps": args.reps,
           "calls": args.calls, "bench_unused": NOT}

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

    def make_nets(groups, seed, dev):
        torch.manual_seed(seed)
        nets, params = [], []
        for _ in range(groups):
            four = []
            for _ in range(4):
                feature = nn.Sequential(nn.Linear(85, H), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, H), nn.ReLU())
                actor = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 6))
                critic = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1))
                memory = nn.Sequential(nn.Linear(H, 16), nn.Tanh())
                with torch.no_grad():
                    feature[0].weight[:, :69].mul_(0.02)   # (unnormalised inputs: bytes up to 255)
                mods = [x.to(dev) for x in (feature, actor, critic, memory)]
                four.append(mb.PolicyNet.from_torch(*mods, memory_in=True))
                params += [p for mod in mods for p in mod.parameters()]
            nets.append(four)
        return nets, params

    def measure(groups, seed):
        m = mb.SimManager(0, args.worlds, SEED, A)
        for t in range(4):
            m.write_synthetic_actions(ACTION_SEED, t, True)
            m.step()
            m.shift_observations()
        starts = [u * args.worlds // groups for u in range(groups)]
        m.set_policy_groups(starts if groups > 1 else None)
        nets, params = make_nets(groups, seed, m.device)
        for u in range(groups):
            m.set_policy(nets[u], group=u)
        # a real window: act() through --horizon tables, then every k-th sequence of it
        win = m.trajectory_window(args.horizon, max_rows=2 * m.num_agents() + 4096, record_obs=True,
                                  record_state=True)
        actions, species = [], []
        for t in range(args.horizon):
            win.push()
            actions.append(m.act()["action"])
            count = m.species_count_tensor().to_torch().sum(dim=0).to(torch.int64)
            species.append(torch.repeat_interleave(torch.arange(4, device=count.device), count).to(torch.int32)
                           .reshape(-1, 1))
            if t + 1 < args.horizon:
                m.step()
        view = win.compute(gamma=0.99)
        S = win.sequences()
        B = min(args.batch, S)
        cols = (torch.arange(B, device=m.device, dtype=torch.int64) * S) // B
        b = win.batch(keys=("len", "obs", "hidden0"))
        world = win.gather([w.to(torch.int32) for w in view["world"]])[0, :, 0].index_select(0, cols).to(torch.int64)
        sp = win.gather(species)[0, :, 0].index_select(0, cols).to(torch.int64)
        action = win.gather(actions)[:, :, 0].index_select(1, cols).contiguous()
        obs = b["obs"].index_select(1, cols).contiguous()
        length, hidden0 = b["len"].index_select(0, cols).contiguous(), b["hidden0"].index_select(0, cols).contiguous()
        group = torch.bucketize(world, torch.tensor(starts, device=m.device), right=True) - 1
        net_id = (group * 4 + sp).to(torch.int32)
        del b
        win.close()
        del m
        torch.cuda.empty_cache()
        L = obs.shape[0]
        g = [torch.randn(L, B, device=obs.device) / (L * B) for _ in range(3)]

        def loop():
            loss = 0.0
            for e, net in enumerate(x for four in nets for x in four):
                c = torch.nonzero(net_id == e).reshape(-1)
                if c.numel() == 0:
                    continue
                out = net.evaluate_sequences(obs.index_select(1, c), action.index_select(1, c), length[c], hidden0[c])
                loss = loss + sum((q.index_select(1, c) * o).sum() for q, o in zip(g, out))
            loss.backward()

        def grouped():
            order, seg = mb.sequence_segments(net_id, groups)
            out = mb.evaluate_sequences_groups(nets, obs, action, length, hidden0, order, seg)
            sum((q * o).sum() for q, o in zip(g, out)).backward()

        def run(fn):
            for p in params:
                p.grad = None
            fn()

        def timed(fn):
            run(fn)
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            h0 = time.perf_counter()
            a.record()
            for _ in range(args.calls):
                run(fn)
            z.record()
            host = (time.perf_counter() - h0) * 1e3 / args.calls
            z.synchronize()
            wall = (time.perf_counter() - h0) * 1e3 / args.calls
            return wall, a.elapsed_time(z) / args.calls, host

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

        sizes = torch.bincount(net_id.to(torch.int64), minlength=4 * groups).tolist()
        out = {"nets": 4 * groups, "sequences": B, "window_sequences": S, "L": L,
               "present_elements": int(length.sum()), "segment_columns_min_max": [min(sizes), max(sizes)]}
        times = {"loop": [], "grouped": []}
        for _ in range(args.reps):
            times["grouped"].append(timed(grouped))
            times["loop"].append(timed(loop))
        for name, fn in (("loop", loop), ("grouped", grouped)):
            wall, dev, host = zip(*times[name])
            out[name] = {"wall_ms_per_call": list(wall), "device_ms_per_call": list(dev), "host_ms_per_call": list(host),
                         "mean_wall_ms": statistics.mean(wall), "mean_device_ms": statistics.mean(dev),
                         "mean_host_ms": statistics.mean(host), "wall_spread_ms": max(wall) - min(wall),
                         "device_spread_ms": max(dev) - min(dev), "host_spread_ms": max(host) - min(host),
                         "peak_extra_mb": peak_mb(fn)}
        out["workspaces_mb"] = sorted(w.numel() / 2 ** 20 for w in mb._workspaces.values())
        out["grouped_wall_minus_loop_ms"] = out["grouped"]["mean_wall_ms"] - out["loop"]["mean_wall_ms"]
        out["loop_wall_spread_ms"] = out["loop"]["wall_spread_ms"]
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
