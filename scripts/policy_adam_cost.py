#!/usr/bin/env python3
"""What the device learner step costs on one GPU (include/mbots.h "The update on
the device"; DESIGN.md "Device learner step"), in the manner of
scripts/policy_eval_groups_cost.py: --groups groups (32) of four
reference-sized nets each (H = 128, a trunk of three Linear layers, the actor
and critic heads), 9.7 M parameters in 1 792 tensors.

  bench. with --parent DIR (a built checkout of the parent commit): bench.py
     --gpus 1 --steps 100 --warmup 20 of that tree and of this one, alternating,
     each in a process of its own: a manager that never calls the new code
     must sit inside the parent's own run-to-run spread.
  a. the optimiser, gradients filled once: the 4 x groups torch.optim.Adam
     instances harness/a2c_groups.py builds (one per species module), one
     torch.optim.Adam over all parameters (torch's best case), and
     PolicyAdam.step, eagerly and as a captured graph's replay (the kernels
     without the wrapper's host loop) -- alternating, --reps runs of at least
     20 calls each.  For the replay also the bytes the pass moves (seven f32
     streams per element) over its device time, and that rate's share of
     --hbm-tbs.
  b. the loss of one table of --rows rows (2.15 M) in 4 x groups equal
     segments: the composition of harness/a2c_groups.py's grouped_update
     (group weights by index_add_ / cumsum, the per-row expression, .sum(),
     index_add_ per group, and autograd back to the three outputs) against
     a2c_loss_groups.
  c. with --worlds > 0: one whole update of harness/a2c_groups.py at that many
     worlds (65536), horizon --horizon, on the same recorded tables:
     grouped_update with the 4 x groups torch optimizers against
     device_update_step.

Per call: wall ms (until the device is idle), device ms (events around the
calls) and host ms (until the last launch is enqueued).  Writes every time,
the means and the spreads to --out (JSON)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from policy_cost import bench_ms   # noqa: E402

H = 128


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2_150_000)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM peak DESIGN.md section 5 quotes, TB/s")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part bench)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_adam_cost.json"))
    args = ap.parse_args()
    G = args.groups
    res = {"groups": G, "reps": args.reps, "calls": args.calls}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    def timed(fn, calls):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        host = (time.perf_counter() - h0) * 1e3 / calls
        b.synchronize()
        wall = (time.perf_counter() - h0) * 1e3 / calls
        return wall, a.elapsed_time(b) / calls, host

    def contest(contenders, calls):
        times = {name: [] for name in contenders}
        for _ in range(args.reps):
            for name, fn in contenders.items():
                times[name].append(timed(fn, calls))
        out = {}
        for name, rows in times.items():
            wall, device, host = zip(*rows)
            out[name] = {"wall_ms_per_call": list(wall), "device_ms_per_call": list(device),
                         "host_ms_per_call": list(host), "mean_wall_ms": statistics.mean(wall),
                         "mean_device_ms": statistics.mean(device), "mean_host_ms": statistics.mean(host),
                         "wall_spread_ms": max(wall) - min(wall)}
        return out

    res["bench_unused"] = "not measured (no --parent)"
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
    sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd", "harness"))
    import torch                     # (after the benchmark's child processes: they start from a process without a GPU)
    import madrona_bots as mb
    import a2c
    import a2c_groups
    if not torch.cuda.is_available():
        raise SystemExit("policy_adam_cost.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    res["device"] = torch.cuda.get_device_name(0)

    # ---- a. the optimiser ----
    modules = [a2c.make_modules(H, dev, seed=u) for u in range(G)]
    nets = [[mb.PolicyNet.from_torch(m["feature"], m["actor"], m["critic"]) for m in four] for four in modules]
    params = [p for four in modules for m in four for p in m.parameters()]
    torch.manual_seed(1)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    per_module = [[torch.optim.Adam(m.parameters(), lr=3e-4) for m in four] for four in modules]
    single = torch.optim.Adam(params, lr=3e-4)
    fused = mb.PolicyAdam(nets, lr=3e-4)
    elements = sum(p.numel() for p in params)

    def step_per_module():
        for opts in per_module:
            for opt in opts:
                opt.step()
    # (PolicyAdam.step's own time is its host loop over the descriptors; the kernels' time is that of a replay)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused.step()
    a = contest({"torch_adam_per_module": step_per_module, "torch_adam_single": single.step,
                 "policy_adam": fused.step, "policy_adam_graph_replay": graph.replay}, max(args.calls, 20))
    nbytes = 7 * 4 * elements
    rate = nbytes / (a["policy_adam_graph_replay"]["mean_device_ms"] * 1e-3) / 1e12
    a.update({"tensors": len(params), "elements": elements, "optimizers_per_module": 4 * G,
              "policy_adam_bytes": nbytes, "policy_adam_tb_per_s": rate, "hbm_tb_per_s": args.hbm_tbs,
              "policy_adam_share_of_hbm_rate": rate / args.hbm_tbs,
              "policy_adam_ms_at_hbm_rate": nbytes / (args.hbm_tbs * 1e12) * 1e3,
              "policy_adam_launches": (len(params) + 63) // 64 + 1})
    res["a_optimiser"] = a
    save()

    # ---- b. the loss of one table ----
    n = args.rows
    torch.manual_seed(2)
    cols = [torch.randn(n, device=dev) for _ in range(5)]
    end = torch.randint(0, 4, (n, 1), dtype=torch.int32, device=dev)
    edges = [k * n // (4 * G) for k in range(4 * G + 1)]
    seg = torch.tensor([[lo, hi] for lo, hi in zip(edges[:-1], edges[1:])], dtype=torch.int32,
                       device=dev).reshape(G, 4, 2)
    total = mb.policy_group_rows(seg, torch.zeros(G, dtype=torch.int64, device=dev))
    value_coef, entropy_coef = 0.5, 0.01

    def torch_loss():
        logp, value, entropy = (c.detach().requires_grad_() for c in cols[:3])
        spans = seg.to(torch.int64)
        count = (spans[..., 1] - spans[..., 0]).sum(dim=1)
        weight = torch.cat([torch.zeros(1, device=dev), torch.where(count > 0, 1.0 / count.to(torch.float32), 0.0)])
        ids = torch.arange(1, G + 1, device=dev).repeat_interleave(4)
        edge = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        edge.index_add_(0, spans[:, :, 0].reshape(-1), ids)
        edge.index_add_(0, spans[:, :, 1].reshape(-1), -ids)
        group = edge.cumsum(0)[:n]
        keep = (end.reshape(-1) != 2).to(torch.float32)
        per_row = (-cols[3] * logp + value_coef * (value - cols[4]) ** 2 - entropy_coef * entropy) * (keep * weight[group])
        per_group = torch.zeros(G + 1, device=dev)
        per_group.index_add_(0, group, per_row.detach())
        return torch.autograd.grad(per_row.sum(), [logp, value, entropy]), per_group

    def library_loss():
        return mb.a2c_loss_groups(*cols, end, seg, total, value_coef, entropy_coef)
    b = contest({"torch_composition": torch_loss, "a2c_loss_groups": library_loss}, args.calls)
    b["rows"] = n
    res["b_loss"] = b
    save()
    del cols, end

    # ---- c. one whole update on recorded tables ----
    if args.worlds > 0:
        sim = mb.SimManager(0, args.worlds, 69, 32)
        starts = [u * args.worlds // G for u in range(G)]
        sim.set_policy_groups(starts)
        for u in range(G):
            sim.set_policy(nets[u], group=u)
        win = sim.trajectory_window(args.horizon, max_rows=sim.num_worlds * sim.agent_capacity)
        rows = []
        for t in range(args.horizon):
            last = t == args.horizon - 1
            obs = None if last else sim.construct_obs().clone()
            o = sim.act(write=not last)
            win.push(o["value"])
            if not last:
                rows.append((obs, o["action"], sim.policy_segments().clone()))
                sim.step()
        out = win.compute(gamma=0.99, lam=0.95, death_reward=-1.0)

        def torch_update():
            a2c_groups.grouped_update(mb, nets, per_module, rows, out, win.END_RESET, value_coef, entropy_coef)

        def device_update():
            a2c_groups.device_update_step(mb, nets, fused, rows, out, value_coef, entropy_coef)
        c = contest({"grouped_evaluate": torch_update, "device_update": device_update}, 1)
        c.update({"worlds": args.worlds, "tables": len(rows), "rows_per_table": [r[0].shape[0] for r in rows]})
        res["c_whole_update"] = c
        win.close()
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
