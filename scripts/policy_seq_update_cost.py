#!/usr/bin/env python3
"""What the recurrent device update costs on one GPU (include/mbots.h "The
recurrent update on the device"; DESIGN.md "Device learner step"), in the
manner of scripts/policy_adam_cost.py: --groups groups (32) of four
reference-sized recurrent nets each (H = 128, harness/a2c_recurrent.py's
modules).

  bench. with --parent DIR (a built checkout of the parent commit): bench.py
     --gpus 1 --steps 100 --warmup 20 of that tree and of this one, alternating,
     each in a process of its own; and PolicyAdam.step without options of
     either tree (this script's --plain-step mode in a child process,
     alternating): code that calls none of the new entry points must sit
     inside the parent's own run-to-run spread.
  a. the optimiser, gradients filled once, eagerly and as a captured graph's
     replay: PolicyAdam.step with max_grad_norm against without it; against
     clip_grad_norm_ per group + the plain PolicyAdam.step; against
     clip_grad_norm_ per group + the 4 x groups torch.optim.Adam.
  b. sequence_group_rows + a2c_loss_sequences at --seqs sequences (65536) of
     L = --steps (16) against harness/a2c_recurrent_groups.py's torch
     composition (keep, total, weight, per.sum(), index_add_, and autograd
     back to the three outputs), with --groups groups and with one group (the
     one-block case of the loss kernel).
  c. with --worlds > 0: one whole update of harness/a2c_recurrent_groups.py at
     that many worlds on one recorded window: the --grouped-evaluate body
     (torch loss, 4 x groups torch optimizers) against device_update_step.

Per call: wall ms (until the device is idle), device ms (events around the
calls) and host ms (until the last launch is enqueued); --reps alternating
runs per contender in one process, mean and max - min spread.  Writes to
--out (JSON)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--seqs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part bench)")
    ap.add_argument("--plain-step", default=None, metavar="TREE",
                    help="(child mode) time PolicyAdam.step without options with TREE's package; print JSON")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_seq_update_cost.json"))
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

    def replay_of(fn):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fn()
        return graph

    tree = os.path.abspath(args.plain_step) if args.plain_step else ROOT
    if args.parent and not args.plain_step:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        from policy_cost import bench_ms
        par, br, par_step, br_step = [], [], [], []
        for _ in range(args.reps):
            par.append(bench_ms(os.path.abspath(args.parent)))
            br.append(bench_ms(ROOT))
            for where, dst in ((os.path.abspath(args.parent), par_step), (ROOT, br_step)):
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-step", where, "--groups",
                                      str(G)], capture_output=True, text=True, check=True)
                dst.append(json.loads(out.stdout.strip().splitlines()[-1]))
            print(f"bench: parent {par[-1]:.4f} ms, branch {br[-1]:.4f} ms per step", file=sys.stderr, flush=True)
        spread = max(par) - min(par)
        res["bench_unused"] = {
            "command": "bench.py --gpus 1 --steps 100 --warmup 20", "parent_ms_per_step": par,
            "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par), "branch_mean_ms": statistics.mean(br),
            "parent_spread_ms": spread,
            "within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}
        res["plain_step_unused"] = {}
        for key in ("eager_wall_ms", "replay_device_ms"):
            p, b = [x[key] for x in par_step], [x[key] for x in br_step]
            res["plain_step_unused"][key] = {
                "parent": p, "branch": b, "parent_mean": statistics.mean(p), "branch_mean": statistics.mean(b),
                "parent_spread": max(p) - min(p),
                "within_parent_spread": abs(statistics.mean(b) - statistics.mean(p)) <= max(p) - min(p)}
        save()

    sys.path.insert(0, os.path.join(tree, "madrona-bots_amd"))
    sys.path.insert(0, os.path.join(tree, "madrona-bots_amd", "harness"))
    import torch                     # (after the benchmark's child processes: they start from a process without a GPU)
    import madrona_bots as mb
    import a2c_recurrent
    import a2c_recurrent_groups as arg
    if not torch.cuda.is_available():
        raise SystemExit("policy_seq_update_cost.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    res["device"] = torch.cuda.get_device_name(0)

    modules = [a2c_recurrent.make_modules(H, dev, seed=u) for u in range(G)]
    nets = [[a2c_recurrent.policy_net(m) for m in four] for four in modules]
    params = [p for four in modules for m in four for p in m.parameters()]
    group_params = [[p for m in four for p in m.parameters()] for four in modules]
    torch.manual_seed(1)
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    plain = mb.PolicyAdam(nets, lr=3e-4)

    if args.plain_step:
        graph = replay_of(plain.step)
        runs = [timed(plain.step, 20) for _ in range(3)]
        reps = [timed(graph.replay, 20) for _ in range(3)]
        print(json.dumps({"eager_wall_ms": statistics.mean(r[0] for r in runs),
                          "replay_device_ms": statistics.mean(r[1] for r in reps)}))
        return

    # ---- a. the optimiser ----
    clipped = mb.PolicyAdam(nets, lr=3e-4, max_grad_norm=0.5)
    per_module = [[torch.optim.Adam(m.parameters(), lr=3e-4) for m in four] for four in modules]

    def torch_clip():
        for ps in group_params:
            torch.nn.utils.clip_grad_norm_(ps, 0.5)

    def torch_clip_plain_step():
        torch_clip()
        plain.step()

    def torch_clip_torch_adam():
        torch_clip()
        for opts in per_module:
            for opt in opts:
                opt.step()
    graphs = {"policy_adam_graph_replay": replay_of(plain.step), "policy_adam_clip_graph_replay": replay_of(clipped.step)}
    try:
        graphs["torch_clip_policy_adam_graph_replay"] = replay_of(torch_clip_plain_step)
    except RuntimeError as e:        # (a torch build whose clip_grad_norm_ cannot be captured)
        res["torch_clip_policy_adam_graph_replay"] = "not measured: " + str(e).splitlines()[0]
    a = contest({"policy_adam": plain.step, "policy_adam_clip": clipped.step,
                 "torch_clip_policy_adam": torch_clip_plain_step, "torch_clip_torch_adam": torch_clip_torch_adam,
                 **{k: g.replay for k, g in graphs.items()}}, max(args.calls, 20))
    a.update({"tensors": len(params), "elements": sum(p.numel() for p in params),
              "policy_adam_clip_launches": 3 * ((len(params) + 63) // 64) + 2})
    res["a_optimiser"] = a
    save()
    del graphs

    # ---- b. the count and the loss of one sequence batch ----
    L, B = args.steps, args.seqs
    value_coef, entropy_coef, horizon = 0.5, 0.01, L + 1
    res["b_loss"] = {"sequences": B, "L": L}
    for label, Gb in (("groups_%d" % G, G), ("groups_1", 1)):
        torch.manual_seed(2)
        cols = [torch.randn(L, B, device=dev) for _ in range(5)]
        length = torch.randint(0, L + 1, (B,), dtype=torch.int32, device=dev)
        t0 = torch.randint(0, 4, (B,), dtype=torch.int32, device=dev)
        end = torch.randint(0, 4, (B,), dtype=torch.int32, device=dev)
        group = torch.randint(0, Gb, (B,), device=dev)
        net_id = (group * 4 + torch.randint(0, 4, (B,), device=dev)).to(torch.int32)
        order, seg = mb.sequence_segments(net_id, Gb)
        rows_live = (torch.arange(L, device=dev, dtype=torch.int32)[:, None] < length[None, :]).to(torch.int32) * 2 - 1

        def torch_loss():
            logp, value, entropy = (c.detach().requires_grad_() for c in cols[:3])
            k = torch.arange(L, device=dev, dtype=torch.int32)[:, None]
            keep = (rows_live >= 0) & (t0[None, :] + k < horizon - 1)
            keep &= ~((end == 2)[None, :] & (k == length[None, :] - 1))
            keep = keep.to(torch.float32)
            total = torch.zeros(Gb, device=dev).index_add_(0, group, keep.sum(dim=0)).clamp_(min=1.0)
            weight = (1.0 / total)[group]
            per = arg.per_element(logp, value, entropy, cols[3], cols[4], value_coef, entropy_coef)
            per = per * (keep * weight[None, :])
            per_group = torch.zeros(Gb, device=dev).index_add_(0, group, per.detach().sum(dim=0))
            return torch.autograd.grad(per.sum(), [logp, value, entropy]), per_group

        def library_loss():
            total = mb.sequence_group_rows(length, t0, end, order, seg, torch.zeros(Gb, dtype=torch.int64, device=dev),
                                           horizon - 1)
            return mb.a2c_loss_sequences(*cols, length, t0, end, order, seg, total, horizon - 1, value_coef,
                                         entropy_coef)
        res["b_loss"][label] = contest({"torch_composition": torch_loss, "sequence_rows_and_loss": library_loss,
                                        "sequence_rows_and_loss_graph_replay": replay_of(library_loss).replay},
                                       args.calls)
        save()
    del cols

    # ---- c. one whole update on one recorded window ----
    if args.worlds > 0:
        sim = mb.SimManager(0, args.worlds, 69, 32)
        starts = [u * args.worlds // G for u in range(G)]
        sim.set_policy_groups(starts)
        for u in range(G):
            sim.set_policy(nets[u], group=u)
        starts_dev = torch.tensor(starts, dtype=torch.int64, device=dev)
        win = sim.trajectory_window(args.horizon, max_rows=sim.num_worlds * sim.agent_capacity, record_obs=True,
                                    record_state=True)
        out, actions, _, species = a2c_recurrent.rollout(sim, win, args.horizon)
        worlds = [w.to(torch.int32) for w in out["world"]]
        b, action, net_id, group, keep = arg.window_batch(sim, win, starts_dev, args.horizon, actions, species, worlds)

        def torch_update():
            total = torch.zeros(G, device=dev).index_add_(0, group, keep.sum(dim=0)).clamp_(min=1.0)
            order, seg = mb.sequence_segments(net_id, G)
            logp, value, entropy = mb.evaluate_sequences_groups(nets, b["obs"], action, b["len"], b["hidden0"], order,
                                                                seg)
            per = arg.per_element(logp, value, entropy, b["adv"], b["ret"], value_coef, entropy_coef)
            per = per * (keep * (1.0 / total)[group][None, :])
            per_group = torch.zeros(G, device=dev).index_add_(0, group, per.detach().sum(dim=0))
            for opts in per_module:
                for opt in opts:
                    opt.zero_grad(set_to_none=True)
            per.sum().backward()
            for opts in per_module:
                for opt in opts:
                    opt.step()
            return per_group.cpu()

        def device_update():
            return arg.device_update_step(mb, nets, clipped, b, action, net_id, args.horizon - 1, value_coef,
                                          entropy_coef).cpu()
        c = contest({"grouped_evaluate": torch_update, "device_update_clipped": device_update}, 1)
        c.update({"worlds": args.worlds, "sequences": int(b["len"].shape[0]), "L": int(b["rows"].shape[0])})
        res["c_whole_update"] = c
        win.close()
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
