#!/usr/bin/env python3
"""What PPO on the device costs on one GPU (include/mbots.h "PPO on the
device"; DESIGN.md "PPO on the device"), in the manner of
scripts/policy_seq_update_cost.py.

  build. --build-variants: compile the library once more per other candidate of
     the two chunk sizes (MBOTS_PPO_CHUNK, MBOTS_PPO_SEQ_CHUNK) into
     build_var/ppo_<rows>_<positions>/madrona_bots, a copy of the package
     beside it.  No GPU needed; the measurement below then finds them.
  a. the loss: advantage moments + PPO loss of --rows rows (2.15 M) and of
     --seqs sequences (65536) of L = --steps (16), with --groups groups (32)
     and with one, against a2c_loss_groups / a2c_loss_sequences at the same
     shapes (the parent commit's kernels, unchanged here) and against a torch
     composition of the same PPO loss with autograd back to the three outputs;
     and the library's two calls with every chunk candidate that was built
     (this script's --variant mode in a child process).
  b. a whole update: --epochs (4) epochs of evaluate_groups, ppo_loss_groups,
     backward, ppo_kl_gate and PolicyAdam.step over --update-rows rows of
     --groups groups of reference-sized nets, eagerly and as one graph replay.
  c. with --parent DIR (a built checkout of the parent commit): bench.py
     --gpus 1 --steps 100 --warmup 20 of that tree and of this one,
     alternating, each in a process of its own.

Per call: wall ms (until the device is idle), device ms (events around the
calls) and host ms (until the last launch is enqueued); --reps alternating
runs per contender in one process, mean and max - min spread.  Writes to
--out (JSON)."""
import argparse
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128
CANDIDATES = ((2048, 256), (4096, 512), (8192, 1024))     # (rows, column positions) of a chunk; the middle one is built in
HYPER = dict(clip=0.2, value_clip=0.5, value_coef=0.5, entropy_coef=0.01)


def build_variants():
    for rows, pos in (CANDIDATES[0], CANDIDATES[2]):
        d = os.path.join(ROOT, "build_var", f"ppo_{rows}_{pos}", "madrona_bots")
        os.makedirs(d, exist_ok=True)
        for f in glob.glob(os.path.join(ROOT, "madrona-bots_amd", "madrona_bots", "*.py")):
            shutil.copy(f, d)
        subprocess.run(["make", "-B", "-C", os.path.join(ROOT, "madrona-bots_amd", "csrc"),
                        "OUT=" + os.path.join(d, "libmbots.so"),
                        f"EXTRA=-DMBOTS_PPO_CHUNK={rows} -DMBOTS_PPO_SEQ_CHUNK={pos}"], check=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--rows", type=int, default=2150000)
    ap.add_argument("--seqs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--update-rows", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part c)")
    ap.add_argument("--build-variants", action="store_true", help="build the chunk candidates and exit")
    ap.add_argument("--variant", default=None, metavar="DIR",
                    help="(child mode) time the library's calls of part a with the package in DIR; print JSON")
    ap.add_argument("--skip", default="", help="parts to leave out, of a, b, c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_ppo_cost.json"))
    args = ap.parse_args()
    if args.build_variants:
        build_variants()
        return
    G = args.groups
    res = {"groups": G, "reps": args.reps, "calls": args.calls}
    if os.path.exists(args.out) and not args.variant:
        with open(args.out) as f:                # parts measured in an earlier run stay
            res = dict(json.load(f), **res)

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
                         "device_spread_ms": max(device) - min(device)}
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

    if args.parent and "c" not in args.skip and not args.variant:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        from policy_cost import bench_ms
        par, br = [], []
        for _ in range(args.reps):
            par.append(bench_ms(os.path.abspath(args.parent)))
            br.append(bench_ms(ROOT))
            print(f"bench: parent {par[-1]:.4f} ms, branch {br[-1]:.4f} ms per step", file=sys.stderr, flush=True)
        spread = max(par) - min(par)
        res["c_bench_unused"] = {
            "command": "bench.py --gpus 1 --steps 100 --warmup 20", "parent_ms_per_step": par,
            "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par), "branch_mean_ms": statistics.mean(br),
            "parent_spread_ms": spread,
            "within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}
        save()

    pkg = os.path.abspath(args.variant) if args.variant else os.path.join(ROOT, "madrona-bots_amd")
    sys.path.insert(0, pkg)
    sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd", "harness"))
    import torch                     # (after the benchmark's child processes: they start from a process without a GPU)
    import madrona_bots as mb
    if not torch.cuda.is_available():
        raise SystemExit("policy_ppo_cost.py measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    res["device"] = torch.cuda.get_device_name(0)

    # ---- a. moments + loss ----
    def rows_case(Gb):
        n = args.rows
        torch.manual_seed(2)
        cols = [torch.randn(n, device=dev) for _ in range(7)]     # logp, value, entropy, old_logp, old_value, adv, ret
        cols[3] = cols[0] + 0.2 * cols[3]
        cols[4] = cols[1] + 0.5 * cols[4]
        end = torch.randint(0, 4, (n,), dtype=torch.int32, device=dev)
        edges = torch.linspace(0, n, 4 * Gb + 1).to(torch.int32)
        seg = torch.stack([edges[:-1], edges[1:]], dim=1).reshape(Gb, 4, 2).contiguous().to(dev)
        rows = mb.policy_group_rows(seg, torch.zeros(Gb, dtype=torch.int64, device=dev))
        group = torch.bucketize(torch.arange(n, device=dev), edges[4::4].to(dev), right=True).clamp_(max=Gb - 1)
        return cols, end, seg, rows, group

    def torch_ppo(cols, keep, weight, group, Gb):
        """The same PPO loss composed of torch operations: normalisation per
        group, both clamps, the six statistics, and autograd back to the
        three outputs."""
        logp, value, entropy = (c.detach().requires_grad_() for c in cols[:3])
        old_logp, old_value, adv, ret = cols[3:]
        cnt = torch.zeros(Gb, device=dev).index_add_(0, group, keep)
        s1 = torch.zeros(Gb, device=dev).index_add_(0, group, keep * adv)
        s2 = torch.zeros(Gb, device=dev).index_add_(0, group, keep * adv * adv)
        mean = s1 / cnt.clamp(min=1.0)
        std = ((s2 - s1 * mean) / (cnt - 1.0).clamp(min=1.0)).clamp(min=0.0).sqrt()
        A = (adv - mean[group]) / (std[group] + 1e-8)
        lr = logp - old_logp
        ratio = torch.exp(lr)
        pol = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - HYPER["clip"], 1.0 + HYPER["clip"]) * A)
        vc = old_value + torch.clamp(value - old_value, -HYPER["value_clip"], HYPER["value_clip"])
        vl = torch.max((value - ret) ** 2, (vc - ret) ** 2)
        w = keep * weight
        per = (pol + HYPER["value_coef"] * vl - HYPER["entropy_coef"] * entropy) * w
        with torch.no_grad():
            parts = torch.stack([per, pol * w, vl * w, entropy * w, ((ratio - 1.0) - lr) * w,
                                 ((ratio - 1.0).abs() > HYPER["clip"]).to(torch.float32) * w], dim=-1)
            stats = torch.zeros(Gb, 6, device=dev).index_add_(0, group.reshape(-1), parts.reshape(-1, 6))
        return torch.autograd.grad(per.sum(), [logp, value, entropy]), stats

    def part_a(library_only):
        out = {"rows": args.rows, "sequences": args.seqs, "L": args.steps}
        for Gb in (1, G):
            cols, end, seg, rows, group = rows_case(Gb)
            keep = (end != 2).to(torch.float32)
            weight = (1.0 / rows.to(torch.float32))[group]

            def ppo():
                m = mb.advantage_moments_groups(cols[5], end, seg)
                return mb.ppo_loss_groups(*cols, end, seg, rows, moments=m, **HYPER)

            def ppo_loss_only():
                return mb.ppo_loss_groups(*cols, end, seg, rows, **HYPER)
            contenders = {"moments_and_ppo_loss": ppo, "ppo_loss_alone": ppo_loss_only}
            if not library_only:
                contenders["a2c_loss_groups"] = lambda: mb.a2c_loss_groups(cols[0], cols[1], cols[2], cols[5], cols[6],
                                                                           end, seg, rows, 0.5, 0.01)
                contenders["torch_composition"] = lambda: torch_ppo(cols, keep, weight, group, Gb)
                contenders["moments_and_ppo_loss_graph_replay"] = replay_of(ppo).replay
            out[f"rows_groups_{Gb}"] = contest(contenders, args.calls)
            del cols, end, group, keep, weight
        L, B = args.steps, args.seqs
        for Gb in (1, G):
            torch.manual_seed(3)
            cols = [torch.randn(L, B, device=dev) for _ in range(7)]
            cols[3] = cols[0] + 0.2 * cols[3]
            cols[4] = cols[1] + 0.5 * cols[4]
            length = torch.randint(0, L + 1, (B,), dtype=torch.int32, device=dev)
            t0 = torch.randint(0, 4, (B,), dtype=torch.int32, device=dev)
            end = torch.randint(0, 4, (B,), dtype=torch.int32, device=dev)
            group = torch.randint(0, Gb, (B,), device=dev)
            net_id = (group * 4 + torch.randint(0, 4, (B,), device=dev)).to(torch.int32)
            order, seg = mb.sequence_segments(net_id, Gb)
            rows = mb.sequence_group_rows(length, t0, end, order, seg, torch.zeros(Gb, dtype=torch.int64, device=dev), L)
            k = torch.arange(L, device=dev, dtype=torch.int32)[:, None]
            keep = ((k < length[None, :]) & (t0[None, :] + k < L) &
                    ~((end == 2)[None, :] & (k == length[None, :] - 1))).to(torch.float32)
            weight = (1.0 / rows.clamp(min=1).to(torch.float32))[group][None, :].expand(L, B)
            gg = group[None, :].expand(L, B)

            def ppo_seq():
                m = mb.advantage_moments_sequences(cols[5], length, t0, end, order, seg, L)
                return mb.ppo_loss_sequences(*cols, length, t0, end, order, seg, rows, L, moments=m, **HYPER)
            contenders = {"moments_and_ppo_loss": ppo_seq}
            if not library_only:
                contenders["a2c_loss_sequences"] = lambda: mb.a2c_loss_sequences(
                    cols[0], cols[1], cols[2], cols[5], cols[6], length, t0, end, order, seg, rows, L, 0.5, 0.01)
                contenders["torch_composition"] = lambda: torch_ppo([c.reshape(-1) for c in cols], keep.reshape(-1),
                                                                    weight.reshape(-1), gg.reshape(-1), Gb)
                contenders["moments_and_ppo_loss_graph_replay"] = replay_of(ppo_seq).replay
            out[f"sequences_groups_{Gb}"] = contest(contenders, args.calls)
            del cols
        return out

    if args.variant:
        print(json.dumps(part_a(True)))
        return
    if "a" not in args.skip:
        res["a_loss"] = part_a(False)
        res["a_loss"]["chunk_built_in"] = list(CANDIDATES[1])
        save()
        res["a_loss"]["chunk_candidates"] = {}
        for rows, pos in CANDIDATES:
            d = os.path.join(ROOT, "build_var", f"ppo_{rows}_{pos}")
            if not os.path.exists(os.path.join(d, "madrona_bots", "libmbots.so")):
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", d, "--groups", str(G), "--rows", str(args.rows),
                   "--seqs", str(args.seqs), "--steps", str(args.steps), "--reps", str(args.reps), "--calls",
                   str(args.calls)]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                res["a_loss"]["chunk_candidates"][f"{rows}_{pos}"] = "not measured: " + out.stderr.strip()[-300:]
                continue
            full = json.loads(out.stdout.strip().splitlines()[-1])
            res["a_loss"]["chunk_candidates"][f"{rows}_{pos}"] = {
                case: {name: {k: v[k] for k in ("mean_device_ms", "device_spread_ms")} for name, v in per.items()}
                for case, per in full.items() if isinstance(per, dict)}
            save()

    # ---- b. a whole multi-epoch update ----
    if "b" not in args.skip:
        import a2c
        n, E = args.update_rows, args.epochs
        modules = [a2c.make_modules(H, dev, seed=u) for u in range(G)]
        nets = [[mb.PolicyNet.from_torch(m["feature"], m["actor"], m["critic"]) for m in four] for four in modules]
        adam = mb.PolicyAdam(nets, lr=3e-4, max_grad_norm=0.5)
        torch.manual_seed(4)
        obs = torch.rand(n, 69, device=dev) * 3.0
        action = torch.randint(0, 6, (n,), dtype=torch.int32, device=dev)
        adv, ret = torch.randn(n, device=dev), torch.randn(n, device=dev)
        end = torch.randint(0, 4, (n,), dtype=torch.int32, device=dev)
        edges = torch.linspace(0, n, 4 * G + 1).to(torch.int32)
        seg = torch.stack([edges[:-1], edges[1:]], dim=1).reshape(G, 4, 2).contiguous().to(dev)
        rows = mb.policy_group_rows(seg, torch.zeros(G, dtype=torch.int64, device=dev))
        first = [x.detach().clone() for x in mb.evaluate_groups(nets, obs, action, seg)]
        moments = mb.advantage_moments_groups(adv, end, seg)
        stats = torch.zeros(E, G, 6, dtype=torch.float64, device=dev)
        gate = rows.clone()

        def update():
            stats.zero_()
            gate.copy_(rows)
            for e in range(E):
                adam.zero_grad()
                outs = mb.evaluate_groups(nets, obs, action, seg)
                g = mb.ppo_loss_groups(*outs, first[0], first[1], adv, ret, end, seg, rows, moments=moments,
                                       stats=stats[e], **HYPER)
                torch.autograd.backward(list(outs), list(g[:3]))
                mb.ppo_kl_gate(stats[e], rows, 1e9, gate)
                adam.step(gate)
        b = contest({"eager": update, "graph_replay": replay_of(update).replay}, max(args.calls // 3, 2))
        b.update({"rows": n, "epochs": E, "nets": 4 * G, "hidden": H})
        res["b_whole_update"] = b
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
