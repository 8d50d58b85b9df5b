#!/usr/bin/env python3
"""What the gated memory head costs on one GPU (DESIGN.md "Gated memory head"),
in the manner of scripts/policy_cost.py and scripts/policy_seq_cost.py, with
reference-sized recurrent nets: H = 128, a trunk of three Linear layers with
codes 0, 3, 1 over the 85 inputs, the actor and critic heads, the memory head,
memory_in -- and, gated, the gate head.  Parts (--part), each a run of its own:

  gate    in this process, --reps alternating repeats of each:
          act() at --worlds worlds (65536) a few steps into bench.py's headline
          run, gated against ungated (device events around --calls calls);
          evaluate_sequences() + backward() for --seqs sequences (65536) of
          --steps steps (16), every length full, gated against ungated
          (--seq-calls calls).
  parent  with --parent DIR (a built checkout of the parent commit): the
          ungated act() and the ungated evaluate_sequences() + backward() above,
          and bench.py --gpus 1 --steps 100 --warmup 20, of that tree and of
          this one, alternating, each run a process of its own.  Nothing
          existing may get slower: each mean must sit inside the parent's own
          run-to-run spread, |mean(branch) - mean(parent)| <= max(parent) -
          min(parent) ("within_parent_spread").
  child   (what `parent` starts) the ungated pair of --tree DIR, as one JSON line.

Parts that were not run say "not measured".  Merges every time and the means
into --out (JSON)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from policy_cost import bench_ms, NOT, H, SEED, A, ACTION_SEED   # noqa: E402


def modules(torch, dev, gated):
    """One species' nn modules (and the gate's when gated)."""
    nn = torch.nn
    feature = nn.Sequential(nn.Linear(85, H), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, H), nn.ReLU())
    actor = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 6))
    critic = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1))
    memory = nn.Sequential(nn.Linear(H, 16), nn.Tanh())
    with torch.no_grad():
        feature[0].weight[:, :69].mul_(0.02)   # (unnormalised inputs: bytes up to 255)
    mods = [feature, actor, critic, memory] + ([nn.Sequential(nn.Linear(H, 16), nn.Sigmoid())] if gated else [])
    return [x.to(dev) for x in mods]


def policy_net(mb, mods):
    kw = {"gate": mods[4]} if len(mods) > 4 else {}
    return mb.PolicyNet.from_torch(mods[0], mods[1], mods[2], mods[3], memory_in=True, **kw)


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


def measure(tree, args, kinds):
    """{"act": {kind: [ms]}, "seq": {kind: [ms]}} of the library of `tree`,
    kinds of ("ungated", "gated"), --reps alternating repeats."""
    sys.path.insert(0, os.path.join(tree, "madrona-bots_amd"))
    import torch
    import madrona_bots as mb
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "act": {k: [] for k in kinds}, "seq": {k: [] for k in kinds}}
    # ---- act() ----
    m = mb.SimManager(0, args.worlds, SEED, A)
    for t in range(4):
        m.write_synthetic_actions(ACTION_SEED, t, True)
        m.step()
        m.shift_observations()
    nets = {k: [policy_net(mb, [x.requires_grad_(False) for x in modules(torch, dev, k == "gated")]) for _ in range(4)]
            for k in kinds}
    n = m.num_agents()
    o = {k: torch.empty((n, 1), dtype=d, device=dev)
         for k, d in (("action", torch.int32), ("logp", torch.float32), ("value", torch.float32))}
    out["rows"] = n
    for _ in range(args.reps):
        for k in kinds:
            m.set_policy(nets[k])
            out["act"][k].append(device_ms(torch, lambda: m.act(out=o), args.calls))
    del m
    # ---- evaluate_sequences() + backward() ----
    L, B = args.steps, args.seqs
    obs = torch.randn(L, B, 69, device=dev).abs_().mul_(30.0)
    action = torch.randint(0, 6, (L, B), device=dev, dtype=torch.int32)
    length = torch.full((B,), L, device=dev, dtype=torch.int32)
    hidden0 = torch.rand(B, 16, device=dev) * 2 - 1
    g = [torch.randn(L, B, device=dev) / (L * B) for _ in range(3)]
    seq = {}
    for k in kinds:
        mods = modules(torch, dev, k == "gated")
        seq[k] = (policy_net(mb, mods), [p for x in mods for p in x.parameters()])

    def call(k):
        net, params = seq[k]
        for p in params:
            p.grad = None
        res = net.evaluate_sequences(obs, action, length, hidden0)
        sum((q * r).sum() for q, r in zip(g, res)).backward()
    for _ in range(args.reps):
        for k in kinds:
            out["seq"][k].append(device_ms(torch, lambda: call(k), args.seq_calls))
    return out


def spread_row(par, br):
    spread = max(par) - min(par)
    return {"parent": par, "branch": br, "parent_mean": statistics.mean(par), "branch_mean": statistics.mean(br),
            "parent_spread": spread, "within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("gate", "parent", "child"), required=True)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--seqs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--seq-calls", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part parent)")
    ap.add_argument("--tree", default=ROOT, help="(part child) the tree whose library is measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_gate_cost.json"))
    args = ap.parse_args()
    if args.part == "child":
        args.reps = 1
        print(json.dumps(measure(os.path.abspath(args.tree), args, ("ungated",))))
        return
    res = {"gated_against_ungated": NOT, "against_parent": NOT}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res.update(json.load(f))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    shape = {"worlds": args.worlds, "sequences": args.seqs, "steps": args.steps, "reps": args.reps,
             "act_calls": args.calls, "seq_calls": args.seq_calls, "H": H}
    if args.part == "gate":
        got = measure(ROOT, args, ("ungated", "gated"))
        row = dict(shape, device=got["device"], rows=got["rows"])
        for what, unit in (("act", "act_device_ms_per_call"), ("seq", "evaluate_sequences_backward_device_ms_per_call")):
            u, gt = got[what]["ungated"], got[what]["gated"]
            row[unit] = {"ungated": u, "gated": gt, "ungated_mean": statistics.mean(u), "gated_mean": statistics.mean(gt),
                         "gated_over_ungated": statistics.mean(gt) / statistics.mean(u)}
        res["gated_against_ungated"] = row
        save()
        print(json.dumps(row))
        return
    if not args.parent:
        ap.error("--part parent needs --parent")
    trees = {"parent": os.path.abspath(args.parent), "branch": ROOT}
    runs = {k: {"act": [], "seq": [], "bench": []} for k in trees}
    t0 = time.time()
    for _ in range(args.reps):
        for k, tree in trees.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--part", "child", "--tree", tree, "--worlds",
                   str(args.worlds), "--seqs", str(args.seqs), "--steps", str(args.steps), "--calls", str(args.calls),
                   "--seq-calls", str(args.seq_calls)]
            line = [ln for ln in subprocess.run(cmd, check=True, capture_output=True, text=True,
                                                timeout=600).stdout.splitlines() if ln.startswith("{")][-1]
            got = json.loads(line)
            runs[k]["act"] += got["act"]["ungated"]
            runs[k]["seq"] += got["seq"]["ungated"]
            runs[k]["bench"].append(bench_ms(tree))
            print(f"[{time.time() - t0:.0f}s] {k}: act {runs[k]['act'][-1]:.3f} ms, seq {runs[k]['seq'][-1]:.2f} ms, "
                  f"bench {runs[k]['bench'][-1]:.4f} ms/step", flush=True)
    res["against_parent"] = dict(
        shape, note="every run a process of its own, parent and branch alternating; ms",
        ungated_act_device_ms_per_call=spread_row(runs["parent"]["act"], runs["branch"]["act"]),
        ungated_evaluate_sequences_backward_device_ms_per_call=spread_row(runs["parent"]["seq"], runs["branch"]["seq"]),
        bench_no_policy_ms_per_step=dict(spread_row(runs["parent"]["bench"], runs["branch"]["bench"]),
                                         command="bench.py --gpus 1 --steps 100 --warmup 20"))
    save()
    print(json.dumps(res["against_parent"]))


if __name__ == "__main__":
    main()
