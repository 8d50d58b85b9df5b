#!/usr/bin/env python3
"""What PolicyNet.evaluate_sequences + backward() costs on one GPU
(include/mbots.h "Training the memory head"), in the manner of
scripts/policy_grad_cost.py.  Two parts, each a run of its own (--part):

  bench  with --parent DIR (a built checkout of the parent commit): bench.py
         --gpus 1 --steps 100 --warmup 20 of that tree and of this one,
         alternating, each in a process of its own.  A manager that never calls
         the new code must sit inside the parent's own run-to-run spread
         ("no_policy_within_parent_spread").
  call   one species' batch of the headline shape -- B = --seqs sequences
         (65536) of L = --steps steps (16), every length L, observation-like
         random rows -- through a reference-sized recurrent net (H = 128, a
         trunk of three Linear layers with codes 0, 3, 1 over the 85 inputs,
         the actor and critic heads, the memory head): evaluate_sequences() +
         backward(), device events around --calls calls, --reps repeats,
         alternating with torch's f32 autograd doing the same backpropagation
         through time with the same nn modules in a Python loop over the steps
         (log_softmax, gather, entropy, value; sum of g * output); the host
         time of each; and the peak device memory each adds over what is
         allocated before the call (torch.cuda.max_memory_allocated).

Parts that were not run say "not measured".  Merges every time and the means
into --out (JSON)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from policy_cost import bench_ms, NOT, H   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--part", choices=("bench", "call"), required=True)
    ap.add_argument("--seqs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part bench)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_seq_cost.json"))
    args = ap.parse_args()
    res = {"bench_no_policy": NOT, "evaluate_sequences_backward": NOT, "torch_autograd": NOT}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res.update(json.load(f))

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    if args.part == "bench":
        if not args.parent:
            ap.error("--part bench needs --parent")
        par, br = [], []
        for _ in range(args.reps):
            par.append(bench_ms(os.path.abspath(args.parent)))
            br.append(bench_ms(ROOT))
        spread = max(par) - min(par)
        res["bench_no_policy"] = {
            "command": "bench.py --gpus 1 --steps 100 --warmup 20", "parent_ms_per_step": par,
            "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par), "branch_mean_ms": statistics.mean(br),
            "parent_spread_ms": spread,
            "no_policy_within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}
        save()
        print(json.dumps(res["bench_no_policy"]))
        return

    sys.path.insert(0, os.path.join(ROOT, "madrona-bots_amd"))
    import torch
    import madrona_bots as mb
    nn = torch.nn
    dev = torch.device("cuda", 0)
    L, B = args.steps, args.seqs
    torch.manual_seed(0)
    feature = nn.Sequential(nn.Linear(85, H), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, H), nn.ReLU())
    actor = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 6))
    critic = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1))
    memory = nn.Sequential(nn.Linear(H, 16), nn.Tanh())
    with torch.no_grad():
        feature[0].weight[:, :69].mul_(0.02)   # (unnormalised inputs: bytes up to 255)
    mods = [x.to(dev) for x in (feature, actor, critic, memory)]
    feature, actor, critic, memory = mods
    net = mb.PolicyNet.from_torch(feature, actor, critic, memory, memory_in=True)
    params = [p for x in mods for p in x.parameters()]
    obs = torch.randn(L, B, 69, device=dev).abs_().mul_(30.0)
    action = torch.randint(0, 6, (L, B), device=dev, dtype=torch.int32)
    length = torch.full((B,), L, device=dev, dtype=torch.int32)
    hidden0 = torch.rand(B, 16, device=dev) * 2 - 1
    g = [torch.randn(L, B, device=dev) / (L * B) for _ in range(3)]
    flop_row = 2 * (88 * H + 2 * H * H + 2 * H * H + H * 6 + H * 1 + H * 16)
    res.update(device=torch.cuda.get_device_name(0), sequences=B, steps=L, reps=args.reps, calls=args.calls,
               elements=L * B, flop_per_element_forward=flop_row)

    def ours():
        out = net.evaluate_sequences(obs, action, length, hidden0)
        sum((q * o).sum() for q, o in zip(g, out)).backward()

    def torch_path():
        h = hidden0
        loss = 0.0
        for k in range(L):
            t = feature(torch.cat([obs[k], h], dim=1))
            lsm = torch.log_softmax(actor(t), dim=1)
            out = (lsm.gather(1, action[k].long()[:, None])[:, 0], critic(t)[:, 0], -(lsm.exp() * lsm).sum(dim=1))
            loss = loss + sum((q[k] * o).sum() for q, o in zip(g, out))
            h = memory(t)
        loss.backward()

    def run(fn):
        for p in params:
            p.grad = None
        fn()

    def device_ms(fn):
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
        return a.elapsed_time(b) / args.calls, host

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

    ev_ms, ev_host, to_ms, to_host = [], [], [], []
    for _ in range(args.reps):
        d, h = device_ms(ours)
        ev_ms.append(d)
        ev_host.append(h)
        d, h = device_ms(torch_path)
        to_ms.append(d)
        to_host.append(h)
    em, tm = statistics.mean(ev_ms), statistics.mean(to_ms)
    res["evaluate_sequences_backward"] = {
        "device_ms_per_call": ev_ms, "host_ms_per_call": ev_host, "mean_device_ms": em, "peak_extra_mb": peak_mb(ours),
        "tflops_two_forwards_one_backward": (2 + 2) * flop_row * L * B / (em * 1e-3) / 1e12,
        "note": "the cached workspace (workspace_mb) is allocated before the measured call and is not part of "
                "peak_extra_mb; the rate counts two forwards and a backward of two products per element"}
    res["workspace_mb"] = sum(w.numel() for w in mb._workspaces.values()) / 2 ** 20
    res["torch_autograd"] = {"device_ms_per_call": to_ms, "host_ms_per_call": to_host, "mean_device_ms": tm,
                             "peak_extra_mb": peak_mb(torch_path),
                             "note": "the same nn modules in torch f32 under autograd, a Python loop over the steps"}
    res["evaluate_sequences_over_torch"] = em / tm
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
