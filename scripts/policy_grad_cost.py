#!/usr/bin/env python3
"""What PolicyNet.evaluate + backward() costs on one GPU (include/mbots.h
"Learning from what the actor did"), in the manner of scripts/policy_cost.py:
--worlds worlds (65536) a few steps into bench.py's headline run,
reference-sized nets (H = 128, a trunk of three Linear layers with codes 0, 3,
1, the actor and critic heads) with different random weights per species, every
row of the table evaluated through its species' net on act()'s actions.

  a. with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1
     --steps 100 --warmup 20 of that tree and of this one, alternating, each in a
     process of its own.  A manager that never evaluates must sit inside the
     parent's own run-to-run spread ("no_policy_within_parent_spread").
  b. evaluate() + backward() of all four species slices per call: device events
     around --calls calls, --reps repeats, alternating with
  c. torch's f32 autograd of the same nn.Sequentials on the same rows, the same
     loss (log_softmax, gather, entropy, value; sum of g * output), timed the
     same way; and the peak device memory each of the two adds over what is
     allocated before the call (torch.cuda.max_memory_allocated).

Parts that were not run say "not measured".  Writes every time and the means
to --out (JSON)."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_grad_cost.json"))
    args = ap.parse_args()
    res = {"worlds": args.worlds, "reps": args.reps, "calls": args.calls, "bench_no_policy": NOT}

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
        res["bench_no_policy"] = {
            "command": "bench.py --gpus 1 --steps 100 --warmup 20", "parent_ms_per_step": par,
            "branch_ms_per_step": br, "parent_mean_ms": statistics.mean(par), "branch_mean_ms": statistics.mean(br),
            "parent_spread_ms": spread,
            "no_policy_within_parent_spread": abs(statistics.mean(br) - statistics.mean(par)) <= spread}
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
    torch.manual_seed(0)
    models = []
    for _ in range(4):
        feature = nn.Sequential(nn.Linear(69, H), nn.Linear(H, H), nn.Tanh(), nn.Linear(H, H), nn.ReLU())
        actor = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 6))
        critic = nn.Sequential(nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 1))
        with torch.no_grad():
            feature[0].weight.mul_(0.02)   # (unnormalised inputs: bytes up to 255)
        models.append(tuple(x.to(m.device) for x in (feature, actor, critic)))
    nets = [mb.PolicyNet.from_torch(*x) for x in models]
    params = [p for x in models for mod in x for p in mod.parameters()]
    m.set_policy(nets)
    n = m.num_agents()
    counts = [int(c) for c in m.species_count_tensor().to_torch().sum(dim=0).tolist()]
    obs = m.construct_obs().clone()
    action = m.act(write=False)["action"].clone()
    g = [torch.randn(n, device=m.device) / n for _ in range(3)]
    flop_row = 2 * (72 * H + 2 * H * H + 2 * H * H + H * 6 + H * 1)
    res.update(rows=n, species_rows=counts, flop_per_row_forward=flop_row)

    def ours():
        lo = 0
        loss = 0.0
        for s, net in enumerate(nets):
            hi = lo + counts[s]
            out = net.evaluate(obs[lo:hi], action[lo:hi])
            loss = loss + sum((q[lo:hi] * o).sum() for q, o in zip(g, out))
            lo = hi
        loss.backward()

    def torch_path():
        lo = 0
        loss = 0.0
        for s, (feature, actor, critic) in enumerate(models):
            hi = lo + counts[s]
            h = feature(obs[lo:hi])
            lsm = torch.log_softmax(actor(h), dim=1)
            out = (lsm.gather(1, action[lo:hi].long())[:, 0], critic(h)[:, 0], -(lsm.exp() * lsm).sum(dim=1))
            loss = loss + sum((q[lo:hi] * o).sum() for q, o in zip(g, out))
            lo = hi
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
    res["evaluate_backward"] = {"device_ms_per_call": ev_ms, "host_ms_per_call": ev_host, "mean_device_ms": em,
                                "peak_extra_mb": peak_mb(ours),
                                "note": "the cached workspace (evaluate_workspace_mb) is allocated before the measured "
                                        "call and is not part of peak_extra_mb"}
    res["evaluate_workspace_mb"] = sum(w.numel() for w in mb._workspaces.values()) / 2 ** 20
    res["torch_autograd"] = {"device_ms_per_call": to_ms, "host_ms_per_call": to_host, "mean_device_ms": tm,
                             "peak_extra_mb": peak_mb(torch_path),
                             "note": "the same nn.Sequentials per species slice in torch f32 under autograd"}
    res["evaluate_over_torch"] = em / tm
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
