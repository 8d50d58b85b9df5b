#!/usr/bin/env python3
"""What acting on the device costs on one GPU (include/mbots.h "Acting on the
device"), in the manner of scripts/seq_cost.py: --worlds worlds (65536) a few
steps into bench.py's headline run, reference-sized nets (H = 128, a trunk of
three Linear layers with codes 0, 3, 1, the actor and critic heads) with
different random weights per species.

  a. with --parent DIR (a built checkout of the parent commit): bench.py --gpus 1
     --steps 100 --warmup 20 of that tree and of this one, alternating, each in a
     process of its own.  A manager without a policy must sit inside the parent's
     own run-to-run spread: |mean(branch) - mean(parent)| <= max(parent) -
     min(parent) ("no_policy_within_parent_spread").
  b. act() per call: device events around --calls calls on the same table
     (write=True: the full call), --reps repeats.
  c. the torch path doing the same work per call -- construct_obs(), the same
     nets per species slice in torch f32, Categorical.sample(), log_prob, the
     one-hot and write_actions() -- timed the same way, plus its host wall time.

The FLOP count is arithmetic from the shapes.  Parts that were not run say "not
measured".  Writes every time and the means to --out (JSON)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, A, ACTION_SEED = 69, 32, 1234   # bench.py's
NOT = "not measured"
H = 128


def bench_ms(tree):
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "100",
                          "--warmup", "20"], cwd=tree, check=True, capture_output=True, text=True, timeout=600).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part a)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "policy_cost.json"))
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
        models.append(tuple(x.to(m.device).requires_grad_(False) for x in (feature, actor, critic)))
    m.set_policy([mb.PolicyNet.from_torch(*x) for x in models])
    n = m.num_agents()
    counts = m.species_count_tensor().to_torch().sum(dim=0).tolist()
    flop_row = 2 * (72 * H + 2 * H * H + 2 * H * H + H * 6 + H * 1)
    res.update(rows=n, species_rows=counts, flop_per_row=flop_row, flop_per_call=flop_row * n)
    out = {k: torch.empty((n, 1), dtype=d, device=m.device)
           for k, d in (("action", torch.int32), ("logp", torch.float32), ("value", torch.float32))}

    def device_ms(fn):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        host = (time.perf_counter() - h0) * 1e3 / args.calls
        b.synchronize()
        return a.elapsed_time(b) / args.calls, host

    onehot = torch.zeros((n, 6), dtype=torch.int32, device=m.device)

    @torch.no_grad()
    def torch_path():
        obs = m.construct_obs()
        lo = 0
        for s, (feature, actor, critic) in enumerate(models):
            hi = lo + int(counts[s])
            h = feature(obs[lo:hi])
            dist = torch.distributions.Categorical(logits=actor(h))
            a = dist.sample()
            out["logp"][lo:hi, 0] = dist.log_prob(a)
            out["value"][lo:hi] = critic(h)
            out["action"][lo:hi, 0] = a.to(torch.int32)
            lo = hi
        onehot.zero_()
        onehot.scatter_(1, out["action"].long(), 1)
        m.write_actions(onehot)

    act_ms, act_host, torch_ms, torch_host = [], [], [], []
    for _ in range(args.reps):
        d, h = device_ms(lambda: m.act(out=out))
        act_ms.append(d)
        act_host.append(h)
        d, h = device_ms(torch_path)
        torch_ms.append(d)
        torch_host.append(h)
    am, tm = statistics.mean(act_ms), statistics.mean(torch_ms)
    res["act"] = {"device_ms_per_call": act_ms, "host_ms_per_call": act_host, "mean_device_ms": am,
                  "tflops": flop_row * n / (am * 1e-3) / 1e12}
    res["torch_path"] = {"device_ms_per_call": torch_ms, "host_ms_per_call": torch_host, "mean_device_ms": tm,
                         "note": "construct_obs + the same nets per species slice in torch f32 + Categorical.sample "
                                 "+ log_prob + one-hot + write_actions"}
    res["torch_over_act"] = tm / am
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
