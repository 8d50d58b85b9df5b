"""G independent PPO learners on one manager, the whole update in the library
(DESIGN.md "PPO on the device"; INTEGRATION.md "PPO") -- beside a2c_groups.py,
whose rollout it repeats and whose nets it builds on:

    act() -> window.push(value) -> step() ... -> window.compute()      (keeping act()'s logp and value)
    policy_group_rows, advantage_moments_groups                          once per update
    per epoch:  PolicyAdam.zero_grad();
                per table: evaluate_groups -> ppo_loss_groups -> autograd.backward;
                ppo_kl_gate; PolicyAdam.step(gate)
    set_policy(group=u)

The importance ratio is formed from the very bits act() returned; the sums run
in an order that is a property of the row indices, so CPU mode and HIP mode end
with the same parameter bits; a group whose KL estimate passes --target-kl stops
for the rest of the update without the host reading anything, and statistics
and row counts are read once, after the last epoch.  One group is the plain
case.  Every epoch passes over all rows: minibatches inside an epoch need an
indexed evaluate_groups.

    python madrona-bots_amd/harness/ppo_groups.py --worlds 64 --groups 1 --iters 5 --exec-mode cpu
    python madrona-bots_amd/harness/ppo_groups.py --worlds 65536 --groups 32 --iters 20 --target-kl 0.02
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from a2c import make_modules  # noqa: E402

STATS = ("loss", "policy", "value", "entropy", "kl", "clipped")


def train(sim, starts, modules, iters, horizon=8, gamma=0.99, lam=0.95, death_reward=-1.0, epochs=4, clip=0.2,
          value_clip=None, target_kl=None, adv_norm=True, value_coef=0.5, entropy_coef=0.01, lr=3e-4,
          max_grad_norm=None, weight_decay=0.0, log=None):
    """`iters` updates of `horizon - 1` steps and `epochs` epochs each of every
    group.  modules[u]: a2c.make_modules' four ModuleDicts of group u.  Returns
    per update {"stats": [epochs][G][6] floats (STATS), "rows": [G], "steps":
    [G] steps the groups' optimisers have taken}."""
    import madrona_bots as mb
    G = len(starts)
    sim.set_policy_groups(starts)
    nets = [[mb.PolicyNet.from_torch(m["feature"], m["actor"], m["critic"]) for m in modules[u]] for u in range(G)]
    for u in range(G):
        sim.set_policy(nets[u], group=u)
    adam = mb.PolicyAdam(nets, lr=lr, max_grad_norm=max_grad_norm, weight_decay=weight_decay)
    win = sim.trajectory_window(horizon, max_rows=sim.num_worlds * sim.agent_capacity)
    seg = torch.empty((G, 4, 2), dtype=torch.int32, device=sim.device)
    out_log = []
    try:
        for it in range(iters):
            rows = []                                   # per table: (obs, action, old logp, old value, segments)
            for t in range(horizon):
                last = t == horizon - 1                 # the last table only bootstraps
                obs = None if last else sim.construct_obs().clone()
                o = sim.act(write=not last)
                win.push(o["value"])
                if not last:
                    rows.append((obs, o["action"], o["logp"], o["value"], sim.policy_segments(out=seg).clone()))
                    sim.step()
            out = win.compute(gamma=gamma, lam=lam, death_reward=death_reward)
            rec = ppo_update(mb, nets, adam, rows, out, epochs, clip, value_clip, target_kl, adv_norm, value_coef,
                             entropy_coef)
            for u in range(G):
                sim.set_policy(nets[u], group=u)
            win.clear()
            out_log.append(rec)
            if log:
                log(json.dumps(dict(rec, iter=it)))
    finally:
        win.close()
    return out_log


def ppo_update(mb, nets, adam, rows, out, epochs, clip, value_clip, target_kl, adv_norm, value_coef, entropy_coef):
    """One PPO update of every group from the recorded tables `rows` -- (obs,
    action, act()'s logp, act()'s value, segments [G, 4, 2] on the device) --
    and the window's `out`.  The row totals and the advantage moments are taken
    once; every epoch is zero_grad, per table evaluate_groups, ppo_loss_groups
    into the epoch's slice of the statistics and one autograd.backward, then the
    KL gate and one PolicyAdam.step(gate).  The device is read once, after the
    last epoch."""
    G = len(nets)
    dev = rows[0][0].device
    total = torch.zeros(G, dtype=torch.int64, device=dev)
    moments = torch.zeros((G, 3), dtype=torch.float64, device=dev) if adv_norm else None
    for t, (_, _, _, _, sg) in enumerate(rows):
        mb.policy_group_rows(sg, total)
        if adv_norm:
            mb.advantage_moments_groups(out["adv"][t], out["end"][t], sg, moments=moments)
    stats = torch.zeros((epochs, G, 6), dtype=torch.float64, device=dev)
    gate = total.clone()
    for e in range(epochs):
        adam.zero_grad()
        for t, (obs, action, old_logp, old_value, sg) in enumerate(rows):
            outs = mb.evaluate_groups(nets, obs, action, sg)
            g = mb.ppo_loss_groups(*outs, old_logp, old_value, out["adv"][t], out["ret"][t], out["end"][t], sg, total,
                                   clip=clip, value_clip=value_clip, value_coef=value_coef, entropy_coef=entropy_coef,
                                   moments=moments, stats=stats[e])
            torch.autograd.backward(list(outs), list(g[:3]))
        if target_kl is not None:
            mb.ppo_kl_gate(stats[e], total, target_kl, gate)
        adam.step(gate)
    host = torch.cat([stats.reshape(-1), total.to(torch.float64), adam.steps.to(torch.float64)]).cpu()
    n = epochs * G * 6
    return {"stats": host[:n].reshape(epochs, G, 6).tolist(), "rows": [int(x) for x in host[n:n + G]],
            "steps": [int(x) for x in host[n + G:]]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--groups", type=int, default=1)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 64],
                    help="trunk widths, cycled over the groups (universes differ in architecture)")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=69)
    ap.add_argument("--exec-mode", choices=("hip", "cpu"), default="hip" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--reward-fixed", action="store_true", help="rewards[speciesID - 1]: universes fully apart")
    ap.add_argument("--epochs", type=int, default=4, help="passes over the rollout per update")
    ap.add_argument("--clip", type=float, default=0.2, help="the surrogate's clip range, in (0, 1)")
    ap.add_argument("--value-clip", type=float, default=None, help="clip the value loss around act()'s value")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="a group stops for the rest of an update once its KL estimate passes this")
    ap.add_argument("--no-adv-norm", action="store_true", help="raw advantages instead of per-group normalised ones")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip every group's global gradient norm")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="decoupled weight decay")
    args = ap.parse_args()
    if not 1 <= args.groups <= 64 or args.worlds < args.groups:
        ap.error("--groups must be in [1, 64] and at most --worlds")
    if args.epochs < 1:
        ap.error("--epochs must be at least 1")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import madrona_bots as mb
    sim = mb.SimManager(0, args.worlds, args.seed, args.agents, exec_mode=args.exec_mode,
                        reward_fixed=args.reward_fixed)
    starts = [u * args.worlds // args.groups for u in range(args.groups)]
    modules = [make_modules(args.hidden[u % len(args.hidden)], sim.device, args.seed + u) for u in range(args.groups)]
    train(sim, starts, modules, args.iters, args.horizon, epochs=args.epochs, clip=args.clip,
          value_clip=args.value_clip, target_kl=args.target_kl, adv_norm=not args.no_adv_norm, lr=args.lr,
          max_grad_norm=args.max_grad_norm, weight_decay=args.weight_decay, log=print)


if __name__ == "__main__":
    main()
