"""G independent recurrent PPO learners on one manager, the whole update in the
library (DESIGN.md "PPO on the device"; INTEGRATION.md "PPO") -- ppo_groups.py
for nets with a memory head, over the trajectory window's padded [L, B]
sequence batches, beside a2c_recurrent_groups.py, whose pieces it builds on:

    push() -> act() -> step() ... -> window.compute()                  (keeping act()'s logp tables)
    sequences(), batch(), gather(actions), gather(logp tables)           the batch's "value" is act()'s
    sequence_segments, sequence_group_rows, advantage_moments_sequences  once per update
    per epoch:  PolicyAdam.zero_grad(); evaluate_sequences_groups -> ppo_loss_sequences ->
                autograd.backward; ppo_kl_gate; PolicyAdam.step(gate)
    set_policy(group=u)

Nothing in an update waits for the host but the one read of the statistics
after the last epoch; CPU mode and HIP mode end with the same parameter bits.

    python madrona-bots_amd/harness/ppo_recurrent_groups.py --worlds 64 --groups 1 --iters 5 --exec-mode cpu
    python madrona-bots_amd/harness/ppo_recurrent_groups.py --worlds 65536 --groups 32 --iters 20 --target-kl 0.02
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from a2c_recurrent import make_modules, policy_net, species_of_rows  # noqa: E402
from a2c_recurrent_groups import window_columns  # noqa: E402


def make_groups(hidden, device, seed, gated=False):
    """a2c_recurrent.make_modules per group: widths `hidden`, seeds from `seed`."""
    return [make_modules(H, device, seed + i, gated) for i, H in enumerate(hidden)]


def rollout(sim, win, horizon, gamma=0.99, lam=0.95, death_reward=-1.0):
    """a2c_recurrent.rollout, keeping act()'s log-probabilities as well: returns
    (compute()'s views, and per table in its row order: action, logp, species)."""
    actions, logps, values, species = [], [], [], []
    for t in range(horizon):
        last = t == horizon - 1                 # the last table only bootstraps
        win.push()
        o = sim.act(write=not last)
        actions.append(o["action"])
        logps.append(o["logp"])
        values.append(o["value"])
        species.append(species_of_rows(sim))
        if not last:
            sim.step()
    out = win.compute(gamma=gamma, lam=lam, death_reward=death_reward)
    for dst, v in zip(out["value"], values):
        dst.copy_(v)
    out = win.compute(gamma=gamma, lam=lam, death_reward=death_reward)
    return out, actions, logps, species


def train(sim, starts, modules, iters, horizon=8, gamma=0.99, lam=0.95, death_reward=-1.0, epochs=4, clip=0.2,
          value_clip=None, target_kl=None, adv_norm=True, value_coef=0.5, entropy_coef=0.01, lr=3e-4,
          max_grad_norm=None, weight_decay=0.0, log=None):
    """`iters` updates of `horizon - 1` steps and `epochs` epochs each of every
    group.  modules[u]: a2c_recurrent.make_modules' four ModuleDicts of group
    u.  Returns per update {"stats": [epochs][G][6], "rows": [G], "steps": [G]}."""
    import madrona_bots as mb
    G = len(starts)
    sim.set_policy_groups(starts)
    nets = [[policy_net(m) for m in modules[u]] for u in range(G)]
    for u in range(G):
        sim.set_policy(nets[u], group=u)
    adam = mb.PolicyAdam(nets, lr=lr, max_grad_norm=max_grad_norm, weight_decay=weight_decay)
    starts_dev = torch.tensor(list(starts), dtype=torch.int64, device=sim.device)
    win = sim.trajectory_window(horizon, max_rows=sim.num_worlds * sim.agent_capacity, record_obs=True,
                                record_state=True)
    out_log = []
    try:
        for it in range(iters):
            out, actions, logps, species = rollout(sim, win, horizon, gamma, lam, death_reward)
            b, action, net_id, _ = window_columns(sim, win, starts_dev, actions, species,
                                                  [w.to(torch.int32) for w in out["world"]])
            old_logp = win.gather(logps)[:, :, 0].contiguous()
            old_value = win.batch(keys=("value",))["value"]
            rec = ppo_update(mb, nets, adam, b, action, net_id, old_logp, old_value, horizon - 1, epochs, clip,
                             value_clip, target_kl, adv_norm, value_coef, entropy_coef)
            for u in range(G):
                sim.set_policy(nets[u], group=u)
            win.clear()
            out_log.append(rec)
            if log:
                log(json.dumps(dict(rec, iter=it)))
    finally:
        win.close()
    return out_log


def ppo_update(mb, nets, adam, b, action, net_id, old_logp, old_value, last_table, epochs, clip, value_clip, target_kl,
               adv_norm, value_coef, entropy_coef):
    """One PPO update of every group over the window's batch `b`: the segments,
    the groups' kept elements and the advantage moments once; per epoch
    zero_grad, evaluate_sequences_groups, ppo_loss_sequences into the epoch's
    slice of the statistics, autograd.backward, the KL gate and one
    PolicyAdam.step(gate).  The device is read once, after the last epoch."""
    G = len(nets)
    dev = net_id.device
    order, seg = mb.sequence_segments(net_id, G)
    total = torch.zeros(G, dtype=torch.int64, device=dev)
    mb.sequence_group_rows(b["len"], b["t0"], b["end"], order, seg, total, last_table)
    moments = mb.advantage_moments_sequences(b["adv"], b["len"], b["t0"], b["end"], order, seg, last_table) \
        if adv_norm else None
    stats = torch.zeros((epochs, G, 6), dtype=torch.float64, device=dev)
    gate = total.clone()
    for e in range(epochs):
        adam.zero_grad()
        outs = mb.evaluate_sequences_groups(nets, b["obs"], action, b["len"], b["hidden0"], order, seg)
        g = mb.ppo_loss_sequences(*outs, old_logp, old_value, b["adv"], b["ret"], b["len"], b["t0"], b["end"], order,
                                  seg, total, last_table, clip=clip, value_clip=value_clip, value_coef=value_coef,
                                  entropy_coef=entropy_coef, moments=moments, stats=stats[e])
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
    ap.add_argument("--gated", action="store_true", help="add the gate head to every net")
    ap.add_argument("--epochs", type=int, default=4, help="passes over the batch per update")
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
    import madrona_bots as mb  # noqa: F401
    sim = mb.SimManager(0, args.worlds, args.seed, args.agents, exec_mode=args.exec_mode,
                        reward_fixed=args.reward_fixed)
    starts = [u * args.worlds // args.groups for u in range(args.groups)]
    modules = make_groups([args.hidden[u % len(args.hidden)] for u in range(args.groups)], sim.device, args.seed,
                          args.gated)
    train(sim, starts, modules, args.iters, args.horizon, epochs=args.epochs, clip=args.clip,
          value_clip=args.value_clip, target_kl=args.target_kl, adv_norm=not args.no_adv_norm, lr=args.lr,
          max_grad_norm=args.max_grad_norm, weight_decay=args.weight_decay, log=print)


if __name__ == "__main__":
    main()
