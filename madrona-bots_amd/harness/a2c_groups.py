"""G independent A2C learners on one manager -- policy groups (INTEGRATION.md
"Policy groups") as runnable code, beside a2c.py, whose pieces it builds on:

    set_policy_groups(starts); per group u: set_policy(nets_u, group=u)
    act() -> window.push(value) -> step() ... -> window.compute() ->
    per group and species: PolicyNet.evaluate(obs[lo:hi], action[lo:hi]) ->
    the group's loss -> backward() -> the group's optimizers -> set_policy(group=u)

Every universe -- a contiguous range of worlds with four nets of its own, of
its own width -- rolls out in the one act() launch of the manager; the flat
[N, ...] tensors of a table are sliced per (group, species) by one
policy_segments().tolist(); each group has a loss, a backward() and optimizers
of its own, over its own rows and parameters.  With reward_fixed managers no
group's update depends on another group's nets; the reference's faithful
reward pays species 4 of a group's last world from the next group's first
world (INTEGRATION.md "Policy groups", "Where groups meet").

--grouped-evaluate: the learner's half in one call per table instead --

    madrona_bots.evaluate_groups(nets, obs, action, segments) -> one loss over
    per-row group weights built on the device from `segments` -> one backward()

-- with no .tolist(): the host never reads the segments, so the update neither
waits for the device nor depends on where the groups' rows lie.  With nets that
own their parameters it leaves the same bits in every parameter as the loop.

    python madrona-bots_amd/harness/a2c_groups.py --worlds 64 --groups 4 --iters 5 --exec-mode cpu
    python madrona-bots_amd/harness/a2c_groups.py --worlds 65536 --groups 32 --iters 20
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from a2c import make_modules  # noqa: E402


def train(sim, starts, modules, optimizers, iters, horizon=8, gamma=0.99, lam=0.95, death_reward=-1.0,
          value_coef=0.5, entropy_coef=0.01, log=None, grouped_evaluate=False, device_update=False, lr=3e-4,
          max_grad_norm=None, weight_decay=0.0):
    """`iters` updates of `horizon - 1` steps each of every group.  modules[u],
    optimizers[u]: a2c.make_modules' four ModuleDicts and their optimizers for
    group u.  grouped_evaluate: one evaluate_groups per table and one
    backward() (train_grouped_update) in place of the per-net loop.
    device_update: the loss and the optimiser in the library as well
    (device_update_step); `optimizers` is then a madrona_bots.PolicyAdam over
    the groups' nets, or None for one with learning rate `lr`, max_grad_norm
    and weight_decay (PolicyAdam's clipping and decoupled weight decay).
    Returns the losses, [iters][groups] floats."""
    import madrona_bots as mb
    G = len(starts)
    sim.set_policy_groups(starts)
    nets = [[mb.PolicyNet.from_torch(m["feature"], m["actor"], m["critic"]) for m in modules[u]] for u in range(G)]
    for u in range(G):
        sim.set_policy(nets[u], group=u)
    if device_update:
        grouped_evaluate = True
        adam = optimizers if isinstance(optimizers, mb.PolicyAdam) else \
            mb.PolicyAdam(nets, lr=lr, max_grad_norm=max_grad_norm, weight_decay=weight_decay)
    win = sim.trajectory_window(horizon, max_rows=sim.num_worlds * sim.agent_capacity)
    seg = torch.empty((G, 4, 2), dtype=torch.int32, device=sim.device)
    losses = []
    try:
        for it in range(iters):
            rows = []                                   # per table: (obs, action, [G][4] (lo, hi))
            for t in range(horizon):
                last = t == horizon - 1                 # the last table only bootstraps
                obs = None if last else sim.construct_obs().clone()
                o = sim.act(write=not last)
                win.push(o["value"])
                if not last:
                    sg = sim.policy_segments(out=seg)
                    rows.append((obs, o["action"], sg.clone() if grouped_evaluate else sg.tolist()))
                    sim.step()
            out = win.compute(gamma=gamma, lam=lam, death_reward=death_reward)
            if grouped_evaluate:
                if device_update:
                    loss, total = device_update_step(mb, nets, adam, rows, out, value_coef, entropy_coef)
                else:
                    loss, total = grouped_update(mb, nets, optimizers, rows, out, win.END_RESET, value_coef,
                                                 entropy_coef)
                for u in range(G):
                    sim.set_policy(nets[u], group=u)
                win.clear()
                losses.append(loss)
                if log:
                    log(json.dumps({"iter": it, "loss": loss, "rows": total}))
                continue
            loss = [torch.zeros((), device=sim.device) for _ in range(G)]
            total = [sum(hi - lo for _, _, sg in rows for lo, hi in sg[u]) for u in range(G)]
            for t, (obs, action, sg) in enumerate(rows):
                keep = (out["end"][t].reshape(-1) != win.END_RESET).to(torch.float32)
                for u in range(G):
                    for net, (lo, hi) in zip(nets[u], sg[u]):
                        if hi == lo:
                            continue
                        logp, value, entropy = net.evaluate(obs[lo:hi], action[lo:hi])
                        adv, ret = out["adv"][t][lo:hi, 0], out["ret"][t][lo:hi, 0]
                        per_row = -adv * logp + value_coef * (value - ret) ** 2 - entropy_coef * entropy
                        loss[u] = loss[u] + (per_row * keep[lo:hi]).sum() / total[u]
            for u in range(G):
                if not total[u]:
                    continue
                for opt in optimizers[u]:
                    opt.zero_grad(set_to_none=True)
                loss[u].backward()
                for opt in optimizers[u]:
                    opt.step()
                sim.set_policy(nets[u], group=u)        # same architecture: re-uploads, stream-ordered
            win.clear()
            losses.append([float(x.detach()) for x in loss])
            if log:
                log(json.dumps({"iter": it, "loss": losses[-1], "rows": total}))
    finally:
        win.close()
    return losses


def grouped_update(mb, nets, optimizers, rows, out, end_reset, value_coef, entropy_coef):
    """One update of every group from the recorded tables `rows` -- (obs,
    action, segments [G, 4, 2] on the device) -- and the window's `out`: one
    evaluate_groups per table, the groups' losses summed into one scalar, one
    backward().  Row r of group u weighs keep[r] / total[u], total[u] the
    group's rows over all tables: what the loop's `.sum() / total[u]` hands
    every row's gradient, so the parameters receive the loop's bits.  (A group
    without a row receives zero gradients here, where the loop skips its
    optimizers.)  Returns ([G] losses, [G] rows) as Python numbers, read from
    the device once, after the optimizers' steps."""
    G = len(nets)
    dev = rows[0][0].device
    spans = torch.stack([sg for _, _, sg in rows]).to(torch.int64)             # [T, G, 4, 2]
    total = (spans[..., 1] - spans[..., 0]).sum(dim=(0, 2))                    # [G]
    weight = torch.cat([torch.zeros(1, device=dev), torch.where(total > 0, 1.0 / total.to(torch.float32), 0.0)])
    ids = torch.arange(1, G + 1, device=dev).repeat_interleave(4)              # the group of every segment, from 1
    loss = torch.zeros((), device=dev)
    per_group = torch.zeros(G + 1, device=dev)
    for t, (obs, action, sg) in enumerate(rows):
        n = obs.shape[0]
        # the row's group (0: none): +id at lo, -id at hi, summed along the rows -- integers, exact
        edge = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        edge.index_add_(0, spans[t, :, :, 0].reshape(-1), ids)
        edge.index_add_(0, spans[t, :, :, 1].reshape(-1), -ids)
        group = edge.cumsum(0)[:n]
        keep = (out["end"][t].reshape(-1) != end_reset).to(torch.float32)
        logp, value, entropy = mb.evaluate_groups(nets, obs, action, sg)
        adv, ret = out["adv"][t][:, 0], out["ret"][t][:, 0]
        per_row = (-adv * logp + value_coef * (value - ret) ** 2 - entropy_coef * entropy) * (keep * weight[group])
        loss = loss + per_row.sum()
        per_group.index_add_(0, group, per_row.detach())
    for opts in optimizers:
        for opt in opts:
            opt.zero_grad(set_to_none=True)
    loss.backward()
    for opts in optimizers:
        for opt in opts:
            opt.step()
    host = torch.cat([per_group[1:].to(torch.float64), total.to(torch.float64)]).cpu()
    return [float(x) for x in host[:G]], [int(x) for x in host[G:]]


def device_update_step(mb, nets, adam, rows, out, value_coef, entropy_coef):
    """grouped_update with the loss and the optimiser in the library: per table
    evaluate_groups, a2c_loss_groups (the three upstream gradients and the
    groups' losses, float64 [G] on the device) and one autograd.backward into
    the gradient buffer `adam` owns; then one PolicyAdam.step over every net.
    A group without a row is left untouched, as the loop leaves it.  Returns
    ([G] losses, [G] rows), read from the device once, after the step."""
    G = len(nets)
    dev = rows[0][0].device
    total = torch.zeros(G, dtype=torch.int64, device=dev)
    for _, _, sg in rows:
        mb.policy_group_rows(sg, total)
    loss = torch.zeros(G, dtype=torch.float64, device=dev)
    adam.zero_grad()
    for t, (obs, action, sg) in enumerate(rows):
        outs = mb.evaluate_groups(nets, obs, action, sg)
        g = mb.a2c_loss_groups(*outs, out["adv"][t], out["ret"][t], out["end"][t], sg, total, value_coef, entropy_coef,
                               loss=loss)
        torch.autograd.backward(list(outs), list(g[:3]))
    adam.step(total)
    host = torch.cat([loss, total.to(torch.float64)]).cpu()
    return [float(x) for x in host[:G]], [int(x) for x in host[G:]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--hidden", type=int, nargs="+", default=[128, 64],
                    help="trunk widths, cycled over the groups (universes differ in architecture)")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=69)
    ap.add_argument("--exec-mode", choices=("hip", "cpu"), default="hip" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--reward-fixed", action="store_true", help="rewards[speciesID - 1]: universes fully apart")
    ap.add_argument("--grouped-evaluate", action="store_true",
                    help="one evaluate_groups and one backward() per update instead of one evaluate per (group, species)")
    ap.add_argument("--device-update", action="store_true",
                    help="--grouped-evaluate with a2c_loss_groups and one PolicyAdam.step in place of torch's loss "
                         "and optimizers")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="with --device-update: clip every group's global gradient norm to this")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="with --device-update: decoupled weight decay")
    args = ap.parse_args()
    if (args.max_grad_norm is not None or args.weight_decay) and not args.device_update:
        ap.error("--max-grad-norm and --weight-decay need --device-update")
    if not 1 <= args.groups <= 64 or args.worlds < args.groups:
        ap.error("--groups must be in [1, 64] and at most --worlds")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import madrona_bots as mb
    sim = mb.SimManager(0, args.worlds, args.seed, args.agents, exec_mode=args.exec_mode,
                        reward_fixed=args.reward_fixed)
    starts = [u * args.worlds // args.groups for u in range(args.groups)]
    modules = [make_modules(args.hidden[u % len(args.hidden)], sim.device, args.seed + u) for u in range(args.groups)]
    optimizers = None if args.device_update else \
        [[torch.optim.Adam(m.parameters(), lr=args.lr) for m in four] for four in modules]
    train(sim, starts, modules, optimizers, args.iters, args.horizon, log=print,
          grouped_evaluate=args.grouped_evaluate, device_update=args.device_update, lr=args.lr,
          max_grad_norm=args.max_grad_norm, weight_decay=args.weight_decay)


if __name__ == "__main__":
    main()
