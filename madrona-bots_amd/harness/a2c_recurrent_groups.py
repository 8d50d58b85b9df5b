"""G independent recurrent A2C learners on one manager -- policy groups
(INTEGRATION.md "Policy groups") with nets that carry HiddenState (INTEGRATION.md
"Training the memory head") as runnable code, beside a2c_recurrent.py and
a2c_groups.py, whose pieces it builds on:

    set_policy_groups(starts); per group u: set_policy(nets_u, group=u)
    window.push() -> act() -> step() ... -> window.compute() -> sequences() ->
    batch() / gather() -> per group and species:
    PolicyNet.evaluate_sequences(obs[:, cols], ...) -> the group's loss ->
    backward() -> the group's optimizers -> set_policy(group=u)

A window's sequences come in (start table, start row) order, so one net's
columns are scattered through the batch: the loop finds them with nonzero (a
host wait per net) and copies them out with index_select.

--grouped-evaluate: the learner's half in one call instead --

    net_id = group(world) * 4 + species, built on the device ->
    madrona_bots.sequence_segments(net_id, G) ->
    madrona_bots.evaluate_sequences_groups(nets, obs, action, len, hidden0,
    order, segments) -> one loss over per-column group weights -> one backward()

-- with no .tolist() and no nonzero: the batch is read in place through
`order`, and the host never learns where a net's columns lie.  With nets that
own their parameters it leaves the same bits in every parameter as the loop.
(A net without a column receives zero gradients here, where the loop leaves
its gradients unset and its optimizer skips it.)

--device-update: --grouped-evaluate with the loss and the optimiser in the
library as well --

    sequence_segments -> evaluate_sequences_groups -> sequence_group_rows ->
    a2c_loss_sequences -> autograd.backward -> PolicyAdam.step(rows) -> set_policy

-- the mask, the groups' normalisation and the loss sums in a fixed order, one
optimiser call for all nets (--max-grad-norm, --weight-decay: clipping of every
group's global gradient norm and decoupled weight decay inside it), so the
parameters after the step are the same bits in CPU mode and on the device.  The
update reads the float64 losses once and nothing else.

    python madrona-bots_amd/harness/a2c_recurrent_groups.py --worlds 64 --groups 4 --iters 5 --exec-mode cpu
    python madrona-bots_amd/harness/a2c_recurrent_groups.py --worlds 65536 --groups 32 --iters 20 --grouped-evaluate
    python madrona-bots_amd/harness/a2c_recurrent_groups.py --worlds 65536 --groups 32 --iters 20 --device-update --max-grad-norm 0.5
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from a2c_recurrent import make_modules, policy_net, rollout  # noqa: E402


def window_columns(sim, win, starts_dev, actions, species, worlds):
    """The window's sequences as the learner reads them: (batch dict, action
    [L, B], net_id [B] = group * 4 + species, group [B]), all on the device
    and without a host wait."""
    win.sequences()
    b = win.batch(keys=("rows", "t0", "len", "end", "obs", "adv", "ret", "hidden0"))
    action = win.gather(actions)[:, :, 0]
    sp = win.gather(species)[0, :, 0]                   # a lifeline keeps its species
    world = win.gather(worlds)[0, :, 0].to(torch.int64)  # and its world
    group = torch.bucketize(world, starts_dev, right=True) - 1
    net_id = (group * 4 + sp.to(torch.int64)).to(torch.int32)
    return b, action, net_id, group


def window_batch(sim, win, starts_dev, horizon, actions, species, worlds):
    """window_columns and keep [L, B] float32, the mask of the elements the
    loss counts: (batch dict, action, net_id, group, keep)."""
    b, action, net_id, group = window_columns(sim, win, starts_dev, actions, species, worlds)
    L = b["rows"].shape[0]
    k = torch.arange(L, device=sim.device, dtype=torch.int32)[:, None]
    keep = (b["rows"] >= 0) & (b["t0"][None, :] + k < horizon - 1)                    # not the bootstrap table
    keep &= ~((b["end"] == win.END_RESET)[None, :] & (k == b["len"][None, :] - 1))   # nor a reset's last row
    return b, action, net_id, group, keep.to(torch.float32)


def per_element(logp, value, entropy, adv, ret, value_coef, entropy_coef):
    """The A2C loss of every element, before the keep mask and the group's weight."""
    return -adv * logp + value_coef * (value - ret) ** 2 - entropy_coef * entropy


def train(sim, starts, modules, optimizers, iters, horizon=8, gamma=0.99, lam=0.95, death_reward=-1.0,
          value_coef=0.5, entropy_coef=0.01, log=None, grouped_evaluate=False, device_update=False, lr=3e-4,
          max_grad_norm=None, weight_decay=0.0):
    """`iters` updates of `horizon - 1` steps each of every group.  modules[u],
    optimizers[u]: a2c_recurrent.make_modules' four ModuleDicts and their
    optimizers for group u.  grouped_evaluate: sequence_segments, one
    evaluate_sequences_groups and one backward() in place of the per-net loop.
    device_update: the mask, the loss and the optimiser in the library as well
    (device_update_step); `optimizers` is then a madrona_bots.PolicyAdam over
    the groups' nets, or None for one with learning rate `lr`, max_grad_norm
    and weight_decay.  A group with no kept element is left untouched then --
    parameters, moments and step count -- where the torch paths step it with
    zero gradients.  Returns the losses, [iters][groups] floats."""
    import madrona_bots as mb
    G = len(starts)
    sim.set_policy_groups(starts)
    nets = [[policy_net(m) for m in modules[u]] for u in range(G)]
    for u in range(G):
        sim.set_policy(nets[u], group=u)
    if device_update:
        adam = optimizers if isinstance(optimizers, mb.PolicyAdam) else \
            mb.PolicyAdam(nets, lr=lr, max_grad_norm=max_grad_norm, weight_decay=weight_decay)
    starts_dev = torch.tensor(list(starts), dtype=torch.int64, device=sim.device)
    win = sim.trajectory_window(horizon, max_rows=sim.num_worlds * sim.agent_capacity, record_obs=True,
                                record_state=True)
    losses = []
    try:
        for it in range(iters):
            out, actions, _, species = rollout(sim, win, horizon, gamma, lam, death_reward)
            if device_update:
                b, action, net_id, _ = window_columns(sim, win, starts_dev, actions, species,
                                                      [w.to(torch.int32) for w in out["world"]])
                loss = device_update_step(mb, nets, adam, b, action, net_id, horizon - 1, value_coef, entropy_coef)
                for u in range(G):
                    sim.set_policy(nets[u], group=u)
                win.clear()
                losses.append([float(x) for x in loss.cpu()])                        # the update's one host read
                if log:
                    log(json.dumps({"iter": it, "loss": losses[-1]}))
                continue
            b, action, net_id, group, keep = window_batch(sim, win, starts_dev, horizon, actions, species,
                                                          [w.to(torch.int32) for w in out["world"]])
            # every group's kept elements, at least 1, as a float32 [G] on the device
            total = torch.zeros(G, device=sim.device).index_add_(0, group, keep.sum(dim=0)).clamp_(min=1.0)
            if grouped_evaluate:
                order, seg = mb.sequence_segments(net_id, G)
                logp, value, entropy = mb.evaluate_sequences_groups(nets, b["obs"], action, b["len"], b["hidden0"],
                                                                    order, seg)
                weight = (1.0 / total)[group]                                         # [B]
                per = per_element(logp, value, entropy, b["adv"], b["ret"], value_coef, entropy_coef)
                per = per * (keep * weight[None, :])
                loss = per.sum()
                per_group = torch.zeros(G, device=sim.device).index_add_(0, group, per.detach().sum(dim=0))
                for opts in optimizers:
                    for opt in opts:
                        opt.zero_grad(set_to_none=True)
                loss.backward()
                for opts in optimizers:
                    for opt in opts:
                        opt.step()
                for u in range(G):
                    sim.set_policy(nets[u], group=u)
                win.clear()
                losses.append([float(x) for x in per_group.cpu()])                    # the update's one host read
            else:
                totals = [float(x) for x in total.cpu()]
                loss = [torch.zeros((), device=sim.device) for _ in range(G)]
                for u in range(G):
                    for s, net in enumerate(nets[u]):
                        cols = torch.nonzero(net_id == 4 * u + s).reshape(-1)
                        if cols.numel() == 0:
                            continue
                        take = lambda x: x.index_select(1, cols)
                        logp, value, entropy = net.evaluate_sequences(take(b["obs"]), take(action), b["len"][cols],
                                                                      b["hidden0"][cols])
                        per = per_element(logp, value, entropy, take(b["adv"]), take(b["ret"]), value_coef,
                                          entropy_coef)
                        loss[u] = loss[u] + (per * take(keep)).sum() / totals[u]
                for u in range(G):
                    if not loss[u].requires_grad:
                        continue
                    for opt in optimizers[u]:
                        opt.zero_grad(set_to_none=True)
                    loss[u].backward()
                    for opt in optimizers[u]:
                        opt.step()
                    sim.set_policy(nets[u], group=u)    # same architecture: re-uploads, stream-ordered
                win.clear()
                losses.append([float(x.detach()) for x in loss])
            if log:
                log(json.dumps({"iter": it, "loss": losses[-1]}))
    finally:
        win.close()
    return losses


def device_update_step(mb, nets, adam, b, action, net_id, last_table, value_coef, entropy_coef):
    """One update of every group with the loss and the optimiser in the
    library: sequence_segments, evaluate_sequences_groups, the groups' kept
    elements (sequence_group_rows), a2c_loss_sequences -- the three upstream
    gradients and the groups' losses -- one autograd.backward into the
    gradient buffer `adam` owns and one PolicyAdam.step over every net.
    Returns the losses, float64 [G] on the device; nothing here waits for the
    host, so the whole of it can be captured into a graph."""
    G = len(nets)
    order, seg = mb.sequence_segments(net_id, G)
    outs = mb.evaluate_sequences_groups(nets, b["obs"], action, b["len"], b["hidden0"], order, seg)
    total = torch.zeros(G, dtype=torch.int64, device=net_id.device)
    mb.sequence_group_rows(b["len"], b["t0"], b["end"], order, seg, total, last_table)
    adam.zero_grad()
    g = mb.a2c_loss_sequences(*outs, b["adv"], b["ret"], b["len"], b["t0"], b["end"], order, seg, total, last_table,
                              value_coef, entropy_coef)
    torch.autograd.backward(list(outs), list(g[:3]))
    adam.step(total)
    return g[3]


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
    ap.add_argument("--gated", action="store_true", help="add the gate head to every net (a2c_recurrent.py --gated)")
    ap.add_argument("--grouped-evaluate", action="store_true",
                    help="one evaluate_sequences_groups and one backward() per update instead of one "
                         "evaluate_sequences per (group, species)")
    ap.add_argument("--device-update", action="store_true",
                    help="--grouped-evaluate with sequence_group_rows, a2c_loss_sequences and one PolicyAdam.step in "
                         "place of torch's mask, loss and optimizers")
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
    modules = [make_modules(args.hidden[u % len(args.hidden)], sim.device, args.seed + u, args.gated)
               for u in range(args.groups)]
    optimizers = None if args.device_update else \
        [[torch.optim.Adam(m.parameters(), lr=args.lr) for m in four] for four in modules]
    train(sim, starts, modules, optimizers, args.iters, args.horizon, log=print,
          grouped_evaluate=args.grouped_evaluate, device_update=args.device_update, lr=args.lr,
          max_grad_norm=args.max_grad_norm, weight_decay=args.weight_decay)


if __name__ == "__main__":
    main()
