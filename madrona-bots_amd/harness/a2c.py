"""A2C on the device's own arithmetic -- the learner loop of INTEGRATION.md
"Learning from what act() did" as runnable code, beside rollout.py:

    act() -> window.push(value) -> step() ... -> window.compute() ->
    PolicyNet.evaluate(obs, action) -> loss -> backward() -> optimizer.step()
    -> set_policy()

act() rolls out on the matrix cores; evaluate() reproduces its logp and value
bit for bit on the recorded rows and is differentiable with respect to the
nets' parameters through the library's own backward kernel, so the importance
ratio of the first epoch is exactly 1 and the update gives the same bits in
CPU mode, on the device and in a sharded run.  Losses and optimisers are plain
torch; with --device-update they are the library's too (a2c_loss_groups and
PolicyAdam: a2c_groups.py's device update with one group), and the parameters
after the optimiser's step are the same bits in CPU mode and on the device.

    python madrona-bots_amd/harness/a2c.py --worlds 64 --iters 10 --exec-mode cpu
    python madrona-bots_amd/harness/a2c.py --worlds 4096 --iters 50
"""
import argparse
import json
import os
import sys

import torch

NUM_SPECIES = 4


def make_modules(hidden=128, device="cpu", seed=0):
    """Per species the reference's a2c_nets stacks (learn/models.py): feature,
    actor, critic.  The first Linear is scaled down: observations are raw
    bytes and positions, not normalised."""
    nn = torch.nn
    torch.manual_seed(seed)
    mods = []
    for _ in range(NUM_SPECIES):
        feature = nn.Sequential(nn.Linear(69, hidden), nn.Linear(hidden, hidden), nn.Tanh(),
                                nn.Linear(hidden, hidden), nn.ReLU())
        actor = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, 6))
        critic = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, 1))
        with torch.no_grad():
            feature[0].weight.mul_(0.01)
        mods.append(nn.ModuleDict({"feature": feature, "actor": actor, "critic": critic}).to(device))
    return mods


def species_slices(sim):
    """[start, end) rows of each species in the current table (learn/env.py:55-57)."""
    end = sim.species_count_tensor().to_torch().sum(dim=0).cumsum(dim=0).tolist()
    return list(zip([0] + [int(e) for e in end[:-1]], [int(e) for e in end]))


def train(sim, modules, optimizers, iters, horizon=8, gamma=0.99, lam=0.95, death_reward=-1.0, value_coef=0.5,
          entropy_coef=0.01, log=None, device_update=False, lr=3e-4, max_grad_norm=None, weight_decay=0.0):
    """`iters` updates of `horizon - 1` steps each.  Returns the losses (floats).
    device_update: a2c_groups.train's device update with one group;
    `optimizers` is then a madrona_bots.PolicyAdam or None."""
    import madrona_bots as mb
    if device_update:
        import a2c_groups
        per_group = a2c_groups.train(sim, [0], [modules], optimizers, iters, horizon, gamma, lam, death_reward,
                                     value_coef, entropy_coef, log, device_update=True, lr=lr,
                                     max_grad_norm=max_grad_norm, weight_decay=weight_decay)
        return [x[0] for x in per_group]
    nets = [mb.PolicyNet.from_torch(m["feature"], m["actor"], m["critic"]) for m in modules]
    sim.set_policy(nets)
    win = sim.trajectory_window(horizon, max_rows=sim.num_worlds * sim.agent_capacity)
    losses = []
    try:
        for it in range(iters):
            rows = []                                   # per table: (obs, action, species slices)
            for t in range(horizon):
                last = t == horizon - 1                 # the last table only bootstraps
                obs = None if last else sim.construct_obs().clone()
                o = sim.act(write=not last)
                win.push(o["value"])
                if not last:
                    rows.append((obs, o["action"], species_slices(sim)))
                    sim.step()
            out = win.compute(gamma=gamma, lam=lam, death_reward=death_reward)
            total = sum(obs.shape[0] for obs, _, _ in rows)
            loss = torch.zeros((), device=sim.device)
            for t, (obs, action, slices) in enumerate(rows):
                keep = (out["end"][t].reshape(-1) != win.END_RESET).to(torch.float32)
                for net, (lo, hi) in zip(nets, slices):
                    if hi == lo:
                        continue
                    logp, value, entropy = net.evaluate(obs[lo:hi], action[lo:hi])
                    adv, ret = out["adv"][t][lo:hi, 0], out["ret"][t][lo:hi, 0]
                    per_row = -adv * logp + value_coef * (value - ret) ** 2 - entropy_coef * entropy
                    loss = loss + (per_row * keep[lo:hi]).sum() / total
            for opt in optimizers:
                opt.zero_grad(set_to_none=True)
            loss.backward()
            for opt in optimizers:
                opt.step()
            sim.set_policy(nets)                        # same architecture: re-uploads, stream-ordered
            win.clear()
            losses.append(float(loss.detach()))
            if log:
                log(json.dumps({"iter": it, "loss": losses[-1], "rows": total}))
    finally:
        win.close()
    return losses


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worlds", type=int, default=64)
    ap.add_argument("--agents", type=int, default=32)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--seed", type=int, default=69)
    ap.add_argument("--exec-mode", choices=("hip", "cpu"), default="hip" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--device-update", action="store_true",
                    help="the loss and the optimiser in the library: a2c_loss_groups and one PolicyAdam.step")
    ap.add_argument("--max-grad-norm", type=float, default=None,
                    help="with --device-update: clip the global gradient norm to this")
    ap.add_argument("--weight-decay", type=float, default=0.0, help="with --device-update: decoupled weight decay")
    args = ap.parse_args()
    if (args.max_grad_norm is not None or args.weight_decay) and not args.device_update:
        ap.error("--max-grad-norm and --weight-decay need --device-update")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import madrona_bots as mb
    sim = mb.SimManager(0, args.worlds, args.seed, args.agents, exec_mode=args.exec_mode)
    modules = make_modules(args.hidden, sim.device, args.seed)
    optimizers = None if args.device_update else [torch.optim.Adam(m.parameters(), lr=args.lr) for m in modules]
    train(sim, modules, optimizers, args.iters, args.horizon, log=print, device_update=args.device_update, lr=args.lr,
          max_grad_norm=args.max_grad_norm, weight_decay=args.weight_decay)


if __name__ == "__main__":
    main()
