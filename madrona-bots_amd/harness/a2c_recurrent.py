"""Recurrent A2C on the device's own arithmetic -- the learner loop of
INTEGRATION.md "Training the memory head" as runnable code, beside a2c.py:

    window.push() -> act() -> step() ... -> window.compute() -> sequences() ->
    batch() / gather() -> PolicyNet.evaluate_sequences(obs, action, len, hidden0)
    -> loss -> backward() -> optimizer.step() -> set_policy()

The nets read HiddenState (memory_in) and write it (a memory head): act()
carries the state from step to step through the species sort, the window
records it, and evaluate_sequences() runs each net along its agents' padded
lifelines -- logp, value and the carried state bit for bit what act() produced
-- and backpropagates through time with the library's own kernels, so the
memory head learns, with the same gradient bits in CPU mode and on the device.
Losses and optimisers are plain torch; with --device-update they are the
library's too (sequence_group_rows, a2c_loss_sequences and PolicyAdam:
a2c_recurrent_groups.py's device update with one group), and the parameters
after the optimiser's step are the same bits in CPU mode and on the device.

    python madrona-bots_amd/harness/a2c_recurrent.py --worlds 64 --iters 10 --exec-mode cpu
    python madrona-bots_amd/harness/a2c_recurrent.py --worlds 4096 --iters 50
    python madrona-bots_amd/harness/a2c_recurrent.py --worlds 4096 --iters 50 --gated

--gated: every species' net also carries a gate head Linear(H, 16), Sigmoid, and
its new HiddenState is (1 - z) h + z c (INTEGRATION.md "Training the memory
head"): the update gate lets an agent keep what it knew.
"""
import argparse
import json
import os
import sys

import torch

NUM_SPECIES = 4


def make_modules(hidden=128, device="cpu", seed=0, gated=False):
    """Per species a2c.py's stacks with the 16 HiddenState floats after the 69
    observation floats as the input, and the memory head Linear(H, 16), Tanh;
    gated: and the gate head Linear(H, 16), Sigmoid."""
    nn = torch.nn
    torch.manual_seed(seed)
    mods = []
    for _ in range(NUM_SPECIES):
        feature = nn.Sequential(nn.Linear(85, hidden), nn.Linear(hidden, hidden), nn.Tanh(),
                                nn.Linear(hidden, hidden), nn.ReLU())
        actor = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, 6))
        critic = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, 1))
        memory = nn.Sequential(nn.Linear(hidden, 16), nn.Tanh())
        with torch.no_grad():
            feature[0].weight[:, :69].mul_(0.01)
        parts = {"feature": feature, "actor": actor, "critic": critic, "memory": memory}
        if gated:
            parts["gate"] = nn.Sequential(nn.Linear(hidden, 16), nn.Sigmoid())
        mods.append(nn.ModuleDict(parts).to(device))
    return mods


def policy_net(m):
    """The PolicyNet over one species' modules of make_modules()."""
    import madrona_bots as mb
    return mb.PolicyNet.from_torch(m["feature"], m["actor"], m["critic"], m["memory"], memory_in=True,
                                   gate=m["gate"] if "gate" in m else None)


def species_of_rows(sim):
    """int32 [N, 1]: the species 0..3 of every row of the current (species-sorted) table."""
    count = sim.species_count_tensor().to_torch().sum(dim=0).to(torch.int64)
    return torch.repeat_interleave(torch.arange(NUM_SPECIES, device=count.device), count).to(torch.int32).reshape(-1, 1)


def rollout(sim, win, horizon, gamma=0.99, lam=0.95, death_reward=-1.0):
    """Fill the (empty) window with `horizon` tables of the manager's policy and
    compute its advantages from act()'s own value estimates.  Returns
    (compute()'s views, and per table in its row order: action, value, species).

    push() comes before act(), so that the window records the HiddenState act()
    is about to read; the critic's estimate of a table therefore exists only
    after its push.  It goes into the window's value column -- a view of the
    window's storage -- once a first compute() has told the host the row
    counts, and a second compute() derives adv and ret from it."""
    actions, values, species = [], [], []
    for t in range(horizon):
        last = t == horizon - 1                 # the last table only bootstraps
        win.push()
        o = sim.act(write=not last)
        actions.append(o["action"])
        values.append(o["value"])
        species.append(species_of_rows(sim))
        if not last:
            sim.step()
    out = win.compute(gamma=gamma, lam=lam, death_reward=death_reward)
    for dst, v in zip(out["value"], values):
        dst.copy_(v)
    out = win.compute(gamma=gamma, lam=lam, death_reward=death_reward)
    return out, actions, values, species


def train(sim, modules, optimizers, iters, horizon=8, gamma=0.99, lam=0.95, death_reward=-1.0, value_coef=0.5,
          entropy_coef=0.01, log=None, device_update=False, lr=3e-4, max_grad_norm=None, weight_decay=0.0):
    """`iters` updates of `horizon - 1` steps each.  Returns the losses (floats).
    device_update: a2c_recurrent_groups.train's device update with one group;
    `optimizers` is then a madrona_bots.PolicyAdam or None.  An update with no
    kept element leaves the nets untouched then, where the torch path steps
    them with zero gradients."""
    if device_update:
        import a2c_recurrent_groups
        per_group = a2c_recurrent_groups.train(sim, [0], [modules], optimizers, iters, horizon, gamma, lam,
                                               death_reward, value_coef, entropy_coef, log, device_update=True, lr=lr,
                                               max_grad_norm=max_grad_norm, weight_decay=weight_decay)
        return [x[0] for x in per_group]
    nets = [policy_net(m) for m in modules]
    sim.set_policy(nets)
    win = sim.trajectory_window(horizon, max_rows=sim.num_worlds * sim.agent_capacity, record_obs=True,
                                record_state=True)
    losses = []
    try:
        for it in range(iters):
            _, actions, _, species = rollout(sim, win, horizon, gamma, lam, death_reward)
            win.sequences()
            b = win.batch(keys=("rows", "t0", "len", "end", "obs", "adv", "ret", "hidden0"))
            action = win.gather(actions)[:, :, 0]
            sp = win.gather(species)[0, :, 0]           # a lifeline keeps its species
            L = b["rows"].shape[0]
            k = torch.arange(L, device=sim.device, dtype=torch.int32)[:, None]
            keep = (b["rows"] >= 0) & (b["t0"][None, :] + k < horizon - 1)            # not the bootstrap table
            keep &= ~((b["end"] == win.END_RESET)[None, :] & (k == b["len"][None, :] - 1))   # nor a reset's last row
            total = max(int(keep.sum()), 1)
            loss = torch.zeros((), device=sim.device)
            for s, net in enumerate(nets):
                cols = torch.nonzero(sp == s).reshape(-1)
                if cols.numel() == 0:
                    continue
                take = lambda x: x.index_select(1, cols)
                logp, value, entropy = net.evaluate_sequences(take(b["obs"]), take(action), b["len"][cols],
                                                              b["hidden0"][cols])
                per_row = -take(b["adv"]) * logp + value_coef * (value - take(b["ret"])) ** 2 - entropy_coef * entropy
                loss = loss + (per_row * take(keep).to(torch.float32)).sum() / total
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
    ap.add_argument("--gated", action="store_true", help="add the gate head to every species' net")
    ap.add_argument("--device-update", action="store_true",
                    help="the mask, the loss and the optimiser in the library: sequence_group_rows, "
                         "a2c_loss_sequences and one PolicyAdam.step")
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
    modules = make_modules(args.hidden, sim.device, args.seed, args.gated)
    optimizers = None if args.device_update else [torch.optim.Adam(m.parameters(), lr=args.lr) for m in modules]
    train(sim, modules, optimizers, args.iters, args.horizon, log=print, device_update=args.device_update, lr=args.lr,
          max_grad_norm=args.max_grad_norm, weight_decay=args.weight_decay)


if __name__ == "__main__":
    main()
