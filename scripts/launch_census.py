#!/usr/bin/env python3
"""Launch census of the manager's deferred columns: a fixed list of call
scripts, 20 steps each at 64 worlds of 32 agents (the shape of
tests/test_lazy_hidden.py), and per script the kernel_times() launches of
every kernel class and schedule_info()'s hidden_lazy / prev_action_lazy after
every call.  Two libraries that defer, move and gather the same columns at the
same calls print the same JSON:

    MBOTS_LIB=build_var/libmbots_x.so python scripts/run_variant.py scripts/launch_census.py out.json

Each script also runs with MBOTS_LAZY_PREV_ACTION=0 (read when the manager is
created)."""
import json
import os
import sys

sys.path.append(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "madrona-bots_amd"))

import torch  # noqa: E402

import madrona_bots as mb  # noqa: E402  (run_variant.py's copy when MBOTS_LIB is set)

W, A, STEPS, SEED = 64, 32, 20, 69


def _write(m, t, hidden=False):
    m.write_synthetic_actions(1234, t, hidden)


def headline(m, t, note):
    m.step(); note()
    m.shift_observations(); note()
    _write(m, t); note()


def headline_write_hidden(m, t, note):
    m.step(); note()
    m.shift_observations(); note()
    _write(m, t, True); note()


def training_loop(m, t, note):
    """the reference training loop's pattern: the previous observation and
    PrevHiddenState read between step and shift"""
    m.step(); note()
    m.construct_obs(is_prev=True); note()
    m.hidden_state_tensor(is_prev=True).to_torch(); note()
    m.shift_observations(); note()
    _write(m, t, True); note()


def step_without_shift(m, t, note):
    m.step(); note()
    _write(m, t); note()


def shift_twice(m, t, note):
    m.step(); note()
    m.shift_observations(); note()
    m.shift_observations(); note()
    _write(m, t); note()


def partial_write(m, t, note):
    """write_actions over num_agents() rows of a table with shard-ghost rows
    behind them on every fourth step, the headline loop otherwise"""
    m.step(); note()
    m.shift_observations(); note()
    if t % 4 == 2:
        n = m.num_agents()
        a = torch.zeros((n, 6), dtype=torch.int32, device=m.device)
        a[:, 0] = 1
        m.write_actions(actions=a)
    else:
        _write(m, t)
    note()


def checkpoint_mid_stretch(m, t, note):
    headline(m, t, note)
    if t == 9:
        m.save_checkpoint(); note()


def growth_mid_stretch(m, t, note):
    headline(m, t, note)
    if t == 9:
        m.grow_capacity(256); note()


SCRIPTS = [headline, headline_write_hidden, training_loop, step_without_shift, shift_twice, partial_write,
           checkpoint_mid_stretch, growth_mid_stretch]


def run(script, pa_on=True):
    """{"launches": {kernel class: launches}, "lazy": one digit per call
    (1 hidden_lazy + 2 prev_action_lazy)}"""
    os.environ["MBOTS_LAZY_PREV_ACTION"] = "1" if pa_on else "0"
    try:
        m = mb.SimManager(0, W, SEED, A, shard_ghost=script is partial_write)
    finally:
        del os.environ["MBOTS_LAZY_PREV_ACTION"]
    m.enable_kernel_timing(True)
    lazy = []

    def note():
        s = m.schedule_info()
        lazy.append(str(int(s["hidden_lazy"]) + 2 * int(s["prev_action_lazy"])))
    for t in range(STEPS):
        script(m, t, note)
    torch.cuda.synchronize()
    return {"launches": {k: int(n) for k, (_, n) in m.kernel_times().items()}, "lazy": "".join(lazy)}


def main():
    out = {}
    for pa_on in (True, False):
        for s in SCRIPTS:
            out[s.__name__ + ("" if pa_on else ", MBOTS_LAZY_PREV_ACTION=0")] = run(s, pa_on)
    text = json.dumps(out, indent=1, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
