"""The deferred columns launch what they launched before they moved into
csrc/mbots_defer.hpp: three of scripts/launch_census.py's call scripts (the
headline loop, the reference training loop's pattern, step without shift), 20
steps at 64 worlds of 32 agents, and the kernel_times() launches of every
kernel class.  The expected counts are the parent commit's census
(profiles/defer_refactor_census_parent.json), not the code under test's."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))
import launch_census  # noqa: E402

pytestmark = pytest.mark.gpu


def _launches(**n):
    return dict({"world_step": 20, "scan": 20, "export": 20, "sensor": 20, "actions": 20, "move": 0, "shift": 0,
                 "obs": 0}, **n)


# per script: launches per kernel class, and one digit per call (1 hidden_lazy +
# 2 prev_action_lazy)
EXPECTED = {
    # one fused shift, then every shift owes both columns and launches nothing
    "headline": (_launches(shift=1), "0000" + "3" * 56),
    # the reads between step and shift are moved (the first step) or
    # prefetched (every later one: one move launch a step); nothing goes lazy
    "training_loop": (_launches(move=20, shift=20, obs=20), "0" * 100),
    # every step's deferred moves run at the next step
    "step_without_shift": (_launches(move=58), "0" * 40),
}


@pytest.mark.parametrize("script", sorted(EXPECTED))
def test_launches_per_class(script):
    got = launch_census.run(getattr(launch_census, script))
    print(script, got)
    launches, lazy = EXPECTED[script]
    assert got["launches"] == launches
    assert got["lazy"] == lazy
