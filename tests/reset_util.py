"""Shared by the reset / episode tests: the test's own computation of a world's
initial population, and the comparison of a manager's episode exports with the
oracle's."""
import numpy as np

import pyoracle


def initial_positions(seed, A, episode, gw):
    """A world's initial positions: the episode key threefry2x32((seed, 0),
    (episode, gw)), draw c = the first word of threefry2x32(key, (c, 0))
    (rng_draw), agent i at (u(draw 2i) * 128, u(draw 2i + 1) * 96) in float32."""
    key = pyoracle.threefry2x32((seed, 0), (episode, gw))
    u = lambda c: np.float32(pyoracle.lib().orc_sample_uniform(pyoracle.threefry2x32(key, (c, 0))[0]))
    return np.array([[u(2 * i) * np.float32(128.0), u(2 * i + 1) * np.float32(96.0)] for i in range(A)],
                    np.float32)


def episode_errors(mgr, orc, where):
    """The three episode arrays of a manager (its num_worlds exported entries)
    against the oracle's first num_worlds entries (an oracle standing in for a
    shard with its ghost has one world more)."""
    W = mgr.num_worlds
    errs = []
    for name, o in (("episode_tensor", orc.episode()), ("episode_step_tensor", orc.episode_step()),
                    ("reset_tensor", orc.reset_flags())):
        g = getattr(mgr, name)().to_torch().cpu().numpy().reshape(-1)
        if not np.array_equal(g, o[:W]):
            bad = np.nonzero(g != o[:W])[0]
            errs.append(f"{where}: {name} differs at worlds {bad[:8].tolist()}: "
                        f"manager {g[bad[:8]].tolist()} oracle {o[bad[:8]].tolist()}")
    return errs
