"""The random call sequences with episodes
(tests/test_parity_gpu.py::test_random_call_sequences_episodes) in CPU mode, at
the small world counts: the same operations and comparisons against the
oracle, on a machine without a device."""
import pytest

from test_parity_gpu import EPISODE_SEEDS, test_random_call_sequences_episodes as _sequences


@pytest.mark.parametrize("seed", [s for s in EPISODE_SEEDS if s % 4])
def test_random_call_sequences_episodes_cpu_mode(seed):
    _sequences(seed, exec_mode="cpu")
