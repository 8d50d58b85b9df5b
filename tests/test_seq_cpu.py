"""CPU mode: the trajectory window's sequences, batches and gathers
(include/mbots.h "Sequences for a recurrent learner") against the numpy
restatement of tests/seq_ref.py, bitwise.  tests/test_seq_gpu.py runs the same
bodies on the device."""
import pytest

import seq_ref as sr


def test_sequences_equal_the_restatement():
    """sequences() and the SEQ_ID / SEQ_POS views on P4, R4, P20 and R20."""
    sr.numbering_scenarios(sr.cpu)


@pytest.mark.parametrize("fixd", [False, True])
@pytest.mark.parametrize("reset", [False, True])
def test_batches_equal_the_restatement(reset, fixd):
    """batch(0, S) and its pieces [0, 1), [1, 130), [130, S) for every key, with
    64-B and 96-B records."""
    sr.batches_scenario(sr.cpu, reset, fixd)


@pytest.mark.parametrize("fixd", [False, True])
def test_obs_equal_the_oracle(fixd):
    sr.oracle_obs_scenario(sr.cpu, fixd)


def test_gather_equals_numpy_indexing():
    sr.gather_scenario(sr.cpu)


def test_ring_wrap_keeps_the_kept_tables_records():
    sr.ring_scenario(sr.cpu)


def test_growth_leaves_the_records_intact():
    sr.growth_scenario(sr.cpu)


def test_errors_and_a_flagless_window():
    sr.errors_scenario(sr.cpu)


def test_two_shards_equal_one_manager():
    sr.shards_scenario(sr.cpu)
