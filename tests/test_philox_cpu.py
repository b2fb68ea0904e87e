"""The NumPy restatement of Philox4x32-10 (tests/mc_ref.py), which the Monte-Carlo tests use to restate the library's step, against
Random123's known-answer vectors."""
import numpy as np

from tests import mc_ref


def words(*h):
    return np.array([int(x, 16) for x in h], np.uint32)


def test_known_answer_zero():
    out = mc_ref.philox4x32_10(np.zeros(4, np.uint32), np.zeros(2, np.uint32))
    assert np.array_equal(out, words("6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"))


def test_known_answer_pi():
    out = mc_ref.philox4x32_10(words("243f6a88", "85a308d3", "13198a2e", "03707344"), words("a4093822", "299f31d0"))
    assert np.array_equal(out, words("d16cfe09", "94fdcceb", "5001e420", "24126ea1"))


def test_block_counter_and_key_layout():
    """block(step, gid, blk, seed) is Philox with counter (step, gid, blk, 0) and key (seed low word, seed high word)"""
    seed = 0x299F31D0A4093822
    out = mc_ref.block(0x243F6A88, np.array([0x85A308D3]), 0x13198A2E, seed)[0]
    ref = mc_ref.philox4x32_10(words("243f6a88", "85a308d3", "13198a2e", "00000000"), words("a4093822", "299f31d0"))
    assert np.array_equal(out, ref)
    u = mc_ref.uniform(np.array([0, 0xFFFFFFFF], np.uint32))
    assert u[0] == 0.5 * 2.0 ** -32 and u[1] == 1.0 - 0.5 * 2.0 ** -32
