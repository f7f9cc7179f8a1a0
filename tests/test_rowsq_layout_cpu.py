"""The permuted layout of the RMSNorm sum-of-squares partials (csrc/common.h rowsq_slot), on a Python mirror of the function.
The mirror is pinned to the native function by tests/test_rowsq_layout_gpu.py (the RESID epilogue stores partial j where this
mirror says)."""
import pytest


def rowsq_slot(j, n):
    """csrc/common.h rowsq_slot"""
    return j if n % 64 else 64 * (j >> 6) + 4 * (j & 15) + ((j >> 4) & 3)


@pytest.mark.parametrize("n", [64, 128, 192, 256])
def test_slot_is_a_bijection_that_keeps_partial_zero(n):
    slots = [rowsq_slot(j, n) for j in range(n)]
    assert sorted(slots) == list(range(n))
    assert slots[0] == 0                            # k_rowsq, k_embed_rowsq and the sampler write the total there and zeros elsewhere
    assert slots != list(range(n))


@pytest.mark.parametrize("n", [1, 4, 24, 32, 72])
def test_slot_is_the_identity_for_other_row_lengths(n):
    assert [rowsq_slot(j, n) for j in range(n)] == list(range(n))


@pytest.mark.parametrize("n", [64, 128, 192, 256])
def test_the_four_pieces_of_a_lane_hold_its_sixteen_partials(n):
    """lane r of a 16-lane group sums partials r + 16 it in the order it = 0..15; 16-byte piece q of that lane starts at float
    64 q + 4 r and must hold exactly partials r + 16 (4 q + c), c = 0..3, in that order"""
    where = {rowsq_slot(j, n): j for j in range(n)}
    for r in range(16):
        got = []
        for q in range(n // 64):
            base = 64 * q + 4 * r
            assert base % 4 == 0 and base + 3 < n
            piece = [where[base + c] for c in range(4)]
            assert piece == [r + 16 * (4 * q + c) for c in range(4)]
            got += piece
        assert got == [r + 16 * it for it in range(n // 16)]
