"""CPU checks of the inputs of tests/test_p12_depth_gpu.py (tests/p12_depth_ref.py): every case's planted fallback blocks are what the
encoder of tests/p12_ref.py produces (build() asserts masks and count against the plan), every fallback pattern occurs in both kernels
at every load-step geometry the cases were chosen for, and a special row keeps its NaN / -0 / denormal blocks packed next to a fallback."""
import numpy as np
import pytest

import p12_depth_ref as D
import p12_ref as R


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.id)
def test_the_encoder_produces_the_planted_pattern(case):
    case.build()
    assert np.array_equal(R.decode(case.packed[:case.period], case.rec[:case.period], case.w[:case.period]), case.w[:case.period])


def test_every_pattern_occurs_in_both_kernels_and_every_own_block_count():
    seen = {"rows": set(), "ksplit": set()}
    for c in D.CASES:
        seen[c.kernel] |= set(c.build().patterns_present)
    for kernel in seen:
        assert seen[kernel] == set(D.PATTERNS), (kernel, seen[kernel])
    counts = {len(D.own_blocks(-(-K // R.BLOCK), "ksplit", 0)) for K in D.KSPLIT_K}
    assert counts >= set(range(1, 2 * D.KS_DEPTH + 2)), counts
    assert {-(-K // R.BLOCK) for K in D.ROWS_K} >= {1, 2, 3, 4, 5, 7} and sum(K % R.BLOCK != 0 for K in D.ROWS_K) == 2
    assert any(K % R.BLOCK for K in D.KSPLIT_K)


def test_pattern_slots():
    own, d = 7, 3                                   # the flagship row in the row kernel: steps (0 1 2) (3 4 5), remainder 6
    assert [D.pattern_blocks(p, own, "rows", 0, d) for p in ("first", "middle", "last", "remainder", "adjacent", "ragged")] == [[0], [1], [2], [6], [2, 3], [6]]
    assert D.pattern_blocks("row", own, "rows", 0, d) == list(range(7)) and D.pattern_blocks("none", own, "rows", 0, d) == []
    # K-split, wave 1 of 37 blocks owns 1, 5, ..., 33: steps (1 5 9) (13 17 21) (25 29 33), no remainder -> its last block
    assert [D.pattern_blocks(p, 37, "ksplit", 1, d) for p in ("first", "middle", "last", "remainder", "adjacent")] == [[1], [5], [9], [33], [9, 13]]
    assert D.pattern_blocks("last", 2, "rows", 0, d) == [1]          # fewer blocks than the depth: singles only


def test_special_rows_keep_their_special_blocks_packed():
    for nan in (False, True):
        row = D.special_row(2560, [1], 5, nan)
        packed, rec, n_fb = R.encode(row[None])
        assert R.masks_of(rec) == [0b00010] and n_fb == 1
        near = np.concatenate([row[:512], row[1024:1536]])
        assert (near == 0x8000).any() and ((near & 0x7F80) == 0).any() and (((near & 0x7F80) == 0x7F80) & ((near & 0x7F) != 0)).any() == nan
        assert np.array_equal(R.decode(packed, rec, row[None]), row[None])
