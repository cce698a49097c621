"""kv_page_copy_kernel (the fork of a group turn) through svln_op_kv_page_copy on a TINY engine, fp32 and bf16.

The pools get a position-coded pattern from the engine itself: layer 0 is poison-filled (svln_op_fill_attn_state), then a 70-token turn is
prefilled, which writes the roped K and the V rows of 70 positions into the env's pages 0 and 1 of EVERY layer (page 1 partly: the fork's
case).  Every page of every layer and both pools is read before and after each copy (svln_op_kv_read for layer 0, svln_op_kv_pool_read
for any layer): the destinations must be bit-equal to the source, every other page untouched.  n_dst = 1, 2 and 7; source and destination at
the first and the last page of the pool; every malformed call refused with the pools unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from scenarios import SEED
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM

pytestmark = pytest.mark.gpu
PAGE, POISON, N_TOKENS = 64, 6.5, 70
MAX_POSITIONS = 1024                  # 16 pages, one env


def _engine(dtype):
    m = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=1, max_positions=MAX_POSITIONS)
    m.load_synthetic(SEED)
    assert m._lib.svln_op_fill_attn_state(m._h, POISON, 0) == 0
    ids = (np.arange(N_TOKENS, dtype=np.int64) * 37 + 11) % TINY.vocab
    assert m._lib.svln_append_turn(m._h, 0, ids.ctypes.data_as(C.POINTER(C.c_int64)), N_TOKENS, 0) == 0, m._lib.svln_last_error()
    out = np.zeros(1, dtype=np.int64)
    assert m._lib.svln_generate_fixed(m._h, 0, 1, out.ctypes.data_as(C.POINTER(C.c_int64))) == 0, m._lib.svln_last_error()
    return m


def _pools(m):
    """[layer][K | V][page][64 positions][kv_heads][128] of the whole pool, fp32 images of the engine dtype"""
    n = MAX_POSITIONS
    out = np.zeros((TINY.layers, 2, n, TINY.kv_heads, 128), dtype=np.float32)
    pf = C.POINTER(C.c_float)
    for layer in range(TINY.layers):
        assert m._lib.svln_op_kv_pool_read(m._h, layer, 0, n, out[layer, 0].ctypes.data_as(pf), out[layer, 1].ctypes.data_as(pf)) == 0
    k0, v0 = np.zeros_like(out[0, 0]), np.zeros_like(out[0, 0])
    assert m._lib.svln_op_kv_read(m._h, -1, 0, n, k0.ctypes.data_as(pf), v0.ctypes.data_as(pf)) == 0
    assert np.array_equal(k0, out[0, 0]) and np.array_equal(v0, out[0, 1])          # the two readers agree on layer 0
    return out.reshape(TINY.layers, 2, n // PAGE, PAGE, TINY.kv_heads, 128)


def _copy(m, src, dst):
    arr = np.asarray(dst, dtype=np.int32)
    return m._lib.svln_op_kv_page_copy(m._h, int(src), arr.ctypes.data_as(C.POINTER(C.c_int32)), len(dst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_page_copy_is_bit_exact_in_every_layer_and_touches_nothing_else(dtype):
    m = _engine(dtype)
    last = MAX_POSITIONS // PAGE - 1
    before = _pools(m)
    # the pattern is what the test thinks it is: positions 0 .. 69 differ from the poison and from each other, the rest of layer 0 is poison
    assert not np.isnan(before).any()
    flat = before[:, :, :2].reshape(TINY.layers, 2, 2 * PAGE, -1)
    assert all(len({flat[l, kv, p].tobytes() for p in range(N_TOKENS)}) == N_TOKENS for l in range(TINY.layers) for kv in range(2))
    assert (before[0, :, 1, N_TOKENS - PAGE:] == POISON).all() and (before[0, :, 2:] == POISON).all()
    # (source, destinations): the partly filled page -> 1, 2, 7 pages; the pool's first page as a source, its last page as a destination
    # and then as a source
    for src, dst in ((1, [5]), (1, [last, 3]), (1, [2, 4, 6, 8, 10, 12, 14]), (0, [last]), (last, [2, 7])):
        assert _copy(m, src, dst) == 0, m._lib.svln_last_error()
        after = _pools(m)
        for d in dst:
            assert np.array_equal(after[:, :, d], before[:, :, src]), (src, d)
        rest = [p for p in range(last + 1) if p not in dst]
        assert np.array_equal(after[:, :, rest], before[:, :, rest]), (src, dst)
        before = after
    # every malformed call is refused before any launch: the pools do not change
    bad = [(1, []), (1, list(range(2, 10))), (-1, [3]), (last + 1, [3]), (1, [-1]), (1, [last + 1]), (1, [1]), (1, [3, 3]), (3, [4, 3]),
           (2, [0]), (2, [5, 1])]
    for src, dst in bad:
        assert _copy(m, src, dst) != 0, (src, dst)
        assert b"svln_op_kv_page_copy" in m._lib.svln_last_error(), (src, dst)
    assert m._lib.svln_op_kv_page_copy(m._h, 1, None, 2) != 0 and b"null" in m._lib.svln_last_error()
    assert np.array_equal(_pools(m), before)
    assert m._lib.svln_reset_env(m._h, 0) == 0
    m.close()
