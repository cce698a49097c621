"""The dealing logic of the persistent decode layer (streamvln_amd/csrc/decode_layer_walk.h: op_row, op_slots, LoadCur, CompCur) through
svln_decode_layer_walk, on the CPU: for one op, every wave's complete slot sequence in the order `prefetch` + `product` impose, checked
against a few lines of Python that restate the intended dealing (tests/decode_layer_ref.py: dealt, op_row, matrix_rows).

For every (element size, blocks per row, rows, pair, first, next op), over the 8 waves and lanes 0 and 63:
  1. every (row, block) of the share is computed exactly once -- wave w computes exactly dealt(bpr, nrows, w), in that order;
  2. the load cursor and the compute cursor agree: the load that filled the register slot k consumes was the load of slot k's block;
  3. every load -- padding slots and the refills from the next op included -- lies inside the op's matrix;
  4. the slot count is a multiple of PF, at least PF, the dealt blocks rounded up; the last group refills with the next op's prefetch;
  5. "row complete" fires exactly at a wave's last block of every row it has a block of (in block mode: for all 8 waves of every row)."""
import ctypes as C
import functools

import numpy as np
import pytest

import decode_layer_ref as R
from streamvln_amd import _lib

PF, NW, BLK = R.PF, R.NW, R.BLK
MAX_SLOTS = 1 << 13
SLOT = np.dtype([("load_off", "<i8"), ("valid", "<i4"), ("row", "<i4"), ("pb", "<i4"), ("row_done", "<i4")])
assert SLOT.itemsize == C.sizeof(_lib.SvlnDecodeLayerSlot)
_BUF = (_lib.SvlnDecodeLayerSlot * MAX_SLOTS)()
FIRSTS = (0, 1, 31, 37, 64 * 5 + 33, 4096)


def walk(op, nxt, wave, lane):
    """(slots as a structured array, refill offsets [PF]) of one wave and lane"""
    buf, n, refill = _BUF, C.c_int32(0), (C.c_int64 * PF)()
    _lib.check(_lib.load().svln_decode_layer_walk(C.byref(_lib.SvlnDecodeLayerWalkOp(*op)), C.byref(_lib.SvlnDecodeLayerWalkOp(*nxt)), wave, lane,
                                                  buf, MAX_SLOTS, C.byref(n), refill))
    return np.frombuffer(buf, dtype=SLOT, count=n.value).copy(), np.array(refill[:], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def next_prefetch(nxt, w):
    return walk(nxt, nxt, w, 0)[0]["load_off"][:PF]


@functools.lru_cache(maxsize=4096)
def expected(bpr, nrows, w):
    """dealt blocks of wave w as arrays (row, block, is the wave's last block of the row)"""
    d = np.array(R.dealt(bpr, nrows, w), dtype=np.int64).reshape(-1, 2)
    last = np.ones(len(d), dtype=bool)
    last[:-1] = d[1:, 0] != d[:-1, 0]
    return d[:, 0], d[:, 1], last


def next_ops(es):
    """products that can follow: whole-row dealt, paired, block-dealt, and a single short row; (None = the op itself, the last product)"""
    e = 1024 // es
    return (None, (es, 3 * e, 5, 0, 10), (es, 7 * e, 12, 1, 38), (es, 37 * e, 3, 0, 6), (es, e, 1, 0, 0))


def in_bounds(off, op, lane):
    es, K, nrows, pair, first = op
    hi = R.matrix_rows(nrows, pair, first) * K * es - BLK + lane * 16
    return bool(((off >= lane * 16) & (off <= hi) & ((off - lane * 16) % BLK == 0)).all())


def check(op, nxt):
    es, K, nrows, pair, first = op
    bpr, ld = K * es // BLK, K * es
    nxt = nxt or op
    seen = []
    for w in range(NW):
        s0, refill0 = walk(op, nxt, w, 0)
        s63, refill63 = walk(op, nxt, w, 63)
        what = (op, nxt, w)
        er, eb, elast = expected(bpr, nrows, w)
        # 4: slot count
        ns = len(s0)
        assert ns % PF == 0 and ns >= PF and ns == R.slots(len(er)) == len(s63), what
        # 1: the valid slots are this wave's dealt blocks, in order
        v = s0[s0["valid"] != 0]
        assert np.array_equal(v["row"], er) and np.array_equal(v["pb"], eb), what
        seen.append(er * bpr + eb)
        # 2: the buffer a valid slot consumes holds that slot's block
        if pair:
            j = first + (er >> 1)
            rows = (j >> 5) * 64 + (j & 31) + (er & 1) * 32
        else:
            rows = first + er
        assert all(int(rows[i]) == R.op_row(first, pair, int(er[i])) for i in range(0, len(er), 7)), what
        assert np.array_equal(v["load_off"], rows * ld + eb * BLK), what
        assert np.array_equal(s63["load_off"], s0["load_off"] + 63 * 16) and np.array_equal(refill63, refill0 + 63 * 16), what
        assert all(np.array_equal(s63[f], s0[f]) for f in ("valid", "row", "pb", "row_done")), what
        # 3: every load in bounds
        assert in_bounds(s0["load_off"], op, 0) and in_bounds(s63["load_off"], op, 63), what
        assert in_bounds(refill0, nxt, 0) and in_bounds(refill63, nxt, 63), what
        # 4: the last group is refilled with what the next op's prefetch loads
        assert np.array_equal(refill0, next_prefetch(nxt, w)), what
        # 5: row completion at this wave's last block of each of its rows, and nowhere else
        assert np.array_equal(v["row_done"] != 0, elast), what
        if bpr > R.ROWMODE_MAX_BPR:
            assert np.array_equal(np.unique(er), np.arange(nrows)), what         # every (row, wave) pair has a block, so each fires
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(nrows * bpr)), (op, "every block exactly once")


def sweep(es, bprs, nrows_of, pairs, per_shape):
    e = BLK // es
    nx = next_ops(es)
    i = 0
    for bpr in bprs:
        for nrows in nrows_of:
            for pair in pairs:
                if pair and nrows % 2:
                    continue
                # `per_shape` (first, next op) combinations per shape; the lists are walked cyclically so that all pairings come up over
                # the sweep (test_every_first_and_next has the full cross on a few shapes)
                for _ in range(per_shape):
                    i += 1
                    yield (es, bpr * e, nrows, pair, FIRSTS[i % len(FIRSTS)]), nx[(i // len(FIRSTS) + i) % len(nx)]


@pytest.mark.parametrize("es", (2, 4))
def test_row_mode(es):
    for op, nxt in sweep(es, range(1, 16), range(0, 131), (0, 1), 2):
        check(op, nxt)


@pytest.mark.parametrize("es", (2, 4))
def test_block_mode(es):
    for op, nxt in sweep(es, range(16, 81), range(1, 65), (0,), 1):
        check(op, nxt)


@pytest.mark.parametrize("es", (2, 4))
def test_every_first_and_next(es):
    """the full cross of firsts and next ops on the shapes the engine launches and on the mode boundary"""
    e = BLK // es
    shapes = [(1, 2, 0), (2, 8, 1), (7, 14, 0), (7, 148, 1), (15, 15, 0), (15, 120, 1), (16, 8, 0), (19, 8, 0), (37, 14, 0), (74, 14, 0)]
    for bpr, nrows, pair in shapes:
        for first in FIRSTS:
            for nxt in next_ops(es):
                check((es, bpr * e, nrows, pair, first), nxt)


def test_refusals():
    L = _lib.load()
    buf, n, refill = (_lib.SvlnDecodeLayerSlot * 64)(), C.c_int32(0), (C.c_int64 * PF)()
    ok = _lib.SvlnDecodeLayerWalkOp(2, 512, 4, 0, 0)
    for bad in ((3, 512, 4, 0, 0), (2, 500, 4, 0, 0), (2, 512, -1, 0, 0), (2, 512, 3, 1, 0), (2, 16 * 512, 4, 1, 0)):
        assert L.svln_decode_layer_walk(C.byref(_lib.SvlnDecodeLayerWalkOp(*bad)), C.byref(ok), 0, 0, buf, 64, C.byref(n), refill) != 0, bad
    assert L.svln_decode_layer_walk(C.byref(ok), C.byref(ok), 8, 0, buf, 64, C.byref(n), refill) != 0
    assert L.svln_decode_layer_walk(C.byref(ok), C.byref(ok), 0, 64, buf, 64, C.byref(n), refill) != 0
    assert L.svln_decode_layer_walk(C.byref(_lib.SvlnDecodeLayerWalkOp(2, 512, 999, 0, 0)), C.byref(ok), 0, 0, buf, 64, C.byref(n), refill) != 0   # max_slots
