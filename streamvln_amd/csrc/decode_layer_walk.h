// The dealing logic of the persistent decode layer (decode_layer.hip): which 1 KiB weight block every slot of every wave loads, which
// (row, block) of the product it is, and when a wave's partial sum of a row is complete.  Host and device: the kernel walks these cursors
// in `prefetch` / `product`; svln_decode_layer_walk (bottom of decode_layer.hip) walks the same cursors on the host, so that
// tests/test_decode_layer_walk.py can check the dealing without a GPU.
#pragma once
#include "common.h"

namespace svln {

constexpr int BLK = 1024;                       // bytes one wave instruction moves (64 lanes x 16 B)
constexpr int NW = 8;                           // waves per workgroup: all of them stream and compute
constexpr int PF = 16;                          // blocks in flight per wave (16 KB: 128 KB per CU; 24 measured slower -- 230 VGPRs -- and 32 no longer unrolls into registers)
constexpr int ROWMODE_MAX_BPR = 15;             // rows of at most this many blocks go to one wave whole

struct Op {            // one product as this CU sees it
    const char* W; size_t ld_bytes;      // weight matrix, row pitch in bytes
    int bpr;                             // 1 KiB blocks per row
    int nrows, pair, first;              // stream rows; pair: rows come as (gate j, up j) of the [gate 32 | up 32] packing; first output index
    int nblk;                            // blocks of this CU's share
    int ch;                              // blocks dealt to a wave at a time: bpr (whole rows) or 1
    int bm;                              // block mode: rows longer than ROWMODE_MAX_BPR blocks, dealt block by block (ch = 1)
};

SVLN_HD size_t op_row(const Op& o, int j) {                   // matrix row of stream row j
    if (!o.pair) return (size_t)(o.first + j);
    return swiglu_gate_row(o.first + (j >> 1)) + (j & 1) * 32;
}
// slots of wave w in op o (chunks of o.ch blocks dealt round-robin), rounded up to whole groups of PF
SVLN_HD int op_slots(const Op& o, int w) {
    const int nchunk = (o.nblk + o.ch - 1) / o.ch;
    const int mine = nchunk > w ? (nchunk - w + NW - 1) / NW : 0;
    const int ns = (mine * o.ch + PF - 1) / PF * PF;
    return ns < PF ? PF : ns;            // at least one group, even without work: the last group of an op is where the next op's first PF slots are loaded
}
// Walking the slots of one wave through one op.  Row mode (o.ch == o.bpr): a chunk is one stream row, rows w, w + NW, ...; block mode
// (o.ch == 1, rows longer than ROWMODE_MAX_BPR blocks, stored back to back): blocks w, w + NW, ... of the CU's contiguous share.
// LoadCur yields the source address of every slot (a padding slot re-reads the op's first block); CompCur says which (row, block) a
// slot is and when a row's partial sum is complete.
struct LoadCur {
    const char* ptr; int kc, row, gb;
    SVLN_HD const char* row_ptr(const Op& o, int r, int lane) const { return o.W + op_row(o, r < o.nrows ? r : 0) * o.ld_bytes + lane * 16; }
    SVLN_HD void start(const Op& o, int w, int lane) {
        kc = 0; row = w; gb = w;
        ptr = o.bm ? (w < o.nblk ? o.W + (size_t)o.first * o.ld_bytes + (size_t)w * BLK + lane * 16 : o.W + lane * 16) : row_ptr(o, w, lane);
    }
    SVLN_HD void next(const Op& o, int lane) {
        if (o.bm) {
            gb += NW;
            ptr = gb < o.nblk ? ptr + (size_t)NW * BLK : o.W + (size_t)o.first * o.ld_bytes + lane * 16;
        } else if (++kc == o.ch) {
            kc = 0; row += NW;
            ptr = row_ptr(o, row, lane);
        } else {
            ptr += BLK;
        }
    }
};
struct CompCur {
    int kc, row, pb, gb;
    SVLN_HD void start(const Op& o, int w) {
        kc = 0; gb = w;
        if (o.bm) { row = w / o.bpr; pb = w - row * o.bpr; } else { row = w; pb = 0; }
    }
    SVLN_HD bool valid(const Op& o) const { return o.bm ? gb < o.nblk : row < o.nrows; }
    // returns true when the slot just consumed was the last one of its row FOR THIS WAVE (its partial sum is complete)
    SVLN_HD bool next(const Op& o) {
        if (o.bm) {
            gb += NW; pb += NW;
            if (pb >= o.bpr) { pb -= o.bpr; ++row; return true; }
            return false;
        }
        if (++kc == o.ch) { kc = 0; row += NW; pb = 0; return true; }
        ++pb;
        return false;
    }
};

}  // namespace svln
