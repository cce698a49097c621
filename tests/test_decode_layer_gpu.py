"""The persistent decode layer kernel (streamvln_amd/csrc/decode_layer.hip) through svln_op_decode_layer -- ONE launch on buffers of the
test's own -- on the cases of tests/decode_layer_ref.py (tests/test_decode_layer_inputs.py proves on the CPU that they are sharp, and
tests/test_decode_layer_walk.py checks the dealing the launch is expected to follow).

Per case: the give-up word is 0; the launch counter grew by 1; every granule of every edge carries this launch's tag; the four edge
payloads, x and qkv_out are compared with the float64 reference STAGE BY STAGE, stage k of the reference fed the kernel's own edge
k - 1 -- torch.equal at the exact stages of the exact family, gemv_ref.bound (util.tol) everywhere else; x equals edge 3 bit for bit;
guard bands around every output stay untouched, and weight rows outside the matrices hold 2^60.
Epochs: a launch on granule buffers another input just used gives the bits it gives on fresh buffers; the same input twice gives the
same bits; a set skip flag leaves everything as it was.  The give-up path is NOT exercised: no case withholds a granule or over-sizes
the grid; the refusals (unsupported shape, more workgroups than CUs) are error returns that launch nothing."""
import ctypes as C
import faulthandler

import pytest
import torch

import decode_layer_ref as R
from streamvln_amd import _lib
from streamvln_amd.config import TINY
from streamvln_amd.model import StreamVLNForCausalLM
from test_e2e_gpu import _note          # the recorder of measured values that DESIGN.md quotes

pytestmark = pytest.mark.gpu
GUARD, FILL, GUARD_ROWS = 64, 777.0, 2
GRAN_FILL = 0x0123456789ABCDEF
TIME_LIMIT = 120          # seconds per test (a launch is microseconds; building a case on the host is the bulk)
_engines = {}


@pytest.fixture(autouse=True)
def _time_limit():
    """each test under its own time limit: a launch that never returns ends the process instead of holding the GPU"""
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def engine(dtype):
    if dtype not in _engines:
        _engines[dtype] = StreamVLNForCausalLM(TINY, dtype=dtype, max_envs=1, max_frames=3, max_positions=2048)
    return _engines[dtype]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _p(t):
    return t.data_ptr() if t is not None else None


class Buffers:
    """device operands of one case; every output sits between guard bands"""

    def __init__(self, case, seq0=None):
        case.build()
        self.case, dt = case, case.dtype
        self.weights = {}
        for name in ("o_w", "gu_w", "down_w", "qkv_w"):
            W = getattr(case, name)
            buf = torch.full((W.shape[0] + 2 * GUARD_ROWS, W.shape[1]), R.POISON, dtype=dt)       # rows outside the matrix proper: 2^60
            buf[GUARD_ROWS:GUARD_ROWS + W.shape[0]] = W.to(dt)
            self.weights[name] = buf.cuda()
        vec = lambda v: None if v is None else v.to(dt).cuda()
        self.post_norm, self.next_norm, self.qkv_b = vec(case.post_norm), vec(case.next_norm), vec(case.qkv_b)
        self.part = case.part.float().cuda()
        self.kv_len = torch.tensor([case.kv_len], dtype=torch.int32).cuda()
        self.skip = torch.zeros(1, dtype=torch.int32).cuda()
        self.xbuf = torch.full((case.H + 2 * GUARD,), FILL, dtype=dt)
        self.xbuf[GUARD:GUARD + case.H] = case.x.to(dt)
        self.xbuf = self.xbuf.cuda()
        self.qbuf = torch.full((case.qkv_dim + 2 * GUARD,), FILL, dtype=dt).cuda()
        self.seq = torch.full((16,), -1, dtype=torch.int32)
        self.seq[0] = case.seq0 if seq0 is None else seq0
        self.seq = self.seq.cuda()
        self.giveup = torch.zeros(16, dtype=torch.int32).cuda()
        self.gran = []
        for e in range(4):
            pre = case.granule_prefill(e)
            g = torch.full((len(pre) + 2 * GUARD,), GRAN_FILL, dtype=torch.int64)
            g[GUARD:GUARD + len(pre)] = pre
            self.gran.append(g.cuda())

    def w(self, name):
        return self.weights[name][GUARD_ROWS:]

    def op(self, cus=None, skip=False):
        c = self.case
        o = _lib.SvlnDecodeLayerOp()
        o.o_w, o.post_norm, o.gu_w, o.down_w = _p(self.w("o_w")), _p(self.post_norm), _p(self.w("gu_w")), _p(self.w("down_w"))
        if c.has_next:
            o.next_norm, o.next_qkv_w, o.next_qkv_b = _p(self.next_norm), _p(self.w("qkv_w")), _p(self.qkv_b)
        o.part, o.kv_len, o.skip = _p(self.part), _p(self.kv_len), _p(self.skip) if skip else None
        o.x, o.qkv_out = _p(self.xbuf[GUARD:]), _p(self.qbuf[GUARD:])
        for e in range(4):
            o.gran[e] = _p(self.gran[e][GUARD:])
        o.seq, o.giveup = _p(self.seq), _p(self.giveup)
        o.nsplit, o.tiles_per_split, o.n_q, o.n_kv, o.H, o.I, o.qkv_dim, o.cus = c.nsplit, c.tps, c.nq, c.nkv, c.H, c.I, c.qkv_dim, cus or c.G
        o.eps = R.EPS
        return o

    def launch(self, m, **kw):
        torch.cuda.synchronize()
        rc = m._lib.svln_op_decode_layer(m._h, C.byref(self.op(**kw)))
        torch.cuda.synchronize()
        return rc

    def read(self):
        """everything a launch may write, on the host"""
        return {"x": self.xbuf.cpu(), "qkv": self.qbuf.cpu(), "seq": self.seq.cpu(), "giveup": self.giveup.cpu(), "gran": [g.cpu() for g in self.gran]}


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in ("x", "qkv")) and torch.equal(a["seq"], b["seq"]) and \
        torch.equal(a["giveup"], b["giveup"]) and all(torch.equal(p, q) for p, q in zip(a["gran"], b["gran"]))


def _guards_intact(case, before, out):
    for k, n in (("x", case.H), ("qkv", case.qkv_dim)):
        assert torch.equal(_bits(out[k][:GUARD]), _bits(before[k][:GUARD])) and torch.equal(_bits(out[k][GUARD + n:]), _bits(before[k][GUARD + n:])), k
    for e in range(4):
        g = out["gran"][e]
        assert bool((g[:GUARD] == GRAN_FILL).all()) and bool((g[-GUARD:] == GRAN_FILL).all()), f"granule guard band of edge {e} written"
    assert bool((out["seq"][1:] == -1).all()) and bool((out["giveup"][1:] == 0).all())


def _compare(case, stage, got, exp, ratios):
    if case.exact_stage(stage):
        bad = ~(got == exp)
        assert not bool(bad.any()), f"{case.id} {stage}: {int(bad.sum())} of {bad.numel()} values differ in their bits, first at {int(torch.nonzero(bad)[0])}: " \
                                    f"{float(got[bad][0])} for {float(exp[bad][0])}"
        return
    dev = R.deviation(case, stage, got, exp)
    ratios[stage] = dev
    print(f"{case.id} {stage}: worst |err| / bound {dev:.2e}")
    assert dev <= 1.0, f"{case.id} {stage}: worst |err| / bound {dev:.2e}"


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_decode_layer(case):
    m = engine(case.dtype)
    b = Buffers(case)
    before = b.read()
    _lib.check(b.launch(m))
    out = b.read()
    assert int(out["giveup"][0]) == 0, f"{case.id}: give-up word {int(out['giveup'][0]):#x}"
    assert int(out["seq"][0]) == case.seq0 + 1
    _guards_intact(case, before, out)
    edges = []
    for e in range(4):
        raw = out["gran"][e][GUARD:-GUARD]
        if e == 3 and not case.has_next:
            assert torch.equal(raw, before["gran"][e][GUARD:-GUARD]), "last layer: edge 3 written"
            edges.append(None)
            continue
        tags, vals = case.unpack(raw)
        bad = tags != case.seq0 * 4 + e + 1
        assert not bool(bad.any()), f"{case.id}: {int(bad.sum())} granules of edge {e} without this launch's tag"
        edges.append(vals)
    attn, x1, h, x2e = edges
    x = out["x"][GUARD:GUARD + case.H].double()
    ratios = {}
    _compare(case, "attn", attn, case.merge(), ratios)
    _compare(case, "x1", x1, case.x1(attn), ratios)
    _compare(case, "h", h, case.swiglu(x1), ratios)
    _compare(case, "x2", x, case.x2(h, x1), ratios)
    q = out["qkv"][GUARD:GUARD + case.qkv_dim]
    if case.has_next:
        assert torch.equal(x2e, x), "x differs from the payload of edge 3"
        _compare(case, "qkv", q.double(), case.qkv(x), ratios)
    else:
        assert torch.equal(_bits(q), _bits(before["qkv"][GUARD:GUARD + case.qkv_dim])), "last layer: qkv_out written"
    _note("decode_layer_stages", f"{case.id}: worst |err| / bound " + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()))


def _pair(name, dtype):
    a, b = [c for c in R.CASES if c.name == name and c.dtype == dtype and c.has_next][:2]
    return a, b


@pytest.mark.parametrize("name,dtype", [("caps", torch.bfloat16), ("blockmode16", torch.float32), ("tiny256", torch.bfloat16)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_epochs(name, dtype):
    """input A then input B on the same granule buffers = B on fresh buffers, bit for bit (tags included: both B launches run at the same
    launch counter); B once more from the same start = the same bits again (the summation order is fixed)"""
    A, B = _pair(name, dtype)
    m = engine(dtype)
    ba, bb = Buffers(A), Buffers(B, seq0=A.seq0 + 1)
    _lib.check(ba.launch(m))
    after_a = ba.read()
    assert int(after_a["giveup"][0]) == 0 and int(after_a["seq"][0]) == A.seq0 + 1
    fresh = Buffers(B, seq0=A.seq0 + 1)
    _lib.check(fresh.launch(m))
    want = fresh.read()
    assert int(want["giveup"][0]) == 0
    bb.gran, bb.seq = ba.gran, ba.seq                       # B on the buffers A's launch left behind
    _lib.check(bb.launch(m))
    got = bb.read()
    assert _same(got, want), "a launch on used granule buffers differs from the launch on fresh ones"
    again = Buffers(B, seq0=A.seq0 + 1)
    _lib.check(again.launch(m))
    assert _same(again.read(), want), "the same input twice gives different bits"


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
def test_skip_flag_and_refusals(dtype):
    case = next(c for c in R.CASES if c.name == "caps" and c.dtype == dtype)
    m = engine(dtype)
    b = Buffers(case)
    b.skip.fill_(1)
    before = b.read()
    _lib.check(b.launch(m, skip=True))
    assert _same(b.read(), before), "a launch with *skip != 0 wrote something"
    # refusals launch nothing: more workgroups than CUs (fp32 TINY shape is admitted at 512 workgroups); a shape past the H limit
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if dtype == torch.float32:
        ok = C.c_int32(0)
        _lib.check(m._lib.svln_decode_layer_supported(_lib.SVLN_F32, case.H, case.I, case.qd, case.qkv_dim, 2 * cus, C.byref(ok)))
        assert ok.value == 1
        assert b.launch(m, cus=2 * cus) != 0 and "CUs" in m._lib.svln_last_error().decode()
        o = b.op()
        o.H = 4096
        assert m._lib.svln_op_decode_layer(m._h, C.byref(o)) != 0 and "not supported" in m._lib.svln_last_error().decode()
    assert b.launch(m, cus=7) != 0 and "not supported" in m._lib.svln_last_error().decode()
    torch.cuda.synchronize()
    assert _same(b.read(), before), "a refused launch wrote something"
