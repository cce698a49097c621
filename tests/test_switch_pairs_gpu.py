"""Every unordered pair of the engine's switches (tests/switches_ref.py) on ONE long-lived bf16 TINY engine, through the public Python
surface.  Every comparison is bit equality of whole probe runs (tests/switch_probe.py: ids, hidden rows, scores, env_state, counters).

  refusal             both orders raise and the message names the switch that is on; afterwards a run is bit-equal to the run under the
                      first switch alone -- a refusal changes no state
  order independence  runs after A -> B and after B -> A are bit-equal
  round trip          under A: r0; B on: r1; B off: r2 == r0; B on: r3 == r1 -- stale graphs, buffers and counters show here
  effect              under A + B both effect probes hold; a NO_EFFECT entry instead has r1 == r0 with its inert switch as B
  lossless            a lossless B leaves ids, hidden rows and scores of r0 unchanged
  fp32 engine         every bf16-only switch refuses with "bf16"; the other setter outcomes equal the table

The engine is never rebuilt between tests: whatever a pair leaves behind, the next pair meets."""
import ctypes as C

import numpy as np
import pytest
import torch

import switch_probe as P
import switches_ref as S

pytestmark = pytest.mark.gpu

ERR = RuntimeError            # _lib.SvlnError and the Python surface's own refusals


@pytest.fixture(scope="module")
def eng():
    m = P.make_model(torch.bfloat16)
    m.probe_on = []
    P.base_state(m)
    m.probe_on = list(S.BASE_ON)
    yield m
    m.close()


@pytest.fixture(scope="module")
def base(eng):
    """the all-off run (the probe's base state: decode graphs, auto-draft armed, packed decode)"""
    restore(eng)
    return P.probe(eng)


def on(m, name):
    S.BY_NAME[name].on(m)
    if name not in m.probe_on:
        m.probe_on.append(name)


def off(m, name):
    S.BY_NAME[name].off(m)
    if name in m.probe_on:
        m.probe_on.remove(name)


def restore(m, dtype=S.BF16):
    """everything off in the fixed order, then the base state"""
    for name in S.RESTORE_ORDER:
        if name in m.probe_on:
            off(m, name)
    for name in S.BASE_ON:
        if dtype in S.BY_NAME[name].dtypes:
            on(m, name)
    assert sorted(m.probe_on) == sorted(n for n in S.BASE_ON if dtype in S.BY_NAME[n].dtypes)


def refused(m, first, second, run=True):
    """with `first` on, `second` raises and names `first`"""
    fn = S.entry(first, second).names[first]
    row = S.BY_NAME[second]
    if not row.call_time:
        with pytest.raises(ERR, match=fn):
            row.on(m)
        return
    row.on(m)                                     # a call-time mode: the flag of the probe driver, then the call
    try:
        with pytest.raises(ERR, match=fn):
            P.probe(m, lock=False)
    finally:
        row.off(m)


def effect_holds(m, name, run, base_run):
    eff = S.BY_NAME[name].effect
    if eff is None:
        return
    kind = eff[0]
    if kind == "stat":
        assert run["stats"][eff[1]] > 0, (name, run["stats"])
    elif kind == "key":
        assert all(eff[1] in t for t in run["solo"]) and all(eff[1] in t for turn in run["lock"] for t in turn), name
    elif kind == "subset":
        ids = [i for t in run["solo"] for i in t["ids"]] + [i for turn in run["lock"] for t in turn for i in t["ids"]]
        extra = () if not m.probe_modes["forced"] else S.FORCED_IDS
        assert ids and set(ids) <= set(S.ALLOWED_IDS) | set(extra), name
    elif kind == "differs":
        assert P.results_of(run, eff[1]) != P.results_of(base_run, eff[1]), f"{name}: the run equals the all-off run in {eff[1]!r}"
    elif kind == "call":
        if name == "generate_group":
            assert len(run["group"]) == len(run["solo"]) and all(len(g["group_ids"]) == 2 for g in run["group"])
        else:
            assert all(t["ids"] == list(S.FORCED_IDS) and "greedy_ids" in t for t in run["solo"])


def outputs_of(run):
    """a run without its counters (what a lossless switch must leave unchanged)"""
    return {k: v for k, v in run.items() if k not in ("stats", "taps")}


def _oriented(a, b):
    """(A, B): B is the inert row of a NO_EFFECT entry, else a lossless row if the pair has one"""
    e = S.entry(a, b)
    if e.kind == S.NO_EFFECT:
        return (a, b) if e.inert == b else (b, a)
    if S.BY_NAME[a].cls == "lossless" and S.BY_NAME[b].cls != "lossless":
        return b, a
    return a, b


@pytest.mark.parametrize("a,b", S.pairs(), ids=[f"{a}-{b}" for a, b in S.pairs()])
def test_pair(eng, base, a, b):
    m, e = eng, S.entry(a, b)
    restore(m)
    try:
        if e.kind == S.REFUSED:
            _refused_pair(m, a, b, e)
        elif e.excluded is not None:
            _accepted_setters_only(m, a, b)
        else:
            _composing_pair(m, base, *_oriented(a, b), e)
    finally:
        _cleanup(m)


def _cleanup(m):
    m.probe_modes.update(group=False, forced=False)
    m.reset(P.N_ENVS)                             # drops turns in flight and a pending group: the setters below need neither
    restore(m)


def _refused_pair(m, a, b, e):
    if a == "generate_group" or b == "generate_group":
        if "generate_forced" in (a, b):
            return _forced_on_a_pending_group(m)
    for first, second in ((a, b), (b, a)):
        if S.BY_NAME[first].call_time:
            continue                              # nothing stays switched on behind a call: the one order that exists is the other one
        restore(m)
        on(m, first)
        alone = P.probe(m) if e.excluded is None else None
        refused(m, first, second)
        if alone is not None:
            P.same(P.probe(m), alone)             # the refusal changed no state
        m.probe_modes.update(group=False, forced=False)


def _forced_on_a_pending_group(m):
    """group x forced: a forced turn on an env whose group is pending.  The Python surface refuses by its own name for the call
    (select_sequence); underneath it the engine refuses by svln_group_select."""
    m.reset(P.N_ENVS)
    ag = P._agent(m, 0, True)
    ag.observe(P.synthetic_frame(0, 0))
    req = ag._build_request("")
    req.update(do_sample=True, temperature=S.SAMPLING[0], num_return_sequences=2)
    out = m.generate(**req)
    state = m.env_state(0)
    forced = dict(ag._build_request(""), forced_ids=list(S.FORCED_IDS))
    with pytest.raises(ERR, match="select_sequence"):
        m.generate(**forced)
    pending = dict(m._group_pending)
    m._group_pending.clear()                      # past the Python guard: the engine's own refusal
    try:
        with pytest.raises(ERR, match="svln_group_select"):
            m.generate(**forced)
    finally:
        m._group_pending.update(pending)
    assert m.env_state(0) == state
    kv = m.select_sequence(1, env_id=0)           # the group is still there, whole
    assert kv.get_seq_length() == state[0] + int(out.sequence_lengths[1]) - 1
    m.set_sampling(None)


def _accepted_setters_only(m, a, b):
    """a pair whose run part is excluded: both orders of the setters are accepted (no turn runs)"""
    for first, second in ((a, b), (b, a)):
        restore(m)
        on(m, first)
        on(m, second)


def _composing_pair(m, base, a, b, e):
    A, B = S.BY_NAME[a], S.BY_NAME[b]
    if b in m.probe_on:                           # a row of the base state as B: the round trip starts with it off
        off(m, b)
    on(m, a)
    r0 = P.probe(m)
    on(m, b)
    r1 = P.probe(m)
    off(m, b)
    P.same(P.probe(m), r0)                        # r2: B left nothing behind
    on(m, b)
    P.same(P.probe(m), r1)                        # r3
    if not (A.call_time or B.call_time):          # (a call-time mode is no state: it has no order)
        restore(m)
        off(m, a)
        off(m, b)
        on(m, b)
        on(m, a)
        P.same(P.probe(m), r1)                    # B -> A
    if e.kind == S.NO_EFFECT:
        P.same(r1, r0)
        effect_holds(m, a, r1, base)
    else:
        effect_holds(m, a, r1, base)
        effect_holds(m, b, r1, base)
    if B.cls == "lossless":
        P.same(outputs_of(r1), outputs_of(r0))


# ---------------------------------------------------------------------------------------------------------------- single rows
@pytest.mark.parametrize("name", S.NAMES)
def test_single_switch_round_trip_and_effect(eng, base, name):
    """every row alone: its effect shows against the all-off run, a lossless one changes nothing, and off is the all-off run again"""
    m = eng
    restore(m)
    try:
        on(m, name)
        r = P.probe(m)
        if name not in S.BASE_ON:                 # (a row of the base state is on in the all-off run as well)
            effect_holds(m, name, r, base)
        if S.BY_NAME[name].cls == "lossless" or name in ("fp8_scaled_mfma", "draft"):
            P.same(outputs_of(r), outputs_of(base))
        off(m, name)
        if name in S.BASE_ON:
            on(m, name)
        P.same(P.probe(m), base)
    finally:
        _cleanup(m)


def test_group_names_the_mode_without_a_sampled_head(eng):
    """svln_set_sampling is refused under the draft switches, the persistent layer and the batched MXFP4 weights, so a group turn cannot
    run under them; through the C ABI the refusal names the switch that is on instead of 'sampling is off'"""
    m = eng
    restore(m)
    out, n_out = np.zeros((2, 8), dtype=np.int64), np.zeros(2, dtype=np.int32)
    eos = np.asarray([2], dtype=np.int64)
    try:
        for name in S.PLAIN_HEAD:
            restore(m)
            on(m, name)
            rc = m._lib.svln_generate_group(m._h, 0, 2, 4, eos.ctypes.data_as(C.POINTER(C.c_int64)), 1, out.ctypes.data_as(C.POINTER(C.c_int64)), 8,
                                            n_out.ctypes.data_as(C.POINTER(C.c_int32)))
            msg = m._lib.svln_last_error().decode()
            assert rc != 0 and S.BY_NAME[name].c_name in msg and "svln_generate_group" in msg, (name, rc, msg)
    finally:
        restore(m)


def test_scheme_setters_refuse_a_change_while_turns_are_in_flight(eng):
    """svln_set_fp8_decode, svln_set_mxfp4_decode, svln_set_fp8_gemm and svln_set_decode_persistent: a change is refused by name while
    scheduler turns are in flight, a call that changes nothing is accepted, and the turn finishes as it does undisturbed"""
    m = eng
    restore(m)

    def one_turn(disturb):
        m.reset(P.N_ENVS)
        ag = P._agent(m, 0, False)
        ag.observe(P.synthetic_frame(0, 0))
        m.submit(**ag._build_request(""))
        if disturb:
            for name in ("fp8_decode", "mxfp4_decode", "fp8_gemm", "decode_persistent"):
                row = S.BY_NAME[name]
                with pytest.raises(ERR, match=f"{row.c_name} cannot change while scheduler turns are in flight"):
                    row.on(m)
                row.off(m)                        # off while off: nothing changes, accepted
        done, hidden = [], None
        while not done:
            done, _ = m.step_batch()
            if not done:
                continue
        return done[0][1].sequences[0].tolist(), list(m.env_state(0))

    try:
        assert one_turn(True) == one_turn(False)
    finally:
        _cleanup(m)


# ---------------------------------------------------------------------------------------------------------------- fp32 engine
def test_fp32_engine_setter_outcomes():
    m = P.make_model(torch.float32)
    m.probe_on = []
    try:
        for r in S.ROWS:
            if S.F32 not in r.dtypes:
                with pytest.raises(ERR, match="bf16"):
                    r.on(m)
                r.off(m)                          # off is always accepted
        setters = [r.name for r in S.ROWS if S.F32 in r.dtypes and not r.call_time]
        for i, a in enumerate(setters):
            for b in setters[i + 1:]:
                e = S.entry(a, b)
                for first, second in ((a, b), (b, a)):
                    restore(m, S.F32)
                    on(m, first)
                    if e.kind == S.REFUSED:
                        refused(m, first, second)
                    else:
                        on(m, second)
        restore(m, S.F32)
        r = P.probe(m, lock=False)                # the engine still runs after all of that
        assert [len(t["ids"]) >= 1 for t in r["solo"]] == [True] * 7
    finally:
        m.close()
