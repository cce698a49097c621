"""The fixed probe workload of the switch-pair and weight-rewrite tests (test infrastructure): one bf16 / fp32 TINY engine with four env
slots through the public Python surface, and everything a run returns as bit patterns, so that two runs compare with `==`.

  solo      the tiny_episode scenario for 16 env steps on env 0: a first turn, two steady turns and the `<memory>` restart turn (4 turns).
            Its EOS set ends every turn but the first at its first token, so a second segment follows on env 1: the same scenario without
            an EOS set for 12 env steps (3 turns of 12 tokens) -- decode steps in every turn, and a previous turn for every draft to guess
            from.  Under the call-time modes of switches_ref (m.probe_modes) every solo turn is a group turn of two sequences followed
            by select_sequence(0), or a forced turn on FORCED_IDS
  lockstep  four envs through generate_batch for 8 env steps, no EOS set (2 turns of 12 tokens): the batched decode step stays at B = 4
            (mxfp4_batched, the B >= 4 branch of fp8_gemm), the scheduler's lm_head, rides of the scheduler's drafts
"""
import numpy as np
import torch

import switches_ref as S
from scenarios import SCENARIOS, SEED, eos_ids
from streamvln_amd.agent import BatchedAgents, StreamingAgent
from streamvln_amd.model import GenerateOutput, StreamVLNForCausalLM
from streamvln_amd.synthetic import SyntheticPromptEncoder
from streamvln_amd.synthetic import synthetic_frame as _synthetic_frame

SC = SCENARIOS["tiny_episode"]
# the same prompts and frames, no EOS set: every turn runs to max_new_tokens -- 12, so that a ride (at most 7 draft rows: 8 tokens)
# leaves the verify passes something to do
FREE = dict(SC, eos_mod=0, max_new=12)
N_ENVS = 4
SOLO_STEPS, FREE_STEPS, LOCK_STEPS = 16, 12, 8
_FRAMES = {}


def synthetic_frame(env, step):
    """the scenario's frames, generated once per session (48 of them)"""
    key = (env, step)
    if key not in _FRAMES:
        _FRAMES[key] = _synthetic_frame(env, step)
    return _FRAMES[key]


def make_model(dtype=torch.bfloat16, seed=SEED):
    """`seed` None: no weights loaded yet"""
    m = StreamVLNForCausalLM(SC["cfg"], dtype=dtype, max_envs=N_ENVS, max_frames=3 * N_ENVS, max_positions=2048)
    if seed is not None:
        m.load_synthetic(seed)
    m.model.num_history = SC["num_history"]
    m.sampling_seed = S.SAMPLING[1]
    m.probe_modes = {"group": False, "forced": False}
    return m


def base_state(m):
    """the probe's base: decode graphs on, auto-draft armed (and the engine's default packed decode on bf16)"""
    m.set_decode_graph(True)
    m.set_auto_draft(True)


def bits(a):
    """bit pattern of an fp32 array / tensor as nested lists of ints"""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).tolist()


class _ProbeAgent(StreamingAgent):
    """StreamingAgent whose model turn is, under m.probe_modes, a group turn + select_sequence(0) or a forced turn"""

    def _turn(self, instruction, env_id=None, forced_ids=None):
        m, modes = self.model, self.model.probe_modes
        req = self._build_request(instruction, env_id)
        if modes["forced"]:
            req["forced_ids"] = list(S.FORCED_IDS)
            return self._consume(m.generate(**req))
        if modes["group"]:
            req.update(do_sample=True, temperature=S.SAMPLING[0], num_return_sequences=2)
            out = m.generate(**req)
            rec = {"group_ids": out.sequences.tolist(), "group_lengths": out.sequence_lengths.tolist(),
                   "group_hidden": [bits(m.last_hidden_group(g)) for g in range(2)]}
            if "token_logprobs" in out:
                rec["group_logprobs"] = bits(out.token_logprobs)
            if "allowed_logprobs" in out:
                rec["group_allowed"] = bits(out.allowed_logprobs)
            kv = m.select_sequence(0, env_id=self.env_id)
            n0 = int(out.sequence_lengths[0])
            self.group_log.append(rec)
            res = GenerateOutput(sequences=out.sequences[0:1, :n0].clone(), past_key_values=kv)
            if "token_logprobs" in out:           # the env goes on with sequence 0: its scores are the turn's
                res["token_logprobs"] = out.token_logprobs[0:1, :n0].clone()
            return self._consume(res)
        return self._consume(m.generate(**req))


def _agent(m, env, sampled, cls=StreamingAgent, sc=SC):
    enc = SyntheticPromptEncoder(SC["cfg"], seed=7 + 31 * env, first_len=SC["lens"][0], memory_len=SC["lens"][1], later_len=SC["lens"][2])
    a = cls(m, enc, num_frames=SC["num_frames"], num_future_steps=SC["nfs"], num_history=SC["num_history"], env_id=env, device="cuda",
            max_new_tokens=sc["max_new"], eos_token_ids=eos_ids(sc), preprocess=m.get_vision_tower().image_processor.preprocess_array,
            do_sample=sampled, temperature=S.SAMPLING[0] if sampled else None)
    a.group_log = []
    return a


def _turn_record(out):
    rec = {"ids": out.sequences[0].tolist()}
    for k in ("token_logprobs", "allowed_logprobs", "greedy_logprobs"):
        if k in out:
            rec[k] = bits(out[k])
    if "greedy_ids" in out:
        rec["greedy_ids"] = out["greedy_ids"].tolist()
    return rec


def _stats(m):
    c = dict(zip(("verify_passes", "verify_tokens", "single_steps"), m.draft_stats()))
    c.update(zip(("rides", "ride_tokens", "ride_rows"), m.prefill_draft_stats()))
    c.update(zip(("batch_rides", "batch_ride_tokens", "batch_ride_rows", "iterations", "single_rows"), m.batch_draft_stats()))
    c.update(zip(("cache_hits", "cache_misses"), m.feature_cache_stats()))
    return c


def probe(m, solo=True, lock=True):
    """one run of the fixed workload from reset envs -> a dict of plain Python values (ids, bit patterns, counters)"""
    m.reset(N_ENVS)
    sampled = m._sampling is not None
    if sampled:
        m.set_sampling(*m._sampling)              # the run starts at draw 0 of every env
    if "feature_cache" in getattr(m, "probe_on", ()):
        m.set_feature_cache(S.CACHE_FRAMES)       # ... and with an empty cache (the call drops the entries)
    before = _stats(m)
    run = {"solo": [], "lock": [], "group": []}
    for env, sc, steps in ((0, SC, SOLO_STEPS), (1, FREE, FREE_STEPS)) if solo else ():
        ag = _agent(m, env, sampled, _ProbeAgent, sc)
        seen = 0
        for step in range(steps):
            ag.act(synthetic_frame(env, step))
            if len(ag.turn_log) > seen:
                seen = len(ag.turn_log)
                rec = _turn_record(ag.turn_log[-1]["out"])
                if not m.probe_modes["group"]:    # (a group's rows are in its own record: the tap of the last single-env turn is stale)
                    rec["hidden"] = bits(m.last_hidden())
                rec["env_state"] = list(m.env_state(env))
                run["solo"].append(rec)
        run["group"] += ag.group_log
    if solo:
        assert len(run["solo"]) == 7, len(run["solo"])
    taps = 0
    if solo and "layer_taps" in getattr(m, "probe_on", ()):
        t = m.layer_taps()                        # the last residual row after every layer of the last solo prefill
        taps = int(np.isfinite(t).all() and np.abs(t[-1]).max() > 0)
        run["taps"] = bits(t)
    if lock:
        m.reset(N_ENVS)
        agents = [_agent(m, e, sampled, sc=FREE) for e in range(N_ENVS)]
        group = BatchedAgents(agents)
        for step in range(LOCK_STEPS):
            n0 = len(agents[0].turn_log)
            group.act([synthetic_frame(e, step) for e in range(N_ENVS)])
            if len(agents[0].turn_log) > n0:
                turn = []
                for e, a in enumerate(agents):
                    rec = _turn_record(a.turn_log[-1]["out"])
                    rec["hidden"] = bits(m.last_hidden_batch(e))
                    rec["env_state"] = list(m.env_state(e))
                    turn.append(rec)
                run["lock"].append(turn)
        assert len(run["lock"]) == 2, len(run["lock"])
    after = _stats(m)
    run["stats"] = {k: after[k] - before[k] for k in after}
    run["stats"]["layer_taps"] = taps
    run["stats"]["packed_blocks"] = m.packed_stats()["blocks"]
    return run


def same(a, b):
    """bit equality of two runs, with the first difference named"""
    if a == b:
        return True
    for part in sorted(set(a) | set(b)):
        if a.get(part) != b.get(part):
            raise AssertionError(f"runs differ in {part!r}: {_first_diff(a.get(part), b.get(part))}")
    return False


def _first_diff(x, y, path=""):
    if type(x) is not type(y):
        return f"{path}: {type(x).__name__} vs {type(y).__name__}"
    if isinstance(x, dict):
        for k in sorted(set(x) | set(y)):
            if x.get(k) != y.get(k):
                return _first_diff(x.get(k), y.get(k), f"{path}.{k}")
    if isinstance(x, list):
        if len(x) != len(y):
            return f"{path}: lengths {len(x)} vs {len(y)}"
        for i, (p, q) in enumerate(zip(x, y)):
            if p != q:
                return _first_diff(p, q, f"{path}[{i}]")
    return f"{path}: {x!r} vs {y!r}"


def results_of(run, part="any"):
    """ids and hidden bits of a run's part (what a 'differs' effect compares)"""
    keep = ("ids", "hidden")
    out = []
    if part in ("solo", "any"):
        out.append([{k: t[k] for k in keep if k in t} for t in run["solo"]] + [run["group"]])
    if part in ("lock", "any"):
        out.append([[{k: t[k] for k in keep} for t in turn] for turn in run["lock"]])
    return out
