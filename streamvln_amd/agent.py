"""Host-side streaming agent: the caller of the hot path.

Mirrors the reference's `VLNEvaluator.step` (streamvln/streamvln_agent.py:169-258) and the
identical turn logic inlined in the Habitat loop (streamvln/streamvln_eval.py:290-350):

  * every env step records the preprocessed frame and its time id;
  * a model turn happens when the pending action queue is empty: first turn of a window
    builds the system+instruction prompt (with `<memory>` iff step_id != 0), later turns a
    short "<conjunction> <image>." prompt; `inputs = cat(prev output_ids, new ids)`;
  * at `step_id % num_frames == 0` (step_id != 0) the history frames
    `rgb_list[0 : t0 : t0 // num_history]` are prepended (streamvln_eval.py:313-321);
  * after the step that makes `step_id % num_frames == 0` the window is reset:
    `model.reset_for_env`, `output_ids = None`, `past_key_values = None`, `time_ids = []`
    (streamvln_eval.py:346-350).

The model is anything exposing the reference's operator surface
(`generate(...)`, `reset_for_env(i)`, `get_vision_tower().image_processor`): the HIP-backed
`streamvln_amd.StreamVLNForCausalLM`, or the CPU oracle in tests.
"""
from __future__ import annotations

import itertools
import re
from collections import OrderedDict
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

ACTIONS2IDX = OrderedDict({"STOP": [0], "↑": [1], "←": [2], "→": [3]})   # streamvln_agent.py:52-57

CONJUNCTIONS = [                                                        # streamvln_agent.py:60-68
    "you can see ", "in front of you is ", "there is ", "you can spot ",
    "you are toward the ", "ahead of you is ", "in your sight is ",
]


def parse_actions(output: str) -> List[int]:
    """streamvln_agent.py:101-107 / streamvln_eval.py:382-389."""
    pattern = "|".join(re.escape(a) for a in ACTIONS2IDX)
    matches = re.compile(pattern).findall(output)
    return list(itertools.chain.from_iterable(ACTIONS2IDX[m] for m in matches))


def update_draft_history(history, ids, cap: int = 8):
    """The draft history of an env after a turn that emitted `ids`: the env's distinct turn outputs, most recent first, at most `cap`.
    A pure function: `history` (a list of id lists) is not changed."""
    ids = [int(t) for t in ids]
    if not ids:
        return [list(h) for h in history][:cap]
    return ([ids] + [list(h) for h in history if list(h) != ids])[:cap]


class StreamingAgent:
    """Stateful single-env agent.  `prompt_encoder(first_turn, with_memory, instruction)`
    returns the new turn's token ids (with -200/-300 sentinels); `decode_actions(ids)` turns the
    generated ids into an action list (tokenizer.batch_decode + parse_actions in the reference)."""

    def __init__(self, model, prompt_encoder: Callable, num_frames: int = 32, num_future_steps: int = 4,
                 num_history: Optional[int] = 8, env_id: int = 0, device: str = "cpu",
                 image_dtype: torch.dtype = torch.float32, max_new_tokens: int = 10000,
                 eos_token_ids: Sequence[int] = (), decode_actions: Optional[Callable] = None,
                 preprocess: Optional[Callable] = None, ids_device: Optional[str] = "cpu",
                 do_sample: bool = False, temperature: Optional[float] = None):
        self.model = model
        # sampled turns (model.set_sampling): passed through to generate / submit; the defaults are the reference's greedy call
        self.do_sample, self.temperature = bool(do_sample), temperature
        # act_candidates: let the candidates' first rows ride the prefill pass (model.generate(fold_candidates=True)); set it on the agent
        self.fold_candidates = False
        # multi-draft turns (model.generate(draft_set=...)): G > 0 passes the env's G most recent distinct turn outputs as this turn's
        # guesses; 0 = off.  Set it on the agent; the actions are the plain agent's either way
        self.draft_history = 0
        self.prompt_encoder = prompt_encoder
        self.num_frames, self.num_future_steps, self.num_history = num_frames, num_future_steps, num_history
        self.env_id, self.device, self.image_dtype = env_id, device, image_dtype
        # the reference callers put `inputs` on the model's device (streamvln_eval.py:326); the engine takes token ids from the host, so
        # this agent leaves them there (no H2D + D2H of a few dozen ids per turn; `sequences` come back on the same device).  None = as
        # the reference: `device`.  The model accepts both.
        self.ids_device = device if ids_device is None else ids_device
        self.max_new_tokens, self.eos_token_ids = max_new_tokens, tuple(eos_token_ids)
        self.decode_actions = decode_actions or (lambda ids: [1] * num_future_steps)
        if preprocess is None:
            proc = model.get_vision_tower().image_processor
            preprocess = lambda rgb: proc.preprocess_array(rgb)
        self.preprocess = preprocess
        self.turn_log: List[dict] = []
        self._aux: dict = {}
        self.pending_turn = False          # AsyncBatchedAgents: the model turn of the current env step has returned, the step itself is pending
        self.reset_memory()

    def reset_memory(self):                                   # streamvln_agent.py:87-99
        self.rgb_list: List[torch.Tensor] = []
        self.time_ids: List[int] = []
        self.action_seq: List[int] = []
        self.output_ids = None
        self.past_key_values = None
        self.turn_history: List[List[int]] = []            # the env's distinct turn outputs, most recent first (draft_history)
        # model confidence of the last model turn (model.set_token_scores): log-probability of every emitted id [1, n_new] and their sum,
        # the joint log-probability of the turn; None when the model provides no scores
        self.last_token_logprobs = None
        self.last_turn_logprob = None
        # the model's distribution over the allowed ids for every id of the last model turn (model.set_allowed_tokens with
        # set_token_scores): [1, n_new, n_allowed]; None otherwise
        self.last_allowed_logprobs = None
        # what else the policy considered at every id of the last model turn (model.set_top_logprobs): ids [1, n_new, k] and their
        # log-probabilities [1, n_new, k]; None otherwise
        self.last_top_token_ids = None
        self.last_top_logprobs = None
        # how undecided the policy was at every id of the last model turn (model.set_token_entropy): the entropy, in nats, of the
        # distribution each id was taken from [1, n_new] and their mean over the turn; None when the model provides none
        self.last_token_entropies = None
        self.last_turn_entropy = None
        # the policy's own arg-max at every position of the last FORCED model turn (act(..., forced_ids=...)): [1, n]; None otherwise
        self.last_greedy_ids = None
        # the joint log-probability of every candidate of the last candidates turn (act(..., candidate_ids=...)): [G]; the index taken
        self.last_candidate_logprobs = None
        self.last_candidate_index = None
        self.last_beam_ids = None               # of the last act_beams turn: every hypothesis' ids, in rank order
        self.last_beam_scores = None
        self.last_beam_index = None
        self.step_id = 0
        self.last_image = None
        self.model.reset_for_env(self.env_id)

    # -- one model turn ---------------------------------------------------------------
    def _build_request(self, instruction: str, env_id: Optional[int] = None) -> dict:
        env_id = self.env_id if env_id is None else env_id
        first = self.output_ids is None
        with_memory = first and self.step_id != 0
        ids = torch.tensor([self.prompt_encoder(first, with_memory, instruction)], dtype=torch.long)
        if not first:
            ids = torch.cat([self.output_ids.to(ids.device), ids], dim=1)
        images = self.rgb_list[-1:]
        if self.step_id != 0 and self.step_id % self.num_frames == 0:
            t0 = self.time_ids[0]
            if self.num_history is None:
                hist = slice(0, t0, self.num_future_steps)
            else:
                hist = slice(0, t0, t0 // self.num_history)
            images = self.rgb_list[hist] + images
        V = len(images)
        self._pending = {"step_id": self.step_id, "n_inputs": int(ids.shape[1]), "views": V, "memory": bool(with_memory)}
        # torch.stack(images) of the reference (streamvln_eval.py:313-321); one view: the same values as a view of the frame (no copy kernel)
        self._prime_stack(images[0])
        stacked = images[0].unsqueeze(0) if V == 1 else torch.stack(images)
        aux = self._aux.get(V)
        if aux is None:              # depths / poses / intrinsics are built by the reference callers and ignored by the model
            aux = self._aux[V] = (torch.zeros(1, V, 1, 1), torch.zeros(1, V, 4, 4), torch.zeros(1, V, 4, 4))
        sampling = {"temperature": float(self.temperature)} if self.do_sample and self.temperature is not None else {}
        return {
            **sampling,
            "images": stacked.unsqueeze(0).to(self.device).to(self.image_dtype),
            "depths": aux[0], "poses": aux[1], "intrinsics": aux[2],
            "inputs": ids.to(self.ids_device), "env_id": env_id, "time_ids": [list(self.time_ids)], "task_type": [0],
            "do_sample": self.do_sample, "num_beams": 1, "max_new_tokens": self.max_new_tokens, "use_cache": True,
            "return_dict_in_generate": True, "past_key_values": self.past_key_values, "eos_token_ids": self.eos_token_ids,
        }

    def _prime_stack(self, frame):
        """torch loads the copy kernel of an N-input torch.stack at its first use: the 9-view stack of the first window restart of a process
        took 8.5-18 ms (0.1 ms at every later restart).  The first turn of an agent therefore runs that stack once on its own frame, so
        the one-time cost sits at the start of the first episode and not in the first restart turn."""
        if not getattr(self, "_stack_primed", False):
            self._stack_primed = True
            if frame.is_cuda and self.num_history:
                torch.stack([frame] * (self.num_history + 1))

    def _consume(self, out):
        self.output_ids = out.sequences
        self.past_key_values = out.past_key_values
        lp = out.get("token_logprobs") if isinstance(out, dict) else getattr(out, "token_logprobs", None)
        self.last_token_logprobs = lp
        self.last_turn_logprob = None if lp is None else float(lp.sum())
        self.last_allowed_logprobs = out.get("allowed_logprobs") if isinstance(out, dict) else getattr(out, "allowed_logprobs", None)
        self.last_greedy_ids = out.get("greedy_ids") if isinstance(out, dict) else getattr(out, "greedy_ids", None)
        self.last_top_token_ids = out.get("top_token_ids") if isinstance(out, dict) else getattr(out, "top_token_ids", None)
        self.last_top_logprobs = out.get("top_logprobs") if isinstance(out, dict) else getattr(out, "top_logprobs", None)
        ent = out.get("token_entropies") if isinstance(out, dict) else getattr(out, "token_entropies", None)
        self.last_token_entropies = ent
        self.last_turn_entropy = None if ent is None else float(ent.mean())
        self.turn_log.append(dict(self._pending, out=out))
        actions = list(self.decode_actions(out.sequences))
        return actions if len(actions) else [0]               # streamvln_eval.py:340-341

    def _turn(self, instruction: str, env_id: Optional[int] = None, forced_ids=None):
        req = self._build_request(instruction, env_id)
        if forced_ids is not None:
            req["forced_ids"] = forced_ids
        G = int(getattr(self, "draft_history", 0) or 0)
        if G <= 0:
            return self._consume(self.model.generate(**req))
        if forced_ids is None:
            req["draft_set"] = [list(h) for h in self.turn_history[:G]]
        out = self.model.generate(**req)
        self.turn_history = update_draft_history(self.turn_history, out.sequences.reshape(-1).tolist())
        return self._consume(out)

    def _turn_candidates(self, instruction: str, candidate_ids, select=None, env_id: Optional[int] = None):
        """the model turn as a candidates call (model.generate(candidate_ids=...)): every candidate is scored against one prefill, the
        env goes on with candidate `select` (default: the largest joint log-probability) as a forced turn on it would"""
        req = self._build_request(instruction, env_id)
        req["candidate_ids"] = candidate_ids
        if getattr(self, "fold_candidates", False):
            req["fold_candidates"] = True
        req.pop("do_sample", None)             # (no token is drawn; the sampling switch of the model stays as it is)
        req.pop("temperature", None)
        out = self.model.generate(**req)
        joint = out.token_logprobs.sum(1)
        G = int(joint.numel())
        index = int(joint.argmax()) if select is None else int(select)
        if not (0 <= index < G):
            index_err = ValueError(f"select={select!r}: the call scored {G} candidates")
            self.model.select_sequence(0, req["env_id"])      # the env must not stay blocked by the pending group
            raise index_err
        kv = self.model.select_sequence(index, req["env_id"])
        n = int(out.sequence_lengths[index])
        self.last_candidate_logprobs = joint
        self.last_candidate_index = index
        one = type(out)(sequences=out.sequences[index:index + 1, :n], past_key_values=kv)
        one["token_logprobs"] = out.token_logprobs[index:index + 1, :n]
        one["greedy_ids"] = out.greedy_ids[index:index + 1, :n]
        one["greedy_logprobs"] = out.greedy_logprobs[index:index + 1, :n]
        alp = out.get("allowed_logprobs") if isinstance(out, dict) else getattr(out, "allowed_logprobs", None)
        if alp is not None:
            one["allowed_logprobs"] = alp[index:index + 1, :n]
            one["allowed_token_ids"] = out["allowed_token_ids"]
        one["candidates"] = out
        return self._consume(one)

    def _turn_beams(self, instruction: str, beam_width: int, select=None, env_id: Optional[int] = None):
        """the model turn as a beam turn (model.generate(beam_width=W)): the env goes on with hypothesis `select` (default: rank 0)"""
        req = self._build_request(instruction, env_id)
        req["beam_width"] = int(beam_width)
        req.pop("do_sample", None)              # (beams are greedy; the sampling switch of the model stays as it is)
        req.pop("temperature", None)
        out = self.model.generate(**req)
        n_hyp = int(out.sequences.shape[0])
        index = 0 if select is None else int(select)
        if not (0 <= index < n_hyp):
            index_err = ValueError(f"select={select!r}: the beam turn returned {n_hyp} hypotheses")
            self.model.select_sequence(0, req["env_id"])      # the env must not stay blocked by the pending group
            raise index_err
        kv = self.model.select_sequence(index, req["env_id"])
        n = int(out.sequence_lengths[index])
        self.last_beam_ids = [out.sequences[g, : int(out.sequence_lengths[g])].tolist() for g in range(n_hyp)]
        self.last_beam_scores = out.sequences_scores
        self.last_beam_index = index
        one = type(out)(sequences=out.sequences[index:index + 1, :n], past_key_values=kv)
        one["token_logprobs"] = out.token_logprobs[index:index + 1, :n]
        one["beams"] = out
        return self._consume(one)

    # -- split form of act() used by BatchedAgents: observe -> (maybe) request -> finish ----------
    def observe(self, rgb):
        self.time_ids.append(self.step_id)
        self.rgb_list.append(self.preprocess(rgb))
        return len(self.action_seq) == 0                      # True: this env needs a model turn now

    def finish_step(self) -> int:
        action = self.action_seq.pop(0)
        self.step_id += 1
        if self.step_id % self.num_frames == 0:
            self.model.reset_for_env(self.env_id)
            self.output_ids = None
            self.past_key_values = None
            self.time_ids = []
        return action

    # -- eval-loop flavour: one env step, returns the action taken -------------------
    def act(self, rgb: np.ndarray, instruction: str = "", forced_ids=None) -> int:
        """One environment step of the Habitat loop (streamvln_eval.py:247-350).
        forced_ids (optional): the model turn that runs at this step is a forced turn on these ids (model.generate(forced_ids=...)): the
        env goes on with them, `last_token_logprobs` / `last_turn_logprob` are the policy's log-probabilities of them and
        `last_greedy_ids` its own picks.  Raises, before anything changes, when no model turn runs at this step."""
        if forced_ids is not None and len(self.action_seq) != 0:
            raise ValueError(f"forced_ids given at step {self.step_id}, but no model turn runs there: {len(self.action_seq)} actions of the last turn are still queued")
        if self.observe(rgb):
            self.action_seq = self._turn(instruction) if forced_ids is None else self._turn(instruction, forced_ids=forced_ids)
        return self.finish_step()

    def act_candidates(self, rgb: np.ndarray, instruction: str = "", candidate_ids=None, select=None) -> int:
        """`act` whose model turn scores candidates: the 2 .. 8 id lists of candidate_ids are scored against one prefill
        (model.generate(candidate_ids=...)) and the env goes on with candidate `select` (default: the largest joint log-probability), as
        a forced turn on it would.  `last_candidate_logprobs` keeps every candidate's joint log-probability, `last_candidate_index` the
        one taken, and the `last_*` fields of a forced turn describe it.  Raises, before anything changes, when no model turn runs at
        this step.  (A method of its own: `act` keeps its argument list.)"""
        if candidate_ids is None:
            raise ValueError("act_candidates needs candidate_ids")
        if len(self.action_seq) != 0:
            raise ValueError(f"candidate_ids given at step {self.step_id}, but no model turn runs there: {len(self.action_seq)} actions of the last turn are still queued")
        if select is not None and not (0 <= int(select) < len(candidate_ids)):
            raise ValueError(f"select={select!r}: {len(candidate_ids)} candidates were given")
        if self.observe(rgb):
            self.action_seq = self._turn_candidates(instruction, candidate_ids, select)
        return self.finish_step()

    def act_beams(self, rgb: np.ndarray, instruction: str = "", beam_width: int = 4, select=None) -> int:
        """`act` whose model turn is a beam turn (model.generate(beam_width=W)): the env goes on with hypothesis `select` (default: rank
        0, the most probable).  `last_beam_ids` / `last_beam_scores` keep every hypothesis in rank order, `last_beam_index` the one
        taken.  Raises, before anything changes, when no model turn runs at this step.  (`act` keeps its argument list.)"""
        if not (1 <= int(beam_width) <= 8):
            raise ValueError(f"beam_width={beam_width!r}: a beam turn keeps 1 .. 8 hypotheses")
        if len(self.action_seq) != 0:
            raise ValueError(f"beam_width given at step {self.step_id}, but no model turn runs there: {len(self.action_seq)} actions of the last turn are still queued")
        if select is not None and not (0 <= int(select) < int(beam_width)):
            raise ValueError(f"select={select!r}: at most {int(beam_width)} hypotheses are returned")
        if self.observe(rgb):
            self.action_seq = self._turn_beams(instruction, beam_width, select)
        return self.finish_step()

    # -- real-world flavour ------------------------------------------------------------
    def step(self, idx: int, rgb: np.ndarray, instruction_text: str = "", run_model: bool = False):
        """`VLNEvaluator.step` (streamvln_agent.py:169-258).  The caller increments
        `self.step_id` (http_realworld_server.py:112)."""
        if run_model:
            self.last_image = self.preprocess(rgb)
        image = self.last_image
        self.time_ids.append(self.step_id)
        self.rgb_list.append(image)
        if not run_model:
            if (self.step_id + 1) % self.num_frames == 0:
                self.model.reset_for_env(idx)
                self.output_ids = None
                self.past_key_values = None
                self.time_ids = []
            return None, 0, None
        actions = self._turn(instruction_text, idx)
        return actions, 0.0, self.turn_log[-1]["out"]


def _forced_map(forced_ids, n_agents) -> dict:
    """`forced_ids` of BatchedAgents.act / AsyncBatchedAgents.tick -- a per-agent list (None = a plain turn) or a dict {agent index: ids}
    -- as {agent index: ids}"""
    if forced_ids is None:
        return {}
    if isinstance(forced_ids, dict):
        named = {int(i): f for i, f in forced_ids.items() if f is not None}
    else:
        if len(forced_ids) != n_agents:
            raise ValueError(f"forced_ids holds {len(forced_ids)} entries for {n_agents} agents")
        named = {i: f for i, f in enumerate(forced_ids) if f is not None}
    for i in named:
        if not (0 <= i < n_agents):
            raise ValueError(f"forced_ids names agent {i}: there are {n_agents}")
    return named


class BatchedAgents:
    """Several envs on one GPU stepped in lockstep (BASELINE configs[4]: DAgger-style concurrent envs; the reference
    runs one env per process, streamvln_dagger.py:299).  Each env keeps its own StreamingAgent state; the turns that fall
    due at the same step are sent to the model together (`generate_batch`)."""

    def __init__(self, agents):
        self.agents = list(agents)
        self.model = self.agents[0].model

    def act(self, rgbs, instructions=None, forced_ids=None):
        """forced_ids (optional; a per-agent list or a dict {agent index: ids}): the agents named there run the model turn of this step
        as a forced job of the scheduler (model.generate_batch_forced) and get `last_greedy_ids`, `last_token_logprobs` and
        `last_turn_logprob`, as StreamingAgent.act(forced_ids=...) gives them.  Raises ValueError, before anything changes, where no
        model turn is due for a named agent.  None: the call of before, generate_batch."""
        instructions = instructions or [""] * len(self.agents)
        forced = _forced_map(forced_ids, len(self.agents))
        for i in forced:
            if len(self.agents[i].action_seq) != 0:
                raise ValueError(f"forced_ids given for agent {i} at step {self.agents[i].step_id}, but no model turn runs there: "
                                 f"{len(self.agents[i].action_seq)} actions of the last turn are still queued")
        due = [a for a, rgb in zip(self.agents, rgbs) if a.observe(rgb)]
        if due and forced_ids is not None:
            reqs = []
            for a in due:
                i = self.agents.index(a)
                reqs.append(a._build_request(instructions[i]))
                if i in forced:
                    reqs[-1]["forced_ids"] = forced[i]
            outs = self.model.generate_batch_forced(reqs)
            for a, out in zip(due, outs):
                a.action_seq = a._consume(out)
        elif due:
            reqs = [a._build_request(instructions[self.agents.index(a)]) for a in due]
            shared = {k: reqs[0][k] for k in ("max_new_tokens", "eos_token_ids")}
            outs = self.model.generate_batch(reqs, **shared)
            for a, out in zip(due, outs):
                a.action_seq = a._consume(out)
        return [a.finish_step() for a in self.agents]


class AsyncBatchedAgents:
    """Several envs on one GPU whose model turns fall due at DIFFERENT times (the DAgger collector's situation: each env mixes
    expert steps, which need no model call, with model steps; streamvln_dagger.py:232-313).  `tick(rgbs)` advances every env that
    is not waiting for the model by one env step (an env whose action queue is empty submits its turn instead) and then runs ONE
    scheduler iteration (`model.step_batch`): envs that submitted in earlier ticks are decoding while new ones prefill, all in the
    same pass over the weights.  Returns {agent index: action taken} for the envs that stepped in this tick."""

    def __init__(self, agents, on_result=None):
        self.agents = list(agents)
        self.model = self.agents[0].model
        self.waiting = {}                                 # scheduler slot -> agent index
        self.on_result = on_result                        # optional callback(agent index, ticket, GenerateOutput)
        self.stats = {"iterations": 0, "mixed_iterations": 0, "max_in_flight": 0}

    def tick(self, rgbs, instructions=None, active=None, forced_ids=None):
        """`rgbs[i]`: the frame of agent i's current env step (ignored for agents that are waiting); `active`: indices allowed to
        step in this tick (default: all).  forced_ids (optional; a per-agent list or a dict {agent index: ids}): the agents named
        there submit the model turn of this tick as a forced job (model.submit_forced), which finishes in this tick's iteration.
        Raises ValueError, before anything changes, where a named agent submits no turn in this tick."""
        instructions = instructions or [""] * len(self.agents)
        acted = {}
        busy = set(self.waiting.values())
        forced = _forced_map(forced_ids, len(self.agents))
        for i in forced:
            a = self.agents[i]
            if i in busy or (active is not None and i not in active) or a.pending_turn or len(a.action_seq) != 0:
                raise ValueError(f"forced_ids given for agent {i} at step {a.step_id}, but it submits no model turn in this tick")
        for i, a in enumerate(self.agents):
            if i in busy or (active is not None and i not in active):
                continue
            if a.pending_turn:                            # its turn came back in an earlier tick: take the env step now
                a.pending_turn = False
                acted[i] = a.finish_step()
                continue
            if a.observe(rgbs[i]):
                if i in forced:
                    t = self.model.submit_forced(**a._build_request(instructions[i]), forced_ids=forced[i])
                else:
                    t = self.model.submit(**a._build_request(instructions[i]))
                self.waiting[t.slot] = i
            else:
                acted[i] = a.finish_step()
        if not self.waiting:
            return acted
        n_new = len(self.waiting) - len(busy)
        self.stats["iterations"] += 1
        self.stats["mixed_iterations"] += int(n_new > 0 and len(busy) > 0)      # new turns prefill while older ones decode
        self.stats["max_in_flight"] = max(self.stats["max_in_flight"], len(self.waiting))
        done, _ = self.model.step_batch()
        for ticket, out in done:
            i = self.waiting.pop(ticket.slot)
            a = self.agents[i]
            a.action_seq = a._consume(out)
            a.pending_turn = True
            if self.on_result is not None:
                self.on_result(i, ticket, out)
        return acted
