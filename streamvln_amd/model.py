"""Host-side mirror of the reference's operator surface for the streaming path.

`StreamVLNForCausalLM` here keeps the names, argument meaning and error behaviour of
streamvln/model/stream_video_vln.py (`generate`, `reset`, `reset_for_env`, `get_vision_tower`,
`get_model`, `.model.num_history`) so `VLNEvaluator.step` / the Habitat eval loop
(streamvln/streamvln_agent.py:169-258, streamvln/streamvln_eval.py:290-350) call it unchanged.
All arithmetic happens in the HIP engine behind include/streamvln_hip.h; PyTorch is used only
for the caller's tensors (device memory in / token ids out).
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .config import CONFIGS, StreamVLNConfig
from .weights import tensor_seed, tensor_specs


def _check(rc):
    _lib.check(rc)


class SigLipImageProcessor:
    """llava/model/multimodal_encoder/siglip_encoder.py:34-67: bicubic resize to 384x384 (aspect not preserved), x/255,
    (x-0.5)/0.5, channels first.

    Two backends with bit-identical results (tests/test_preprocess.py):
      * "hip"  -- the processor a model hands out (`model.get_vision_tower().image_processor`): upload of the uint8 frame +
                  one HIP kernel reproducing Pillow's fixed-point bicubic (csrc/preprocess.hip); returns a CUDA tensor, so the
                  harness's `dict_to_cuda` is a no-op.  No fallback: it raises without the engine / a GPU.
      * "pil"  -- stand-alone `SigLipImageProcessor()`: Pillow on the host, exactly what the reference runs (host utility
                  for callers without an engine, and the comparison leg of the tests)."""

    def __init__(self, size=(384, 384), engine=None, device_index: int = 0):
        self.image_mean, self.image_std = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
        self.size = size
        self.rescale_factor = 1 / 255
        self.crop_size = {"height": size[0], "width": size[1]}
        self._engine = engine                 # (lib, handle) of the owning model
        self.device_index = device_index
        self.backend = "hip" if engine is not None else "pil"
        self._ext_stream = None               # the engine's HIP stream as a torch stream (lazily wrapped)

    # -- host path (Pillow) ----------------------------------------------------------------------------
    def _pil(self, rgb) -> torch.Tensor:
        from PIL import Image
        img = rgb if isinstance(rgb, Image.Image) else Image.fromarray(np.asarray(rgb, dtype=np.uint8))
        img = img.convert("RGB").resize((self.size[1], self.size[0]), resample=Image.BICUBIC)
        a = (np.asarray(img).astype(np.float64) * self.rescale_factor).astype(np.float32)
        a = (a - np.float32(0.5)) / np.float32(0.5)
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))

    # -- GPU path --------------------------------------------------------------------------------------
    @staticmethod
    def _as_u8(rgb) -> np.ndarray:
        if not isinstance(rgb, np.ndarray):                       # PIL image (the reference callers pass Image.fromarray(rgb))
            rgb = np.asarray(rgb.convert("RGB"))
        a = np.ascontiguousarray(rgb, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"expected an RGB frame [H, W, 3], got shape {a.shape}")
        return a

    def _hip(self, frames) -> torch.Tensor:
        """frames: list of uint8 [H,W,3] arrays of one geometry -> CUDA fp32 [n,3,S,S]"""
        if self._engine is None:
            raise RuntimeError("the model that owns this image processor was closed")
        lib, h = self._engine
        n, (H, W, _) = len(frames), frames[0].shape
        buf = frames[0] if n == 1 else np.ascontiguousarray(np.stack(frames))
        dev = torch.device("cuda", self.device_index)
        out = torch.empty((n, 3, self.size[0], self.size[1]), dtype=torch.float32, device=dev)
        # the engine writes `out` on its own stream: order the two streams on the device instead of stalling the host twice per frame
        # (the call returns once the frame bytes are staged; svln_encode_frames on the same engine is ordered behind the kernel)
        ext, cur = self._engine_stream(dev), torch.cuda.current_stream(dev)
        same = cur.cuda_stream == ext.cuda_stream          # the caller runs torch on the engine's stream (model.torch_stream): already ordered
        if not same:
            ext.wait_stream(cur)
        _check(lib.svln_preprocess_frames_enqueue(h, buf.ctypes.data, n, H, W, 0, out.data_ptr()))
        if not same:
            cur.wait_stream(ext)  # torch work on `out` (and any later reuse of its memory, which stays on this stream) follows the kernel
        return out

    def _engine_stream(self, dev):
        if self._ext_stream is None:
            lib, h = self._engine
            sp = C.c_void_p()
            _check(lib.svln_engine_stream(h, C.byref(sp)))
            self._ext_stream = torch.cuda.ExternalStream(sp.value, device=dev)
        return self._ext_stream

    def preprocess_array(self, rgb) -> torch.Tensor:
        if self.backend == "pil":
            return self._pil(rgb)
        return self._hip([self._as_u8(rgb)])[0]

    def preprocess(self, images, return_tensors="pt"):
        from PIL import Image
        if isinstance(images, Image.Image) or (isinstance(images, np.ndarray) and images.ndim == 3):
            images = [images]
        if self.backend == "pil":
            vals = [self._pil(im) for im in images]
        else:
            frames = [self._as_u8(im) for im in images]
            if len({f.shape for f in frames}) == 1:
                vals = list(self._hip(frames))                    # one upload + one launch for the batch
            else:
                vals = [self._hip([f])[0] for f in frames]
        if return_tensors == "pt":
            return {"pixel_values": torch.stack(vals)}
        return {"pixel_values": [v.cpu().numpy() for v in vals]}


class _VisionTower:
    def __init__(self, cfg: StreamVLNConfig, engine=None, device_index: int = 0):
        self.config = SimpleNamespace(hidden_size=cfg.v_hidden, image_size=cfg.v_image, patch_size=cfg.v_patch)
        self.image_processor = SigLipImageProcessor((cfg.v_image, cfg.v_image), engine=engine, device_index=device_index)
        self.is_loaded = True

    @property
    def num_patches_per_side(self):
        return self.config.image_size // self.config.patch_size

    @property
    def num_patches(self):
        return self.num_patches_per_side ** 2

    @property
    def hidden_size(self):
        return self.config.hidden_size


class KVHandle:
    """Opaque `past_key_values` handle: the KV pages live in the engine, keyed by env."""

    def __init__(self, env_id: int, epoch: int, length: int):
        self.env_id, self.epoch, self.length = env_id, epoch, length

    def get_seq_length(self):
        return self.length

    def __len__(self):
        return self.length


class GenerateOutput(dict):
    """`return_dict_in_generate=True` result: `.sequences` (new tokens only, EOS included) and
    `.past_key_values` (streamvln_eval.py:334-335).  `.top_token_ids` / `.top_logprobs` (set_top_logprobs) and `.token_entropies`
    (set_token_entropy) read as None while their switch is off, `.draft_index` / `.draft_tokens` on a turn without draft_set; like every optional entry they are keys only of a result that carries them."""

    _OPTIONAL = ("top_token_ids", "top_logprobs", "token_entropies", "draft_index", "draft_tokens")

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            if k in GenerateOutput._OPTIONAL:
                return None
            raise AttributeError(k) from e


class StreamVLNForCausalLM:
    def __init__(self, config: StreamVLNConfig, dtype: torch.dtype = torch.bfloat16, device: int = 0, max_envs: int = 1,
                 max_frames: int = 9, max_positions: Optional[int] = None):
        lib = _lib.load()
        self.cfg = config
        self.dtype = dtype
        self.device_index = device
        c = _lib.SvlnConfig(
            v_hidden=config.v_hidden, v_inter=config.v_inter, v_heads=config.v_heads, v_layers=config.v_layers,
            v_patch=config.v_patch, v_image=config.v_image, v_eps=config.v_eps,
            hidden=config.hidden, layers=config.layers, q_heads=config.q_heads, kv_heads=config.kv_heads,
            head_dim=config.head_dim, inter=config.inter, vocab=config.vocab, rope_theta=config.rope_theta,
            rms_eps=config.rms_eps, max_positions=max_positions or config.max_positions, max_envs=max_envs,
            max_frames=max_frames, dtype=_lib.SVLN_F32 if dtype == torch.float32 else _lib.SVLN_BF16)
        h = C.c_void_p()
        _check(lib.svln_create(C.byref(c), device, C.byref(h)))
        self._lib, self._h = lib, h
        self.max_envs, self.max_frames = max_envs, max_frames
        self._tower = _VisionTower(config, engine=(lib, h), device_index=device)
        # `.model` = StreamVLNModel in the reference; callers set `.model.num_history` (streamvln_eval.py:531)
        self.model = SimpleNamespace(num_history=None, get_vision_tower=lambda: self._tower)
        # tokenizer_model_max_length: read at every call like the reference does (stream_video_vln.py:241-244); None = no truncation
        self.config = SimpleNamespace(mm_spatial_pool_mode="bilinear", hidden_size=config.hidden, vocab_size=config.vocab,
                                      tokenizer_model_max_length=None)
        # Qwen2-7B-Instruct <|im_end|>, <|endoftext|>; repetition_penalty as transformers' GenerationConfig defaults it
        self.generation_config = SimpleNamespace(eos_token_id=[151645, 151643], repetition_penalty=1.0)
        self._row_limit, self._rep_penalty = 0, 1.0           # what the engine currently holds
        self._tickets: Dict[int, tuple] = {}
        self._forced_tickets: Dict[int, np.ndarray] = {}           # slot -> forced ids of the tickets that submit_forced issued
        self._auto_draft = False                                   # set_auto_draft: guess that a turn repeats the env's previous one
        self._last_out: Dict[int, torch.Tensor] = {}
        self._token_scores = False                                 # set_token_scores: results carry token_logprobs
        self.top_logprobs_k = 0                                    # set_top_logprobs: results carry the k best ids per token
        self._token_entropy = False                                # set_token_entropy: results carry token_entropies
        self.allowed_token_ids = None                              # set_allowed_tokens: the list in force (tuple), None when off
        self._sampling = None                                      # set_sampling: None (greedy) or (temperature, seed) the engine holds
        self.sampling_seed = 0                                     # seed of the noise of generate(do_sample=True) (see set_sampling)
        self.sampling_truncation = None                            # None or (top_k, top_p): applied whenever sampling is switched on (see set_sampling_truncation)
        self._batch_draft = False                                  # set_batch_draft: the scheduler consumes drafts
        self._group_pending: Dict[int, int] = {}                   # env_id -> sequences of its group turn awaiting select_sequence
        self.reset(max_envs)

    # ---- construction -------------------------------------------------------------------------
    @classmethod
    def from_config(cls, config, seed: Optional[int] = None, **kw):
        if isinstance(config, str):
            config = CONFIGS[config]
        m = cls(config, **kw)
        if seed is not None:
            m.load_synthetic(seed)
        return m

    @classmethod
    def from_pretrained(cls, path, config=None, torch_dtype=torch.bfloat16, attn_implementation=None, low_cpu_mem_usage=False,
                        device: int = 0, **kw):
        """Checkpoint ingestion (HF safetensors layout).  No checkpoint exists offline."""
        import glob
        import os
        files = sorted(glob.glob(os.path.join(str(path), "*.safetensors")))
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {path}")
        from safetensors import safe_open
        from .config import TRUE, config_from_hf
        import json
        # dims: an explicit StreamVLNConfig, else the harness's HF config object, else the checkpoint's config.json, else Qwen2-7B
        if isinstance(config, StreamVLNConfig):
            cfg = config
        elif config is not None:
            cfg = config_from_hf(config)
        elif os.path.exists(os.path.join(str(path), "config.json")):
            cfg = config_from_hf(json.load(open(os.path.join(str(path), "config.json"))))
        else:
            cfg = TRUE
        m = cls(cfg, dtype=torch_dtype, device=device, **kw)
        hf = config if config is not None and not isinstance(config, StreamVLNConfig) else None
        if hf is None and os.path.exists(os.path.join(str(path), "config.json")):
            hf = json.load(open(os.path.join(str(path), "config.json")))
        if hf is not None:
            tml = hf.get("tokenizer_model_max_length") if isinstance(hf, dict) else getattr(hf, "tokenizer_model_max_length", None)
            m.config.tokenizer_model_max_length = None if tml is None else int(tml)
        gen = os.path.join(str(path), "generation_config.json")
        if os.path.exists(gen):                                   # the checkpoint's generation defaults
            m.apply_generation_config(json.load(open(gen)))
        for f in files:
            with safe_open(f, framework="pt") as sf:
                for name in sf.keys():
                    if name in m.tensor_names():
                        m.set_tensor(name, sf.get_tensor(name))
        m.check_weights()
        return m

    #: generation_config.json keys that would change what `generate(do_sample=False, num_beams=1, max_new_tokens=...)` returns in
    #: transformers 4.45.1 and that the engine does not implement -> an error at load time, never a silently different answer.
    #: (value = the neutral setting.)  Sampling knobs (temperature / top_k / top_p / typical_p ...) are inert under the harness's
    #: explicit do_sample=False and are ignored, as HF itself does (with a warning).
    _UNSUPPORTED_GENERATION_KEYS = {
        "no_repeat_ngram_size": 0, "encoder_repetition_penalty": 1.0, "encoder_no_repeat_ngram_size": 0, "bad_words_ids": None,
        "min_length": 0, "min_new_tokens": None, "forced_bos_token_id": None, "forced_eos_token_id": None, "suppress_tokens": None,
        "begin_suppress_tokens": None, "sequence_bias": None, "penalty_alpha": None, "guidance_scale": None, "num_beam_groups": 1,
        "diversity_penalty": 0.0, "length_penalty": 1.0, "exponential_decay_length_penalty": None, "renormalize_logits": False,
        "remove_invalid_values": False, "forced_decoder_ids": None, "constraints": None, "force_words_ids": None,
        "prompt_lookup_num_tokens": None, "assistant_model": None, "dola_layers": None, "watermarking_config": None,
    }

    def apply_generation_config(self, gen: dict):
        """A checkpoint's generation_config.json -> the stop ids and the repetition penalty of the greedy loop; any other key that
        changes greedy decoding raises."""
        eos = gen.get("eos_token_id")
        if eos is not None:
            self.generation_config.eos_token_id = list(eos) if isinstance(eos, (list, tuple)) else [int(eos)]
        rp = gen.get("repetition_penalty")
        if rp is not None:
            if not float(rp) > 0:
                raise ValueError(f"generation_config.repetition_penalty must be > 0, got {rp}")
            self.generation_config.repetition_penalty = float(rp)
        if gen.get("temperature") is not None:                   # read by do_sample=True calls only (inert under the greedy call)
            self.generation_config.temperature = float(gen["temperature"])
        bad = []
        for k, neutral in self._UNSUPPORTED_GENERATION_KEYS.items():
            v = gen.get(k, neutral)
            if v is None or v == neutral or (isinstance(v, (list, dict)) and not v):
                continue
            if k == "length_penalty" and int(gen.get("num_beams", 1)) == 1:
                continue                                          # beam-search only
            bad.append(f"{k}={v!r}")
        if bad:
            raise NotImplementedError("generation_config.json changes greedy decoding in ways the HIP path does not implement: "
                                      + ", ".join(bad))

    def _sync_call_config(self):
        """config.tokenizer_model_max_length and generation_config.repetition_penalty are plain attributes the caller may change
        between calls (the reference reads them at call time): push them to the engine when they differ from what it holds.
        The row limit has no in-flight restriction and is pushed at every call; the penalty cannot change while scheduler turns are
        in flight (the engine refuses it), so a changed value raises here instead of being ignored."""
        tml = getattr(self.config, "tokenizer_model_max_length", None)
        if tml is not None and int(tml) < 1:
            # the reference would splice `new_input_embeds[:0]` -- an empty turn -- and fail further down (stream_video_vln.py:241-244);
            # the engine's 0 means "no truncation", so 0 must never reach it
            raise ValueError(f"config.tokenizer_model_max_length must be None (no truncation) or >= 1, got {tml!r}")
        lim = 0 if tml is None else int(tml)
        if lim != self._row_limit:
            _check(self._lib.svln_set_turn_row_limit(self._h, lim))
            self._row_limit = lim
        rp = float(getattr(self.generation_config, "repetition_penalty", 1.0) or 1.0)
        if rp != self._rep_penalty:
            if self._tickets:
                raise RuntimeError("generation_config.repetition_penalty changed while turns are in flight: collect or cancel them first")
            _check(self._lib.svln_set_repetition_penalty(self._h, rp))
            self._rep_penalty = rp

    def tensor_names(self):
        return {s.name for s in tensor_specs(self.cfg)}

    def load_synthetic(self, seed: int):
        """Seeded random-init weights generated on the device (streamvln_amd/weights.py)."""
        for s in tensor_specs(self.cfg):
            _check(self._lib.svln_synth_tensor(self._h, s.name.encode(), tensor_seed(seed, s.name), s.half_width, s.base))
        self.check_weights()
        return self

    def set_tensor(self, name: str, value):
        """Write one canonical tensor (host array / tensor, or a device tensor; fp32 or bf16).  May come at any time between turns: the
        packed, e4m3 and MXFP4 copies of the matrix follow it and a vision-tower / projector write empties the feature cache
        (svln_set_tensor); envs hold rows and KV computed with the old weights -- reset them.  Refused by name while scheduler turns are
        in flight or a group turn is pending."""
        if isinstance(value, torch.Tensor):
            t = value.detach()
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            t = t.contiguous()
            dt = _lib.SVLN_F32 if t.dtype == torch.float32 else _lib.SVLN_BF16
            if t.is_cuda:
                torch.cuda.synchronize()
            _check(self._lib.svln_set_tensor(self._h, name.encode(), C.c_void_p(t.data_ptr()), dt, t.numel(), int(t.is_cuda)))
        else:
            a = np.ascontiguousarray(value, dtype=np.float32)
            _check(self._lib.svln_set_tensor(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), _lib.SVLN_F32, a.size, 0))

    def load_state_dict(self, sd: Dict[str, object]):
        for k, v in sd.items():
            self.set_tensor(k, v)
        self.check_weights()
        return self

    def check_weights(self):
        _check(self._lib.svln_weights_ready(self._h))

    def get_tensor(self, name: str) -> np.ndarray:
        spec = {s.name: s for s in tensor_specs(self.cfg)}[name]
        out = np.empty(spec.numel, dtype=np.float32)
        _check(self._lib.svln_get_tensor_f32(self._h, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out.reshape(spec.shape)

    # ---- nn.Module-flavoured no-ops the harness calls (streamvln_eval.py:531-539) -----------------
    def requires_grad_(self, flag=False):
        return self

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def get_model(self):
        return self.model

    def get_vision_tower(self):
        return self._tower

    def _order_engine_after(self, pix):
        """The engine's stream is about to read `pix`: order it behind the torch work that produced the tensor (on the device, no host
        stall).  Nothing to do when the caller runs torch on the engine's stream (`torch_stream`)."""
        ext, cur = self._tower.image_processor._engine_stream(pix.device), torch.cuda.current_stream(pix.device)
        if cur.cuda_stream != ext.cuda_stream:
            ext.wait_stream(cur)

    def _order_torch_after(self, pix):
        """... and the caller's stream behind that read, so that freeing `pix` cannot hand its memory to later torch work too early."""
        ext, cur = self._tower.image_processor._engine_stream(pix.device), torch.cuda.current_stream(pix.device)
        if cur.cuda_stream != ext.cuda_stream:
            cur.wait_stream(ext)

    @property
    def torch_stream(self):
        """The engine's HIP stream as a torch stream.  A harness that wraps its loop in `with torch.cuda.stream(model.torch_stream):`
        runs its own tensor ops (stack / to / cat) on the stream the engine uses, so no cross-stream ordering (two event records and
        two stream waits per frame and per turn) is needed; any other stream works too, at that cost."""
        return self._tower.image_processor._engine_stream(self.device)

    def frame_ring(self, slots: int, height: int, width: int) -> np.ndarray:
        """Engine-owned pinned frame ring (svln_frame_ring) as a uint8 array [slots, height, width, 3].  Frames written into a slot and
        handed to the image processor as that slot's view (`ring[k]`) are read by the GPU in place: no host-side staging copy.  Rewrite
        a slot only after `frame_ring_wait(k)` (or any call that synchronises, e.g. `generate`'s return for frames preprocessed before)."""
        base, stride = C.c_void_p(), C.c_int64()
        _check(self._lib.svln_frame_ring(self._h, int(slots), int(height), int(width), C.byref(base), C.byref(stride)))
        raw = (C.c_uint8 * (stride.value * slots)).from_address(base.value)
        arr = np.frombuffer(raw, dtype=np.uint8)
        self._ring = np.lib.stride_tricks.as_strided(arr, shape=(slots, height, width, 3), strides=(stride.value, width * 3, 3, 1))
        return self._ring

    def frame_ring_wait(self, slot: int):
        _check(self._lib.svln_frame_ring_wait(self._h, int(slot)))

    @property
    def device(self):
        return torch.device("cuda", self.device_index)

    # ---- session state (stream_video_vln.py:473-479) ----------------------------------------------
    def reset(self, env_num: int):
        """`model.reset(world_size)` in the reference harness (streamvln_eval.py:542): sizes the per-env host state.  The
        reference indexes that state with `env_id = rank` while each process only ever drives ONE env, so `env_num` may
        exceed the engine's `max_envs`: an env_id is bound to one of the engine's slots on first use, and at most
        `max_envs` env_ids can be live at a time."""
        if env_num < 1:
            raise ValueError("env_num must be >= 1")
        self.curr_t = [0] * env_num
        self._epoch = [0] * env_num
        self._slots: Dict[int, int] = {}
        self._last_out = {}                                        # auto-draft: the previous turn's ids per env_id
        self._group_pending = {}                                   # (svln_reset_env below drops a pending group and frees its pages)
        _check(self._lib.svln_batch_cancel(self._h, -1))           # turns still in the scheduler belong to the old state
        self._tickets.clear()
        self._forced_tickets.clear()
        for i in range(self.max_envs):
            _check(self._lib.svln_reset_env(self._h, i))

    def _slot(self, env_id: int) -> int:
        s = self._slots.get(env_id)
        if s is None:
            used = set(self._slots.values())
            free = [i for i in range(self.max_envs) if i not in used]
            if not free:
                raise ValueError(f"env_id {env_id}: all {self.max_envs} engine slots are bound to other envs "
                                 f"({sorted(self._slots)}); build the model with a larger max_envs")
            s = self._slots[env_id] = free[0]
        return s

    def reset_for_env(self, env_idx: int):
        if not (0 <= env_idx < len(self.curr_t)):
            raise IndexError(f"env_id {env_idx} out of range")
        self.curr_t[env_idx] = 0
        self._epoch[env_idx] += 1
        self._last_out.pop(env_idx, None)
        self._group_pending.pop(env_idx, None)                     # (svln_reset_env drops the env's pending group)
        if env_idx in self._slots:
            _check(self._lib.svln_reset_env(self._h, self._slots[env_idx]))       # (drops the env's scheduler turn, if any)
        for slot in [k for k, v in self._tickets.items() if v[0] == env_idx]:
            del self._tickets[slot]
            self._forced_tickets.pop(slot, None)

    # ---- the call (stream_video_vln.py:353-407) -------------------------------------------------------
    def _parse_call(self, inputs, images, kwargs):
        """argument handling shared by generate / generate_batch; returns (ids, pixels [V,3,S,S] fp32, V, n_memory, env_id, past,
        max_new, eos)"""
        kwargs = dict(kwargs)
        for k in ("position_ids", "attention_mask", "task_type", "image_sizes", "depths", "poses", "intrinsics", "task_ids"):
            kwargs.pop(k, None)
        time_ids = kwargs.pop("time_ids", None)
        if "inputs_embeds" in kwargs:
            raise NotImplementedError("`inputs_embeds` is not supported")
        env_id = kwargs.pop("env_id", None)
        past = kwargs.pop("past_key_values", None)
        max_new = int(kwargs.pop("max_new_tokens", 10000))
        eos = kwargs.pop("eos_token_ids", None)
        if kwargs.get("num_beams", 1) != 1:
            raise NotImplementedError(f"num_beams={kwargs.get('num_beams')!r}: only greedy decoding and temperature sampling (num_beams=1) are on the path")
        if kwargs.get("do_sample", False):
            # the per-call keys stay refused: truncation is a setting of the model (set_sampling_truncation / sampling_truncation), as
            # the seed is, so that every call of a run samples under the same rule
            if kwargs.get("top_k") not in (None, 0):
                raise NotImplementedError(f"top_k={kwargs['top_k']!r}: do_sample=True takes the temperature only (top_k None or 0); "
                                          f"truncated sampling is set on the model: set_sampling_truncation(top_k, top_p)")
            if kwargs.get("top_p") not in (None, 1.0):
                raise NotImplementedError(f"top_p={kwargs['top_p']!r}: do_sample=True takes the temperature only (top_p None or 1.0); "
                                          f"truncated sampling is set on the model: set_sampling_truncation(top_k, top_p)")
        if eos is None:
            eos = self.generation_config.eos_token_id
        eos = [int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos])]
        if images is None:
            raise NotImplementedError("text-only turns are not part of the streaming path")
        if env_id is None or not (0 <= env_id < len(self.curr_t)):
            raise IndexError(f"env_id {env_id} out of range")
        if env_id in self._group_pending:
            raise RuntimeError(f"env_id {env_id}: a group turn (num_return_sequences={self._group_pending[env_id]}) is pending; call "
                               f"select_sequence(index, env_id={env_id}) before the env's next turn")
        ids = torch.as_tensor(inputs).reshape(-1).to("cpu", torch.int64)
        if ids.numel() == 1:
            raise NotImplementedError("single-token `inputs` bypasses the multimodal path in the reference "
                                      "(stream_video_vln.py:149)")
        B, V = images.shape[0], images.shape[1]
        if B != 1:
            raise NotImplementedError("one env per request (reference harnesses run batch 1); use generate_batch for several envs")
        n_memory = 0
        if V != 1:                                            # encode_rgbd, stream_video_vln.py:111-130
            start_idx = time_ids[0][0] if (time_ids is not None and time_ids[0] is not None) else 0
            if start_idx != 0:
                if self.model.num_history is None:
                    raise TypeError("model.num_history must be set before a <memory> turn")
                n_memory = int(self.model.num_history)
        pix = images[0].to(torch.float32).contiguous()
        return ids, pix, V, n_memory, env_id, past, max_new, eos

    def _begin_turn(self, env_id, past):
        """KV handle / per-env embeds bookkeeping of StreamVLNForCausalLM.generate (stream_video_vln.py:396-401)"""
        if past is None:
            _check(self._lib.svln_kv_reset(self._h, self._slot(env_id)))
        elif not isinstance(past, KVHandle) or past.env_id != env_id or past.epoch != self._epoch[env_id]:
            raise ValueError("past_key_values does not belong to this env's current window")
        if self.curr_t[env_id] == 0:
            ne, kl = C.c_int32(), C.c_int32()
            _check(self._lib.svln_env_state(self._h, self._slot(env_id), C.byref(ne), C.byref(kl)))
            if ne.value != 0:
                _check(self._lib.svln_reset_env(self._h, self._slot(env_id)))
        self.curr_t[env_id] += 1

    def _result(self, env_id, tokens, inputs):
        ne, kl = C.c_int32(), C.c_int32()
        _check(self._lib.svln_env_state(self._h, self._slot(env_id), C.byref(ne), C.byref(kl)))
        dev = inputs.device if isinstance(inputs, torch.Tensor) else "cpu"
        seq = torch.from_numpy(np.asarray(tokens, dtype=np.int64).copy()).unsqueeze(0).to(dev)
        return GenerateOutput(sequences=seq, past_key_values=KVHandle(env_id, self._epoch[env_id], kl.value))

    def _sync_sampling(self, kwargs):
        """`do_sample` of a call -> the engine switch, flipped only when it differs from what the engine holds (a flip restarts the draw
        counters).  do_sample=True: the temperature of the call, else generation_config.temperature, else 1.0; the seed is
        self.sampling_seed.  do_sample=False -- the reference harness's call -- is the untouched greedy path whatever a checkpoint's
        generation_config says.  A call without the key leaves the switch as set_sampling left it."""
        if "do_sample" not in kwargs:
            return
        want = None
        if kwargs["do_sample"]:
            t = kwargs.get("temperature")
            if t is None:
                t = getattr(self.generation_config, "temperature", None)
            want = (float(1.0 if t is None else t), int(self.sampling_seed))
        if want != self._sampling:
            self.set_sampling(None) if want is None else self._switch_sampling_on(*want)

    def _scores(self, getter, *args, n_new, device):
        """token_logprobs [1, n_new] (fp32, on `device`) of a finished turn from one of the engine's score getters"""
        buf = np.empty(max(n_new, 1), dtype=np.float32)
        n = C.c_int32()
        _check(getter(self._h, *args, buf.ctypes.data_as(C.POINTER(C.c_float)), int(buf.size), C.byref(n)))
        if n.value != n_new:
            raise RuntimeError(f"the engine holds {n.value} token scores for a turn of {n_new} ids")
        return torch.from_numpy(buf[:n_new].copy()).unsqueeze(0).to(device)

    def _topk(self, n_new, device, getter=None, *args):
        """top_token_ids int64 [1, n_new, k] and top_logprobs fp32 [1, n_new, k] (on `device`) of a finished turn from one of the engine's
        list getters (default: svln_get_topk, the last single-env turn)"""
        k = self.top_logprobs_k
        getter = getter or self._lib.svln_get_topk
        ids = np.empty(max(n_new, 1) * k, dtype=np.int32)
        lps = np.empty(max(n_new, 1) * k, dtype=np.float32)
        nr, nk = C.c_int32(), C.c_int32()
        _check(getter(self._h, *args, ids.ctypes.data_as(C.POINTER(C.c_int32)), lps.ctypes.data_as(C.POINTER(C.c_float)), max(n_new, 1),
                      C.byref(nr), C.byref(nk)))
        if nr.value != n_new or nk.value != k:
            raise RuntimeError(f"the engine holds {nr.value} x {nk.value} top log-probabilities for a turn of {n_new} ids at k = {k}")
        return (torch.from_numpy(ids[: n_new * k].astype(np.int64).reshape(1, n_new, k)).to(device),
                torch.from_numpy(lps[: n_new * k].reshape(1, n_new, k).copy()).to(device))

    def _allowed(self, res, getter, *args):
        """with set_token_scores and set_allowed_tokens both on: add `allowed_logprobs` [1, n_new, n_allowed] (fp32) and `allowed_token_ids`
        [n_allowed] (int64) of a finished turn to its result, from the engine's allowed-logprob getter named `getter`"""
        if not (self._token_scores and self.allowed_token_ids):
            return res
        getter = getattr(self._lib, getter)
        n_new, n_ids = int(res.sequences.shape[1]), len(self.allowed_token_ids)
        buf = np.empty(max(n_new * n_ids, 1), dtype=np.float32)
        nt, ni = C.c_int32(), C.c_int32()
        _check(getter(self._h, *args, buf.ctypes.data_as(C.POINTER(C.c_float)), int(buf.size), C.byref(nt), C.byref(ni)))
        if nt.value != n_new or ni.value != n_ids:
            raise RuntimeError(f"the engine holds {nt.value} x {ni.value} allowed log-probabilities for a turn of {n_new} ids over {n_ids} allowed ids")
        dev = res.sequences.device
        res["allowed_logprobs"] = torch.from_numpy(buf[: n_new * n_ids].reshape(1, n_new, n_ids).copy()).to(dev)
        res["allowed_token_ids"] = torch.tensor(self.allowed_token_ids, dtype=torch.int64, device=dev)
        return res

    @torch.no_grad()
    def generate(self, inputs=None, images=None, image_sizes=None, depths=None, poses=None, intrinsics=None, task_ids=None,
                 draft_ids=None, forced_ids=None, candidate_ids=None, beam_width=None, fold_candidates=False, draft_set=None, **kwargs):
        """One model turn = ONE crossing into the engine (svln_turn: encode_rgbd, the KV / embeds bookkeeping of the reference's generate,
        splice, prefill + greedy decode).  draft_ids (optional, set_speculative / set_prefill_draft): a guess of this turn's whole id sequence; with
        set_auto_draft(True) and no explicit draft, the env's previous turn output is the guess.
        While set_token_scores is on the result also carries `token_logprobs`, fp32 [1, n_new] aligned with `sequences` (see there).  HF's
        `output_scores` / `output_logits` stay ignored: a [n_new, vocab] tensor is exactly what this engine exists not to build.
        do_sample=True with num_return_sequences=G, 2 <= G <= 8: a group turn (see _group_result for the result, select_sequence for what
        must follow); absent or 1: this path, launch for launch; a greedy call leaves the key unread.
        forced_ids (1 .. 32 ids): a forced turn -- the turn's ids are the caller's (see _generate_forced); `max_new_tokens` is not read.
        candidate_ids (2 .. 8 id lists of 1 .. 32 ids): the candidates are scored against ONE prefill of the prompt (see
        _generate_candidates for the result, select_sequence for what must follow); `max_new_tokens` is not read.
        fold_candidates=True (with candidate_ids only): the candidates' first rows ride the prefill pass (svln_turn_candidates_folded) --
        same result layout and follow-up, one weight pass less; no result is bit-equal to the unfolded call's.
        beam_width (1 .. 8): a beam turn -- the beam_width most probable turns of the prompt (see _generate_beams for the result,
        select_sequence for what must follow); HF's `num_beams` stays refused.
        draft_set (0 .. 8 guessed id sequences of 0 .. 32 ids): a multi-draft turn (svln_turn_drafts) -- the plain greedy turn with hints,
        all verified in the one prefill pass; ids, cache length and getters are the plain turn's.  The result also carries `draft_index`
        (the winning draft; -1: no pass ran, the hints were ignored) and `draft_tokens` (the tokens the pass emitted)."""
        draft = draft_ids
        if fold_candidates and candidate_ids is None:
            raise ValueError("fold_candidates without candidate_ids: only a candidates call has rows to fold into the prefill")
        dset = None
        if draft_set is not None:
            for name, v in (("draft_ids", draft_ids), ("forced_ids", forced_ids), ("candidate_ids", candidate_ids), ("beam_width", beam_width)):
                if v is not None:
                    raise NotImplementedError(f"draft_set together with {name}: a multi-draft turn is a plain greedy turn with hints")
            dset = self._draft_set_arrays(draft_set)
        W = self._beam_request(beam_width, forced_ids, candidate_ids, kwargs)
        ids, pix, V, n_memory, env_id, past, max_new, eos = self._parse_call(inputs, images, kwargs)
        n_seq = self._num_return_sequences(kwargs)
        if dset is not None and n_seq > 1:
            raise NotImplementedError("draft_set together with num_return_sequences > 1: a multi-draft turn returns one sequence")
        if forced_ids is not None and n_seq > 1:
            raise NotImplementedError("forced_ids with num_return_sequences > 1: a forced turn has one sequence")
        if candidate_ids is not None and forced_ids is not None:
            raise NotImplementedError("candidate_ids together with forced_ids: a forced turn scores one sequence, a candidates call several")
        if candidate_ids is not None and n_seq > 1:
            raise NotImplementedError("candidate_ids with num_return_sequences > 1: the candidates are the call's sequences")
        self._sync_call_config()
        held = self._sampling
        self._sync_sampling(kwargs)
        if W or forced_ids is not None or candidate_ids is not None or n_seq > 1:
            try:
                if W:
                    return self._generate_beams(W, inputs, ids, pix, V, n_memory, env_id, past, max_new, eos)
                if candidate_ids is not None:
                    return self._generate_candidates(candidate_ids, inputs, ids, pix, V, n_memory, env_id, past, eos, fold=bool(fold_candidates))
                if forced_ids is not None:
                    return self._generate_forced(forced_ids, inputs, ids, pix, V, n_memory, env_id, past, eos)
                return self._generate_group(n_seq, inputs, ids, pix, V, n_memory, env_id, past, max_new, eos)
            except Exception:
                # a refused call changes no state: the sampling switch this call flipped goes back to what the engine held
                if self._sampling != held:
                    self.set_sampling(None) if held is None else self._switch_sampling_on(*held)
                raise
        # the reference's bookkeeping that needs no engine call: the KV handle must be this env's current one; curr_t counts the turns
        if past is not None and (not isinstance(past, KVHandle) or past.env_id != env_id or past.epoch != self._epoch[env_id]):
            raise ValueError("past_key_values does not belong to this env's current window")
        slot = self._slot(env_id)
        on_dev = int(pix.is_cuda)
        ids_np = ids.numpy()
        cap = min(max_new, self.cfg.max_positions)
        buf = self._turn_buffers(cap, eos)
        a = buf["args"]
        a.pixels, a.n_frames, a.pixels_on_device, a.env = pix.data_ptr(), V, on_dev, slot
        a.ids, a.n_ids, a.n_memory = ids_np.ctypes.data, ids_np.size, n_memory
        a.new_window, a.new_episode, a.max_new_tokens = int(past is None), int(self.curr_t[env_id] == 0), max_new
        auto = self._auto_draft
        if draft is None and auto and dset is None:
            draft = self._last_out.get(env_id)
        if draft is not None:
            d_np = np.ascontiguousarray(torch.as_tensor(draft).reshape(-1).to("cpu", torch.int64).numpy())
            _check(self._lib.svln_set_draft(self._h, slot, d_np.ctypes.data_as(C.POINTER(C.c_int64)), int(d_np.size)))
        if on_dev:
            self._order_engine_after(pix)
        if dset is not None:
            # a multi-draft turn (svln_turn_drafts): the plain turn with hints; the result says which draft won and what the pass emitted
            flat, lens = dset
            win, ptok = C.c_int32(-1), C.c_int32(0)
            rc = self._lib.svln_turn_drafts(self._h, buf["args_ref"], int(lens.size), flat.ctypes.data_as(C.POINTER(C.c_int64)),
                                            lens.ctypes.data_as(C.POINTER(C.c_int32)), buf["out_p"], cap, buf["n_out_ref"], buf["kv_ref"],
                                            C.byref(win), C.byref(ptok))
        else:
            rc = self._lib.svln_turn(self._h, buf["args_ref"], buf["out_p"], cap, buf["n_out_ref"], buf["kv_ref"])
        if on_dev:
            self._order_torch_after(pix)
        _check(rc)
        self.curr_t[env_id] += 1
        dev = inputs.device if isinstance(inputs, torch.Tensor) else "cpu"
        seq = torch.from_numpy(buf["out"][: buf["n_out"].value].copy()).unsqueeze(0)
        if auto:
            self._last_out[env_id] = seq[0].clone()
        if dev != "cpu" and str(dev) != "cpu":
            seq = seq.to(dev)
        res = GenerateOutput(sequences=seq, past_key_values=KVHandle(env_id, self._epoch[env_id], buf["kv"].value))
        if dset is not None:
            res["draft_index"], res["draft_tokens"] = int(win.value), int(ptok.value)
        if self._token_scores:
            res["token_logprobs"] = self._scores(self._lib.svln_get_token_scores, n_new=int(seq.shape[1]), device=seq.device)
        if self.top_logprobs_k:
            res["top_token_ids"], res["top_logprobs"] = self._topk(n_new=int(seq.shape[1]), device=seq.device)
        if self._token_entropy:
            res["token_entropies"] = self._scores(self._lib.svln_get_token_entropy, n_new=int(seq.shape[1]), device=seq.device)
        return self._allowed(res, "svln_get_allowed_logprobs")

    @staticmethod
    def _draft_set_arrays(draft_set):
        """draft_set -> (flat int64 ids, int32 lengths); 0 .. 8 guessed id sequences of 0 .. 32 ids"""
        rows = [np.ascontiguousarray(torch.as_tensor(d).reshape(-1).to("cpu", torch.int64).numpy()) for d in draft_set]
        if len(rows) > 8:
            raise ValueError(f"draft_set holds {len(rows)} drafts: a multi-draft turn takes 0 .. 8")
        for g, r in enumerate(rows):
            if r.size > 32:
                raise ValueError(f"draft_set[{g}] holds {int(r.size)} ids: a draft has 0 .. 32")
        flat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, np.int64), dtype=np.int64)
        if flat.size == 0:
            flat = np.zeros(1, np.int64)              # (never read: every length is 0)
        return flat, np.asarray([r.size for r in rows], np.int32).reshape(-1)

    # ---- forced turns: log-probabilities of given ids in one prefill pass (svln_turn_forced) --------------
    def _generate_forced(self, forced, inputs, ids, pix, V, n_memory, env_id, past, eos):
        """generate(..., forced_ids=F): ONE vision pass and ONE prefill pass that also feeds F[:-1]; no decode phase.  The result carries
        `sequences` = F [1, n], `token_logprobs` fp32 [1, n] (the policy's log-probability of every F[i] given the prompt and F[:i];
        always present, whatever set_token_scores says), `greedy_ids` int64 [1, n] and `greedy_logprobs` fp32 [1, n] (the policy's own
        arg-max at every position), with an allowed list `allowed_logprobs` [1, n, n_allowed] / `allowed_token_ids`, and the usual
        `past_key_values`: the env is where a plain turn that emitted F would have left it."""
        if past is not None and (not isinstance(past, KVHandle) or past.env_id != env_id or past.epoch != self._epoch[env_id]):
            raise ValueError("past_key_values does not belong to this env's current window")
        f_np = np.ascontiguousarray(torch.as_tensor(forced).reshape(-1).to("cpu", torch.int64).numpy())
        n = int(f_np.size)
        if not (1 <= n <= 32):
            raise ValueError(f"forced_ids holds {n} ids: a forced turn takes 1 .. 32")
        slot = self._slot(env_id)
        on_dev = int(pix.is_cuda)
        ids_np = np.ascontiguousarray(ids.numpy())
        eos_np = np.asarray(eos, dtype=np.int64)
        lp, glp, gid, kv = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64), C.c_int32()
        a = _lib.SvlnTurnArgs()
        a.pixels, a.n_frames, a.pixels_on_device, a.env = pix.data_ptr(), V, on_dev, slot
        a.ids, a.n_ids, a.n_memory = ids_np.ctypes.data, ids_np.size, n_memory
        a.new_window, a.new_episode, a.max_new_tokens = int(past is None), int(self.curr_t[env_id] == 0), n
        a.eos_ids, a.n_eos = eos_np.ctypes.data, eos_np.size
        if on_dev:
            self._order_engine_after(pix)
        PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int64)
        rc = self._lib.svln_turn_forced(self._h, C.byref(a), f_np.ctypes.data_as(PI), n, lp.ctypes.data_as(PF), gid.ctypes.data_as(PI),
                                        glp.ctypes.data_as(PF), C.byref(kv))
        if on_dev:
            self._order_torch_after(pix)
        _check(rc)
        self.curr_t[env_id] += 1
        dev = inputs.device if isinstance(inputs, torch.Tensor) else "cpu"
        seq = torch.from_numpy(f_np.copy()).unsqueeze(0)
        if self._auto_draft:
            self._last_out[env_id] = seq[0].clone()
        res = GenerateOutput(sequences=seq.to(dev), past_key_values=KVHandle(env_id, self._epoch[env_id], kv.value))
        res["token_logprobs"] = torch.from_numpy(lp).unsqueeze(0).to(dev)
        res["greedy_ids"] = torch.from_numpy(gid).unsqueeze(0).to(dev)
        res["greedy_logprobs"] = torch.from_numpy(glp).unsqueeze(0).to(dev)
        if self.allowed_token_ids:
            n_ids = len(self.allowed_token_ids)
            buf, nt, ni = np.empty(n * n_ids, dtype=np.float32), C.c_int32(), C.c_int32()
            _check(self._lib.svln_get_allowed_logprobs(self._h, buf.ctypes.data_as(PF), int(buf.size), C.byref(nt), C.byref(ni)))
            if nt.value != n or ni.value != n_ids:
                raise RuntimeError(f"the engine holds {nt.value} x {ni.value} allowed log-probabilities for a forced turn of {n} ids over {n_ids} allowed ids")
            res["allowed_logprobs"] = torch.from_numpy(buf.reshape(1, n, n_ids).copy()).to(dev)
            res["allowed_token_ids"] = torch.tensor(self.allowed_token_ids, dtype=torch.int64, device=dev)
        return res

    # ---- candidate scoring: several given continuations of one prompt in one prefill (svln_turn_candidates) ----
    @staticmethod
    def _candidate_arrays(cands):
        """candidate_ids -> (flat int64 ids, int32 lengths); 2 .. 8 sequences of 1 .. 32 ids"""
        if isinstance(cands, torch.Tensor) and cands.dim() != 2:
            raise ValueError("candidate_ids: a list of id sequences (or a [G, n] tensor)")
        rows = [np.ascontiguousarray(torch.as_tensor(c).reshape(-1).to("cpu", torch.int64).numpy()) for c in cands]
        if not (2 <= len(rows) <= 8):
            raise ValueError(f"candidate_ids holds {len(rows)} sequences: a candidates call takes 2 .. 8")
        for g, r in enumerate(rows):
            if not (1 <= r.size <= 32):
                raise ValueError(f"candidate_ids[{g}] holds {int(r.size)} ids: a candidate has 1 .. 32")
        return np.ascontiguousarray(np.concatenate(rows)), np.asarray([r.size for r in rows], dtype=np.int32)

    def _generate_candidates(self, cands, inputs, ids, pix, V, n_memory, env_id, past, eos, *, fold=False):
        """generate(..., candidate_ids=[F_0, ..., F_{G-1}]): ONE vision pass, ONE prefill of the prompt and ceil(max_g (n_g - 1) / r) scoring
        passes for all candidates together; no decode phase.  The result is shaped like a group turn's: `sequences` int64 [G, n_max]
        (padded like a group's), `sequence_lengths` [G], `token_logprobs` fp32 [G, n_max] (log p(F_g[i] | prompt, F_g[:i]), pad 0: a row
        sum is the candidate's joint log-probability; always present), `greedy_ids` int64 / `greedy_logprobs` fp32 [G, n_max] (the
        policy's own arg-max at every position; pads: the pad id / 0), with an allowed list `allowed_logprobs` [G, n_max, n_allowed] /
        `allowed_token_ids`, and `past_key_values` None: select_sequence(index, env_id) must follow, and leaves the env where
        generate(forced_ids=F_index) would have.  fold=True (generate's fold_candidates): the first min(r, n_g - 1) fed rows of every
        candidate ride the prefill pass (svln_turn_candidates_folded); the result has the same layout."""
        if past is not None and (not isinstance(past, KVHandle) or past.env_id != env_id or past.epoch != self._epoch[env_id]):
            raise ValueError("past_key_values does not belong to this env's current window")
        flat, lens = self._candidate_arrays(cands)
        G, n_max, total = int(lens.size), int(lens.max()), int(flat.size)
        slot = self._slot(env_id)
        on_dev = int(pix.is_cuda)
        ids_np = np.ascontiguousarray(ids.numpy())
        eos_np = np.asarray(eos, dtype=np.int64)
        lp, glp, gid = np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.int64)
        a = _lib.SvlnTurnArgs()
        a.pixels, a.n_frames, a.pixels_on_device, a.env = pix.data_ptr(), V, on_dev, slot
        a.ids, a.n_ids, a.n_memory = ids_np.ctypes.data, ids_np.size, n_memory
        a.new_window, a.new_episode, a.max_new_tokens = int(past is None), int(self.curr_t[env_id] == 0), n_max
        a.eos_ids, a.n_eos = eos_np.ctypes.data, eos_np.size
        if on_dev:
            self._order_engine_after(pix)
        PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int64)
        turn = self._lib.svln_turn_candidates_folded if fold else self._lib.svln_turn_candidates
        rc = turn(self._h, C.byref(a), G, flat.ctypes.data_as(PI), lens.ctypes.data_as(C.POINTER(C.c_int32)),
                  lp.ctypes.data_as(PF), gid.ctypes.data_as(PI), glp.ctypes.data_as(PF))
        if on_dev:
            self._order_torch_after(pix)
        _check(rc)
        self.curr_t[env_id] += 1
        self._group_pending[env_id] = G
        dev = inputs.device if isinstance(inputs, torch.Tensor) else "cpu"
        pad = getattr(self.generation_config, "pad_token_id", None)
        if pad is None:
            pad = eos[0] if len(eos) else 0
        seq, gids = np.full((G, n_max), int(pad), dtype=np.int64), np.full((G, n_max), int(pad), dtype=np.int64)
        tlp, tglp = np.zeros((G, n_max), dtype=np.float32), np.zeros((G, n_max), dtype=np.float32)
        off = 0
        for g in range(G):
            n = int(lens[g])
            seq[g, :n], gids[g, :n], tlp[g, :n], tglp[g, :n] = flat[off:off + n], gid[off:off + n], lp[off:off + n], glp[off:off + n]
            off += n
        res = GenerateOutput(sequences=torch.from_numpy(seq).to(dev), sequence_lengths=torch.from_numpy(lens.astype(np.int64)).to(dev),
                             past_key_values=None)
        res["token_logprobs"] = torch.from_numpy(tlp).to(dev)
        res["greedy_ids"] = torch.from_numpy(gids).to(dev)
        res["greedy_logprobs"] = torch.from_numpy(tglp).to(dev)
        if self.allowed_token_ids:
            n_ids = len(self.allowed_token_ids)
            alp = np.zeros((G, n_max, n_ids), dtype=np.float32)
            buf, nr, nc = np.empty(n_max * n_ids, dtype=np.float32), C.c_int32(), C.c_int32()
            for g in range(G):
                n = int(lens[g])
                _check(self._lib.svln_group_dist(self._h, g, buf.ctypes.data_as(PF), n_max, C.byref(nr), C.byref(nc)))
                if nr.value != n or nc.value != n_ids:
                    raise RuntimeError(f"the engine holds {nr.value} x {nc.value} allowed log-probabilities for a candidate of {n} ids over {n_ids} allowed ids")
                alp[g, :n] = buf[: n * n_ids].reshape(n, n_ids)
            res["allowed_logprobs"] = torch.from_numpy(alp).to(dev)
            res["allowed_token_ids"] = torch.tensor(self.allowed_token_ids, dtype=torch.int64, device=dev)
        return res

    # ---- group sampling: several sampled continuations of one prefill (svln_turn_group) ----------------
    @staticmethod
    def _num_return_sequences(kwargs) -> int:
        """HF's `num_return_sequences` of a generate call: read under do_sample=True only (a greedy call leaves the key unread, as
        before); 1 or absent = the plain turn; 2 .. 8 = a group turn; anything else raises."""
        if not kwargs.get("do_sample", False):
            return 1
        g = kwargs.get("num_return_sequences")
        g = 1 if g is None else int(g)
        if not (1 <= g <= 8):
            raise ValueError(f"num_return_sequences={g}: a group turn returns 1 .. 8 sequences")
        return g

    @staticmethod
    def _beam_request(beam_width, forced_ids, candidate_ids, kwargs) -> int:
        """`beam_width` of a generate call: None = no beam turn (0); 1 .. 8 = the width; the combinations a beam turn does not have raise"""
        if beam_width is None:
            return 0
        W = int(beam_width)
        if not (1 <= W <= 8):
            raise ValueError(f"beam_width={beam_width!r}: a beam turn keeps 1 .. 8 hypotheses")
        if forced_ids is not None:
            raise NotImplementedError("beam_width together with forced_ids: a forced turn's ids are the caller's, a beam turn's the policy's")
        if candidate_ids is not None:
            raise NotImplementedError("beam_width together with candidate_ids: a candidates call scores given turns, a beam turn finds them")
        if kwargs.get("do_sample", False):
            raise NotImplementedError("beam_width together with do_sample=True: beams are greedy (no beam sampling on the path)")
        g = kwargs.get("num_return_sequences")
        if g is not None and int(g) > 1:
            raise NotImplementedError(f"beam_width together with num_return_sequences={g!r}: a beam turn returns its whole set")
        return W

    def _generate_beams(self, W, inputs, ids, pix, V, n_memory, env_id, past, max_new, eos):
        """generate(..., beam_width=W): ONE vision pass, ONE prefill and one batched decode phase for at most W hypotheses (svln_turn_beams).
        The result is shaped like a group turn's: `sequences` int64 [n, n_max] in rank order (n <= W; padded like a group's),
        `sequence_lengths` [n], `token_logprobs` fp32 [n, n_max] (pad 0), `sequences_scores` fp32 [n] (the fp32 sum of a row's
        log-probabilities, no length penalty), `past_key_values` None: select_sequence(index, env_id) must follow.  The pages of every
        hypothesis are reserved up front: pass the max_new_tokens the turn really needs (see _generate_group)."""
        if past is not None and (not isinstance(past, KVHandle) or past.env_id != env_id or past.epoch != self._epoch[env_id]):
            raise ValueError("past_key_values does not belong to this env's current window")
        slot = self._slot(env_id)
        on_dev = int(pix.is_cuda)
        ids_np = np.ascontiguousarray(ids.numpy())
        eos_np = np.asarray(eos, dtype=np.int64)
        cap = min(max_new, self.cfg.max_positions)
        out, n_out, sc = np.zeros((W, cap), dtype=np.int64), np.zeros(W, dtype=np.int32), np.zeros(W, dtype=np.float32)
        a = _lib.SvlnTurnArgs()
        a.pixels, a.n_frames, a.pixels_on_device, a.env = pix.data_ptr(), V, on_dev, slot
        a.ids, a.n_ids, a.n_memory = ids_np.ctypes.data, ids_np.size, n_memory
        a.new_window, a.new_episode, a.max_new_tokens = int(past is None), int(self.curr_t[env_id] == 0), max_new
        a.eos_ids, a.n_eos = eos_np.ctypes.data, eos_np.size
        if on_dev:
            self._order_engine_after(pix)
        rc = self._lib.svln_turn_beams(self._h, C.byref(a), W, out.ctypes.data_as(C.POINTER(C.c_int64)), cap,
                                       n_out.ctypes.data_as(C.POINTER(C.c_int32)), sc.ctypes.data_as(C.POINTER(C.c_float)))
        if on_dev:
            self._order_torch_after(pix)
        _check(rc)
        self.curr_t[env_id] += 1
        n = int((n_out > 0).sum())
        self._group_pending[env_id] = n
        dev = inputs.device if isinstance(inputs, torch.Tensor) else "cpu"
        lens = [int(v) for v in n_out[:n]]
        n_max = max(lens)
        pad = getattr(self.generation_config, "pad_token_id", None)
        if pad is None:
            pad = eos[0] if len(eos) else 0
        seq, lp = np.full((n, n_max), int(pad), dtype=np.int64), np.zeros((n, n_max), dtype=np.float32)
        buf, m = np.empty(n_max, dtype=np.float32), C.c_int32()
        for g in range(n):
            seq[g, : lens[g]] = out[g, : lens[g]]
            _check(self._lib.svln_group_logprobs(self._h, g, buf.ctypes.data_as(C.POINTER(C.c_float)), n_max, C.byref(m)))
            if m.value != lens[g]:
                raise RuntimeError(f"the engine holds {m.value} token scores for a hypothesis of {lens[g]} ids")
            lp[g, : lens[g]] = buf[: lens[g]]
        res = GenerateOutput(sequences=torch.from_numpy(seq).to(dev), sequence_lengths=torch.tensor(lens, dtype=torch.int64, device=dev),
                             past_key_values=None)
        res["token_logprobs"] = torch.from_numpy(lp).to(dev)
        res["sequences_scores"] = torch.from_numpy(sc[:n].copy()).to(dev)
        return res

    def beam_trace(self):
        """test tap: the steps of the last beam turn -> (W, list_ids int32 [steps, 8, 8], list_lps fp32 [steps, 8, 8], records int32 [steps, 28])"""
        cap = self.cfg.max_positions
        li, ll, rec = np.zeros((cap, 8, 8), dtype=np.int32), np.zeros((cap, 8, 8), dtype=np.float32), np.zeros((cap, 28), dtype=np.int32)
        ns, w = C.c_int32(), C.c_int32()
        _check(self._lib.svln_beam_trace(self._h, cap, C.byref(ns), C.byref(w), li.ctypes.data_as(C.POINTER(C.c_int32)),
                                         ll.ctypes.data_as(C.POINTER(C.c_float)), rec.ctypes.data_as(C.POINTER(C.c_int32))))
        return w.value, li[: ns.value].copy(), ll[: ns.value].copy(), rec[: ns.value].copy()

    @staticmethod
    def _reject_group_request(kwargs, who):
        if kwargs.get("beam_width") is not None:
            raise NotImplementedError(f"beam_width in a {who} request: beam turns run through generate() only")
        if kwargs.get("forced_ids") is not None:
            raise NotImplementedError(f"forced_ids in a {who} request: forced turns run through generate() only")
        if kwargs.get("candidate_ids") is not None:
            raise NotImplementedError(f"candidate_ids in a {who} request: candidates are scored through generate() only")
        if kwargs.get("fold_candidates"):
            raise NotImplementedError(f"fold_candidates in a {who} request: candidates are scored through generate() only")
        if kwargs.get("draft_set") is not None:
            raise NotImplementedError(f"draft_set in a {who} request: multi-draft turns run through generate() only")
        g = kwargs.get("num_return_sequences")
        if g is not None and int(g) > 1:
            raise NotImplementedError(f"num_return_sequences={g!r} in a {who} request: group turns run through generate() only")

    def _generate_group(self, n_seq, inputs, ids, pix, V, n_memory, env_id, past, max_new, eos):
        """generate(do_sample=True, num_return_sequences=G): ONE vision pass, ONE prefill, one batched decode phase for G sequences.
        The fork reserves the pages of every sequence up front, so the engine refuses a call whose n_embeds + max_new_tokens - 1 exceeds
        max_positions: pass the max_new_tokens the turn really needs (the default of 10000 never fits).  draft_ids are not used."""
        if past is not None and (not isinstance(past, KVHandle) or past.env_id != env_id or past.epoch != self._epoch[env_id]):
            raise ValueError("past_key_values does not belong to this env's current window")
        slot = self._slot(env_id)
        on_dev = int(pix.is_cuda)
        ids_np = np.ascontiguousarray(ids.numpy())
        eos_np = np.asarray(eos, dtype=np.int64)
        cap = min(max_new, self.cfg.max_positions)
        out = np.zeros((n_seq, cap), dtype=np.int64)
        n_out = np.zeros(n_seq, dtype=np.int32)
        a = _lib.SvlnTurnArgs()
        a.pixels, a.n_frames, a.pixels_on_device, a.env = pix.data_ptr(), V, on_dev, slot
        a.ids, a.n_ids, a.n_memory = ids_np.ctypes.data, ids_np.size, n_memory
        a.new_window, a.new_episode, a.max_new_tokens = int(past is None), int(self.curr_t[env_id] == 0), max_new
        a.eos_ids, a.n_eos = eos_np.ctypes.data, eos_np.size
        if on_dev:
            self._order_engine_after(pix)
        rc = self._lib.svln_turn_group(self._h, C.byref(a), n_seq, out.ctypes.data_as(C.POINTER(C.c_int64)), cap,
                                       n_out.ctypes.data_as(C.POINTER(C.c_int32)))
        if on_dev:
            self._order_torch_after(pix)
        _check(rc)
        self.curr_t[env_id] += 1
        self._group_pending[env_id] = n_seq
        dev = inputs.device if isinstance(inputs, torch.Tensor) else "cpu"
        return self._group_result(out, n_out, eos, dev)

    def _group_result(self, out, n_out, eos, device="cpu"):
        """the GenerateOutput of a group turn from the engine's rows: `sequences` int64 [G, n_max] padded with
        generation_config.pad_token_id (else the first EOS id, else 0), `sequence_lengths` int64 [G], `past_key_values` None (the env has
        no cache length until select_sequence); with set_token_scores `token_logprobs` fp32 [G, n_max] padded with 0, so that a row sum is
        the sequence's joint log-probability; with set_allowed_tokens too `allowed_logprobs` fp32 [G, n_max, n_allowed] (padded with 0)
        and `allowed_token_ids`"""
        G, lens = int(out.shape[0]), [int(v) for v in n_out]
        n_max = max(lens)
        pad = getattr(self.generation_config, "pad_token_id", None)
        if pad is None:
            pad = eos[0] if len(eos) else 0
        seq = np.full((G, n_max), int(pad), dtype=np.int64)
        for g in range(G):
            seq[g, : lens[g]] = out[g, : lens[g]]
        res = GenerateOutput(sequences=torch.from_numpy(seq).to(device), sequence_lengths=torch.tensor(lens, dtype=torch.int64, device=device),
                             past_key_values=None)
        if self._token_scores:
            lp = np.zeros((G, n_max), dtype=np.float32)
            buf, n = np.empty(max(n_max, 1), dtype=np.float32), C.c_int32()
            for g in range(G):
                _check(self._lib.svln_group_logprobs(self._h, g, buf.ctypes.data_as(C.POINTER(C.c_float)), int(buf.size), C.byref(n)))
                if n.value != lens[g]:
                    raise RuntimeError(f"the engine holds {n.value} token scores for a sequence of {lens[g]} ids")
                lp[g, : lens[g]] = buf[: lens[g]]
            res["token_logprobs"] = torch.from_numpy(lp).to(device)
        if self._token_scores and self.allowed_token_ids:
            n_ids = len(self.allowed_token_ids)
            alp = np.zeros((G, n_max, n_ids), dtype=np.float32)
            buf, nr, nc = np.empty(max(n_max, 1) * n_ids, dtype=np.float32), C.c_int32(), C.c_int32()
            for g in range(G):
                _check(self._lib.svln_group_dist(self._h, g, buf.ctypes.data_as(C.POINTER(C.c_float)), max(n_max, 1), C.byref(nr), C.byref(nc)))
                if nr.value != lens[g] or nc.value != n_ids:
                    raise RuntimeError(f"the engine holds {nr.value} x {nc.value} allowed log-probabilities for a sequence of {lens[g]} ids over {n_ids} allowed ids")
                alp[g, : lens[g]] = buf[: lens[g] * n_ids].reshape(lens[g], n_ids)
            res["allowed_logprobs"] = torch.from_numpy(alp).to(device)
            res["allowed_token_ids"] = torch.tensor(self.allowed_token_ids, dtype=torch.int64, device=device)
        return res

    def select_sequence(self, index: int, env_id: int = 0) -> KVHandle:
        """After generate(do_sample=True, num_return_sequences=G): the env goes on with sequence `index` of that group turn -- its K / V
        pages become the env's, every other continuation's go back to the pool.  Returns the env's KVHandle (the `past_key_values` of its
        next turn); must be called before that env's next turn."""
        if env_id not in self._group_pending:
            raise RuntimeError(f"env_id {env_id}: no group turn is pending")
        kv = C.c_int32()
        _check(self._lib.svln_group_select(self._h, self._slot(env_id), int(index), C.byref(kv)))
        del self._group_pending[env_id]
        return KVHandle(env_id, self._epoch[env_id], kv.value)

    def last_hidden_group(self, index: int) -> np.ndarray:
        """parity tap: the final-norm rows of the first <= 8 tokens of sequence `index` of the pending group turn"""
        buf = np.empty((8, self.cfg.hidden), dtype=np.float32)
        n = C.c_int32()
        _check(self._lib.svln_get_hidden_group(self._h, int(index), buf.ctypes.data_as(C.POINTER(C.c_float)), 8, C.byref(n)))
        return buf[: n.value].copy()

    def _arm_batch_draft(self, env_id, draft):
        """set_batch_draft on: arm env_id's draft for the submit that follows -- explicit ids, or the env's previous output under
        set_auto_draft.  Off: nothing is armed."""
        if not self._batch_draft:
            return
        if draft is None and self._auto_draft:
            draft = self._last_out.get(env_id)
        if draft is None:
            return
        d_np = np.ascontiguousarray(torch.as_tensor(draft).reshape(-1).to("cpu", torch.int64).numpy())
        _check(self._lib.svln_set_draft(self._h, self._slot(env_id), d_np.ctypes.data_as(C.POINTER(C.c_int64)), int(d_np.size)))

    def _batch_result(self, env_id, tokens, inputs, scores=None):
        res = self._result(env_id, tokens, inputs)
        if scores is not None:
            res["token_logprobs"] = scores.to(res.sequences.device)
        if self._auto_draft:
            self._last_out[env_id] = res.sequences[0].to("cpu").clone()
        return res

    def _turn_buffers(self, cap, eos):
        """ctypes scratch of generate(), built once per (capacity, eos list): no per-turn allocation or pointer casting"""
        key = (cap, tuple(eos))
        buf = getattr(self, "_tbuf", None)
        if buf is None or buf["key"] != key:
            out = np.zeros(cap, dtype=np.int64)
            eos_np = np.asarray(eos, dtype=np.int64)
            args = _lib.SvlnTurnArgs()
            args.eos_ids, args.n_eos = eos_np.ctypes.data, eos_np.size
            n_out, kv = C.c_int32(), C.c_int32()
            buf = self._tbuf = {"key": key, "out": out, "out_p": out.ctypes.data_as(C.POINTER(C.c_int64)), "eos": eos_np, "args": args,
                                "args_ref": C.byref(args), "n_out": n_out, "n_out_ref": C.byref(n_out), "kv": kv, "kv_ref": C.byref(kv)}
        return buf

    @torch.no_grad()
    def generate_batch(self, requests, max_new_tokens: int = 10000, eos_token_ids=None):
        """Several envs' turns executed together (build-side extension, SURVEY.md 8f-1 / BASELINE configs[4]).
        `requests`: list of kwargs dicts as passed to `generate` (distinct env_id, at most 8).  Per-env results are those of
        `generate` called env by env (same protocol, same KV / embeds state); the dense layers and every decode step run
        once for the whole batch.  A request's `draft_ids` (or, under set_auto_draft, the env's previous output) is armed for the turn
        while set_batch_draft is on, and ignored otherwise.  Returns a list of GenerateOutput in request order."""
        if not (1 <= len(requests) <= 8):
            raise ValueError("1..8 requests per batch")
        parsed, drafts = [], []
        for r in requests:
            r = dict(r)
            self._reject_group_request(r, "generate_batch")
            drafts.append(r.pop("draft_ids", None))
            r.setdefault("max_new_tokens", max_new_tokens)
            if eos_token_ids is not None:
                r.setdefault("eos_token_ids", eos_token_ids)
            parsed.append((r,) + self._parse_call(r.pop("inputs", None), r.pop("images", None), r))
        if len({p[5] for p in parsed}) != len(parsed):
            raise ValueError("duplicate env_id in batch")
        max_new, eos = parsed[0][7], parsed[0][8]
        if any(p[7] != max_new or p[8] != eos for p in parsed):
            raise ValueError("max_new_tokens / eos_token_ids must be the same for every request of a batch")
        if self._tickets:
            raise RuntimeError("generate_batch needs an idle scheduler: collect or cancel the submitted turns first")
        self._sync_call_config()
        modes = {(bool(p[0].get("do_sample", False)), p[0].get("temperature")) if "do_sample" in p[0] else None for p in parsed}
        if len(modes) != 1:
            raise ValueError("do_sample / temperature must be the same for every request of a batch")
        self._sync_sampling(parsed[0][0])
        # vision: encode the frames of as many requests as fit the frame buffer per call, then splice per env
        i = 0
        while i < len(parsed):
            j, frames = i, 0
            while j < len(parsed) and (j == i or frames + parsed[j][3] <= self.max_frames):
                frames += parsed[j][3]
                j += 1
            if frames > self.max_frames:
                raise ValueError(f"a request has {frames} frames but the engine was built with max_frames={self.max_frames}")
            pix = torch.cat([p[2] for p in parsed[i:j]], 0).contiguous()
            on_dev = int(pix.is_cuda)
            if on_dev:
                self._order_engine_after(pix)
            _check(self._lib.svln_encode_frames(self._h, C.c_void_p(pix.data_ptr()), frames, on_dev))
            if on_dev:
                self._order_torch_after(pix)
            base = 0
            for (_, ids, _, V, n_memory, env_id, past, _, _) in parsed[i:j]:
                self._begin_turn(env_id, past)
                ids_np = np.ascontiguousarray(ids.numpy())
                _check(self._lib.svln_append_turn_at(self._h, self._slot(env_id), ids_np.ctypes.data_as(C.POINTER(C.c_int64)), ids_np.size, base, n_memory))
                base += V
            i = j
        for p, d in zip(parsed, drafts):
            self._arm_batch_draft(p[5], d)
        envs = np.asarray([self._slot(p[5]) for p in parsed], dtype=np.int32)
        cap = min(max_new, self.cfg.max_positions)
        out = np.zeros((len(parsed), cap), dtype=np.int64)
        n_out = np.zeros(len(parsed), dtype=np.int32)
        eos_np = np.asarray(eos, dtype=np.int64)
        _check(self._lib.svln_generate_batch(self._h, envs.ctypes.data_as(C.POINTER(C.c_int32)), len(parsed), max_new,
                                             eos_np.ctypes.data_as(C.POINTER(C.c_int64)), eos_np.size,
                                             out.ctypes.data_as(C.POINTER(C.c_int64)), cap, n_out.ctypes.data_as(C.POINTER(C.c_int32))))
        scores = [None] * len(parsed)
        if self._token_scores:
            scores = [self._scores(self._lib.svln_generate_batch_scores, k, n_new=int(n_out[k]), device="cpu") for k in range(len(parsed))]
        res = [self._allowed(self._batch_result(p[5], out[k, : n_out[k]], requests[k].get("inputs"), scores[k]),
                             "svln_generate_batch_allowed_logprobs", k) for k, p in enumerate(parsed)]
        if self.top_logprobs_k:
            for k, r in enumerate(res):
                r["top_token_ids"], r["top_logprobs"] = self._topk(int(n_out[k]), r.sequences.device, self._lib.svln_generate_batch_topk, k)
        if self._token_entropy:
            for k, r in enumerate(res):
                r["token_entropies"] = self._scores(self._lib.svln_generate_batch_entropy, k, n_new=int(n_out[k]), device=r.sequences.device)
        return res

    # ---- iteration-level scheduler: envs whose turns fall due at different times (streamvln_dagger.py:232-313) ----
    @torch.no_grad()
    def submit(self, inputs=None, images=None, **kwargs):
        """Start one env's turn without waiting for it: same arguments as `generate`.  The turn joins the next `step_batch`
        iteration, sharing its pass over the weights with whatever the other envs in flight are doing (prefill or decode).
        `draft_ids` (or the env's previous output under set_auto_draft) is armed for the turn while set_batch_draft is on, and ignored
        otherwise.  Returns a ticket; the result arrives from `step_batch`."""
        draft = kwargs.pop("draft_ids", None)
        self._reject_group_request(kwargs, "submit")
        ids, pix, V, n_memory, env_id, past, max_new, eos = self._parse_call(inputs, images, kwargs)
        # refuse BEFORE the env's state changes (frames encoded, curr_t advanced, rows spliced): a turn the scheduler cannot take must
        # leave the env exactly as it was, so that the caller can retry it later
        if any(v[0] == env_id for v in self._tickets.values()):
            raise RuntimeError(f"env_id {env_id} already has a turn in flight")
        if len(self._tickets) >= 8:
            raise RuntimeError("at most 8 turns in flight: collect finished turns with step_batch first")
        self._sync_call_config()
        self._sync_sampling(kwargs)               # (a flip while other turns are in flight is refused by the engine: nothing has changed yet)
        on_dev = int(pix.is_cuda)
        if on_dev:
            self._order_engine_after(pix)
        _check(self._lib.svln_encode_frames(self._h, C.c_void_p(pix.data_ptr()), V, on_dev))
        if on_dev:
            self._order_torch_after(pix)
        self._begin_turn(env_id, past)
        ids_np = np.ascontiguousarray(ids.numpy())
        _check(self._lib.svln_append_turn(self._h, self._slot(env_id), ids_np.ctypes.data_as(C.POINTER(C.c_int64)), ids_np.size, n_memory))
        eos_np = np.asarray(eos, dtype=np.int64)
        slot = C.c_int32()
        self._arm_batch_draft(env_id, draft)
        _check(self._lib.svln_batch_submit(self._h, self._slot(env_id), min(max_new, self.cfg.max_positions),
                                           eos_np.ctypes.data_as(C.POINTER(C.c_int64)), eos_np.size, C.byref(slot)))
        self._tickets[slot.value] = (env_id, inputs)
        return SimpleNamespace(env_id=env_id, slot=slot.value)

    def _forced_array(self, forced):
        f_np = np.ascontiguousarray(torch.as_tensor(forced).reshape(-1).to("cpu", torch.int64).numpy())
        if not (1 <= int(f_np.size) <= 32):
            raise ValueError(f"forced_ids holds {int(f_np.size)} ids: a forced turn takes 1 .. 32")
        return f_np

    def _forced_precheck(self, env_id, f_np, eos):
        """the refusals of svln_batch_submit_forced that need no state of the env's rows, raised BEFORE a frame is encoded or a row spliced
        (its dry run: nothing is queued); the two that depend on the spliced length come with the submit itself, as svln_turn_forced's do"""
        eos_np = np.asarray(eos, dtype=np.int64)
        _check(self._lib.svln_batch_submit_forced(self._h, self._slot(env_id), f_np.ctypes.data_as(C.POINTER(C.c_int64)), int(f_np.size),
                                                  eos_np.ctypes.data_as(C.POINTER(C.c_int64)), eos_np.size, None))

    @torch.no_grad()
    def submit_forced(self, inputs=None, images=None, forced_ids=None, **kwargs):
        """`submit` for a FORCED turn (see _generate_forced): the turn's ids are forced_ids (1 .. 32).  The job shares the next `step_batch`
        iteration with whatever the other envs are doing and finishes in it -- one prefill pass that also feeds forced_ids[:-1], no decode
        iteration.  `max_new_tokens` is not read; `draft_ids` is armed as `submit` arms it and never used.  Nothing changes before a
        refusal.  Returns a ticket; `step_batch` returns the GenerateOutput `generate(forced_ids=...)` builds."""
        draft = kwargs.pop("draft_ids", None)
        if forced_ids is None:
            raise ValueError("submit_forced needs forced_ids")
        g = kwargs.get("num_return_sequences")
        if g is not None and int(g) > 1:
            raise NotImplementedError(f"num_return_sequences={g!r} in a submit_forced request: a forced turn has one sequence")
        if kwargs.get("candidate_ids") is not None:
            raise NotImplementedError("candidate_ids in a submit_forced request: candidates are scored through generate() only")
        if kwargs.get("fold_candidates"):
            raise NotImplementedError("fold_candidates in a submit_forced request: candidates are scored through generate() only")
        if kwargs.get("draft_set") is not None:
            raise NotImplementedError("draft_set in a submit_forced request: multi-draft turns run through generate() only")
        if kwargs.get("beam_width") is not None:
            raise NotImplementedError("beam_width in a submit_forced request: beam turns run through generate() only")
        f_np = self._forced_array(forced_ids)
        ids, pix, V, n_memory, env_id, past, max_new, eos = self._parse_call(inputs, images, kwargs)
        if any(v[0] == env_id for v in self._tickets.values()):
            raise RuntimeError(f"env_id {env_id} already has a turn in flight")
        if len(self._tickets) >= 8:
            raise RuntimeError("at most 8 turns in flight: collect finished turns with step_batch first")
        self._sync_call_config()
        held = self._sampling
        self._sync_sampling(kwargs)               # (a flip while other turns are in flight is refused by the engine: nothing has changed yet)
        try:
            self._forced_precheck(env_id, f_np, eos)
        except Exception:
            # a refused call changes no state: the sampling switch this call flipped goes back to what the engine held
            if self._sampling != held:
                self.set_sampling(None) if held is None else self._switch_sampling_on(*held)
            raise
        on_dev = int(pix.is_cuda)
        if on_dev:
            self._order_engine_after(pix)
        _check(self._lib.svln_encode_frames(self._h, C.c_void_p(pix.data_ptr()), V, on_dev))
        if on_dev:
            self._order_torch_after(pix)
        self._begin_turn(env_id, past)
        ids_np = np.ascontiguousarray(ids.numpy())
        _check(self._lib.svln_append_turn(self._h, self._slot(env_id), ids_np.ctypes.data_as(C.POINTER(C.c_int64)), ids_np.size, n_memory))
        eos_np = np.asarray(eos, dtype=np.int64)
        slot = C.c_int32()
        self._arm_batch_draft(env_id, draft)
        _check(self._lib.svln_batch_submit_forced(self._h, self._slot(env_id), f_np.ctypes.data_as(C.POINTER(C.c_int64)), int(f_np.size),
                                                  eos_np.ctypes.data_as(C.POINTER(C.c_int64)), eos_np.size, C.byref(slot)))
        self._tickets[slot.value] = (env_id, inputs)
        self._forced_tickets[slot.value] = f_np
        return SimpleNamespace(env_id=env_id, slot=slot.value, forced=True)

    def _forced_batch_result(self, slot, f_np):
        """the GenerateOutput of a finished forced job (the keys of _generate_forced); frees the engine slot"""
        n = int(f_np.size)
        PF, PI = C.POINTER(C.c_float), C.POINTER(C.c_int64)
        lp, glp, gid, m = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int64), C.c_int32()
        _check(self._lib.svln_batch_forced(self._h, slot, lp.ctypes.data_as(PF), gid.ctypes.data_as(PI), glp.ctypes.data_as(PF), n, C.byref(m)))
        if m.value != n:
            raise RuntimeError(f"the engine holds {m.value} forced log-probabilities for a forced turn of {n} ids")
        alp = None
        if self.allowed_token_ids:
            n_ids = len(self.allowed_token_ids)
            abuf, nt, ni = np.empty(n * n_ids, dtype=np.float32), C.c_int32(), C.c_int32()
            _check(self._lib.svln_batch_allowed_logprobs(self._h, slot, abuf.ctypes.data_as(PF), int(abuf.size), C.byref(nt), C.byref(ni)))
            if nt.value != n or ni.value != n_ids:
                raise RuntimeError(f"the engine holds {nt.value} x {ni.value} allowed log-probabilities for a forced turn of {n} ids over {n_ids} allowed ids")
            alp = torch.from_numpy(abuf.reshape(1, n, n_ids).copy())
        out, n_out, env = np.zeros(n, dtype=np.int64), C.c_int32(), C.c_int32()
        _check(self._lib.svln_batch_result(self._h, slot, C.byref(env), out.ctypes.data_as(PI), n, C.byref(n_out)))
        env_id, inputs = self._tickets.pop(slot)
        res = self._batch_result(env_id, out[: n_out.value], inputs)
        dev = res.sequences.device
        res["token_logprobs"] = torch.from_numpy(lp).unsqueeze(0).to(dev)
        res["greedy_ids"] = torch.from_numpy(gid).unsqueeze(0).to(dev)
        res["greedy_logprobs"] = torch.from_numpy(glp).unsqueeze(0).to(dev)
        if alp is not None:
            res["allowed_logprobs"] = alp.to(dev)
            res["allowed_token_ids"] = torch.tensor(self.allowed_token_ids, dtype=torch.int64, device=dev)
        return SimpleNamespace(env_id=env_id, slot=slot, forced=True), res

    @torch.no_grad()
    def generate_batch_forced(self, requests, max_new_tokens: int = 10000, eos_token_ids=None):
        """Several envs' turns executed together, forced and plain mixed: a request (kwargs dict as passed to `generate`, distinct env_id,
        at most 8) with a `forced_ids` key runs as a forced job (svln_batch_submit_forced), the others as plain ones (svln_batch_submit).
        The frames of the requests are encoded together, as generate_batch encodes them; then the call is the submits followed by
        `step_batch` until every turn is done.  Needs an idle scheduler; every refusal that needs no rows of an env comes before a frame is
        encoded.  `max_new_tokens` / `eos_token_ids` may differ between the plain requests.  Returns a list of GenerateOutput in request
        order: a forced request's is what generate(forced_ids=...) builds."""
        if not (1 <= len(requests) <= 8):
            raise ValueError("1..8 requests per batch")
        parsed, drafts, forced = [], [], []
        for r in requests:
            r = dict(r)
            f = r.pop("forced_ids", None)
            if r.get("candidate_ids") is not None:
                raise NotImplementedError("candidate_ids in a generate_batch_forced request: candidates are scored through generate() only")
            if r.get("fold_candidates"):
                raise NotImplementedError("fold_candidates in a generate_batch_forced request: candidates are scored through generate() only")
            if r.get("draft_set") is not None:
                raise NotImplementedError("draft_set in a generate_batch_forced request: multi-draft turns run through generate() only")
            g = r.get("num_return_sequences")
            if g is not None and int(g) > 1:
                raise NotImplementedError(f"num_return_sequences={g!r} in a generate_batch_forced request: group turns run through generate() only")
            forced.append(None if f is None else self._forced_array(f))
            drafts.append(r.pop("draft_ids", None))
            r.setdefault("max_new_tokens", max_new_tokens)
            if eos_token_ids is not None:
                r.setdefault("eos_token_ids", eos_token_ids)
            parsed.append((r,) + self._parse_call(r.pop("inputs", None), r.pop("images", None), r))
        if len({p[5] for p in parsed}) != len(parsed):
            raise ValueError("duplicate env_id in batch")
        if self._tickets:
            raise RuntimeError("generate_batch_forced needs an idle scheduler: collect or cancel the submitted turns first")
        self._sync_call_config()
        modes = {(bool(p[0].get("do_sample", False)), p[0].get("temperature")) if "do_sample" in p[0] else None for p in parsed}
        if len(modes) != 1:
            raise ValueError("do_sample / temperature must be the same for every request of a batch")
        held = self._sampling
        self._sync_sampling(parsed[0][0])
        try:
            for p, f in zip(parsed, forced):
                if f is not None:
                    self._forced_precheck(p[5], f, p[8])
        except Exception:
            # a refused call changes no state: the sampling switch this call flipped goes back to what the engine held
            if self._sampling != held:
                self.set_sampling(None) if held is None else self._switch_sampling_on(*held)
            raise
        # vision: encode the frames of as many requests as fit the frame buffer per call, then splice per env (generate_batch's loop)
        i = 0
        while i < len(parsed):
            j, frames = i, 0
            while j < len(parsed) and (j == i or frames + parsed[j][3] <= self.max_frames):
                frames += parsed[j][3]
                j += 1
            if frames > self.max_frames:
                raise ValueError(f"a request has {frames} frames but the engine was built with max_frames={self.max_frames}")
            pix = torch.cat([p[2] for p in parsed[i:j]], 0).contiguous()
            on_dev = int(pix.is_cuda)
            if on_dev:
                self._order_engine_after(pix)
            _check(self._lib.svln_encode_frames(self._h, C.c_void_p(pix.data_ptr()), frames, on_dev))
            if on_dev:
                self._order_torch_after(pix)
            base = 0
            for (_, ids, _, V, n_memory, env_id, past, _, _) in parsed[i:j]:
                self._begin_turn(env_id, past)
                ids_np = np.ascontiguousarray(ids.numpy())
                _check(self._lib.svln_append_turn_at(self._h, self._slot(env_id), ids_np.ctypes.data_as(C.POINTER(C.c_int64)), ids_np.size, base, n_memory))
                base += V
            i = j
        slot_of = {}
        try:
            for k, (p, d, f) in enumerate(zip(parsed, drafts, forced)):
                env_id, max_new = p[5], p[7]
                self._arm_batch_draft(env_id, d)
                eos_np = np.asarray(p[8], dtype=np.int64)
                eos_p, slot = eos_np.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32()
                if f is None:
                    _check(self._lib.svln_batch_submit(self._h, self._slot(env_id), min(max_new, self.cfg.max_positions), eos_p, eos_np.size, C.byref(slot)))
                else:
                    _check(self._lib.svln_batch_submit_forced(self._h, self._slot(env_id), f.ctypes.data_as(C.POINTER(C.c_int64)), int(f.size), eos_p,
                                                              eos_np.size, C.byref(slot)))
                    self._forced_tickets[slot.value] = f
                self._tickets[slot.value] = (env_id, requests[k].get("inputs"))
                slot_of[slot.value] = k
            res = [None] * len(requests)
            while any(x is None for x in res):
                done, _ = self.step_batch()
                for t, out in done:
                    res[slot_of[t.slot]] = out
        except Exception:
            if self._tickets:
                self.cancel()
            raise
        return res

    def batch_forced_stats(self, reset: bool = False):
        """counters of the scheduler's forced jobs: jobs finished, rows they fed (n - 1 each), EPI_TARGET head chunks launched"""
        v = [C.c_int64() for _ in range(3)]
        _check(self._lib.svln_batch_forced_stats(self._h, *[C.byref(x) for x in v], int(reset)))
        return {"jobs": v[0].value, "rows_fed": v[1].value, "head_launches": v[2].value}

    @torch.no_grad()
    def step_batch(self):
        """One scheduler iteration (one pass over the weights for every turn in flight).  Returns (finished, running): `finished` is
        a list of (ticket, GenerateOutput) for the turns that ended in this iteration, `running` the number still in flight."""
        running, nf = C.c_int32(), C.c_int32()
        fin = (C.c_int32 * 8)()
        try:
            _check(self._lib.svln_batch_step(self._h, C.byref(running), fin, C.byref(nf)))
        except Exception:
            # the engine has dropped the failing turn(s); drop the rest too so that tickets and engine slots cannot disagree
            self._lib.svln_batch_cancel(self._h, -1)
            self._tickets.clear()
            self._forced_tickets.clear()
            raise
        done = []
        cap = self.cfg.max_positions
        for k in range(nf.value):
            if fin[k] in self._forced_tickets:
                done.append(self._forced_batch_result(fin[k], self._forced_tickets.pop(fin[k])))
                continue
            out = np.zeros(cap, dtype=np.int64)
            n, env = C.c_int32(), C.c_int32()
            scores = None
            if self._token_scores:             # (valid until svln_batch_result frees the slot; a turn holds at most max_new <= cap ids)
                ns = C.c_int32()
                sbuf = np.empty(cap, dtype=np.float32)
                _check(self._lib.svln_batch_scores(self._h, fin[k], sbuf.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(ns)))
                scores = torch.from_numpy(sbuf[: ns.value].copy()).unsqueeze(0)
            top = self._topk(int(ns.value), "cpu", self._lib.svln_batch_topk, fin[k]) if self.top_logprobs_k else None
            ent = self._scores(self._lib.svln_batch_entropy, fin[k], n_new=int(ns.value), device="cpu") if self._token_entropy else None
            alp = None
            if self._token_scores and self.allowed_token_ids:      # (read before svln_batch_result frees the slot)
                abuf = np.empty(cap * len(self.allowed_token_ids), dtype=np.float32)
                nt, ni = C.c_int32(), C.c_int32()
                _check(self._lib.svln_batch_allowed_logprobs(self._h, fin[k], abuf.ctypes.data_as(C.POINTER(C.c_float)), int(abuf.size), C.byref(nt),
                                                             C.byref(ni)))
                alp = torch.from_numpy(abuf[: nt.value * ni.value].reshape(1, nt.value, ni.value).copy())
            _check(self._lib.svln_batch_result(self._h, fin[k], C.byref(env), out.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n)))
            env_id, inputs = self._tickets.pop(fin[k])
            res = self._batch_result(env_id, out[: n.value], inputs, scores)
            if top is not None:
                res["top_token_ids"], res["top_logprobs"] = (t.to(res.sequences.device) for t in top)
            if ent is not None:
                res["token_entropies"] = ent.to(res.sequences.device)
            if alp is not None:
                res["allowed_logprobs"] = alp.to(res.sequences.device)
                res["allowed_token_ids"] = torch.tensor(self.allowed_token_ids, dtype=torch.int64, device=res.sequences.device)
            done.append((SimpleNamespace(env_id=env_id, slot=fin[k]), res))
        return done, running.value

    def cancel(self, ticket=None):
        """Drop a submitted turn (ticket from `submit`), or every turn in flight (ticket=None)."""
        slot = -1 if ticket is None else int(ticket.slot)
        _check(self._lib.svln_batch_cancel(self._h, slot))
        if ticket is None:
            self._tickets.clear()
            self._forced_tickets.clear()
        else:
            self._tickets.pop(slot, None)
            self._forced_tickets.pop(slot, None)

    def last_hidden_batch(self, slot: int) -> np.ndarray:
        buf = np.empty((8, self.cfg.hidden), dtype=np.float32)
        n = C.c_int32()
        _check(self._lib.svln_get_hidden_batch(self._h, slot, buf.ctypes.data_as(C.POINTER(C.c_float)), 8, C.byref(n)))
        return buf[: n.value].copy()

    # ---- parity taps (tests) / perf helpers (bench) ---------------------------------------------------
    def last_hidden(self) -> np.ndarray:
        buf = np.empty((64, self.cfg.hidden), dtype=np.float32)
        n = C.c_int32()
        _check(self._lib.svln_get_hidden(self._h, buf.ctypes.data_as(C.POINTER(C.c_float)), 64, C.byref(n)))
        return buf[: n.value].copy()

    def set_layer_taps(self, enable: bool, probe_layer: int = -1):
        """test taps of the prefill: last residual row after every LLM layer; all rows around `probe_layer` (see include/streamvln_hip.h)"""
        _check(self._lib.svln_set_layer_taps(self._h, int(enable), int(probe_layer)))

    def layer_taps(self) -> np.ndarray:
        out = np.empty((self.cfg.layers, self.cfg.hidden), dtype=np.float32)
        _check(self._lib.svln_get_layer_taps(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def layer_probe(self, which: int, max_rows: int = 512) -> np.ndarray:
        """operand `which` of the probed layer as the last prefill saw it (0 x_in, 1 x_out, 2 attention out, 3 x after attention,
        4 post-attention norm, 5 SwiGLU product, 6 input norm, 7 the q|k|v buffer after RoPE -- q rotated, k / v as the product left them,
        the rotated k lives in the KV pages): fp32 [rows, cols].  The host buffer is sized by the probe's own width."""
        width = {2: self.cfg.q_dim, 5: self.cfg.inter, 7: self.cfg.q_dim + 2 * self.cfg.kv_dim}.get(int(which), self.cfg.hidden)
        out = np.empty(max_rows * width, dtype=np.float32)
        n, cols = C.c_int32(), C.c_int32()
        _check(self._lib.svln_get_layer_probe(self._h, int(which), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n), C.byref(cols)))
        return out[: n.value * cols.value].reshape(n.value, cols.value).copy()

    def env_state(self, env_id=0):
        ne, kl = C.c_int32(), C.c_int32()
        _check(self._lib.svln_env_state(self._h, self._slot(env_id), C.byref(ne), C.byref(kl)))
        return ne.value, kl.value

    def get_embeds(self, env_id, start, n) -> np.ndarray:
        out = np.empty((n, self.cfg.hidden), dtype=np.float32)
        _check(self._lib.svln_get_embeds(self._h, self._slot(env_id), start, n, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def preprocess_time(self, reset: bool = False):
        """(GPU ms, frames) spent in the image processor's HIP path since the last reset"""
        ms, n = C.c_double(), C.c_int64()
        _check(self._lib.svln_preprocess_time(self._h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def set_feature_cache(self, capacity_frames: int):
        """Memoise pooled frame features by pixel content (opt-in; 0 = re-encode every frame like the reference)."""
        _check(self._lib.svln_set_feature_cache(self._h, int(capacity_frames)))

    def feature_cache_stats(self):
        hits, misses = C.c_int64(), C.c_int64()
        _check(self._lib.svln_feature_cache_stats(self._h, C.byref(hits), C.byref(misses)))
        return hits.value, misses.value

    def set_decode_graph(self, enable: bool):
        _check(self._lib.svln_set_decode_graph(self._h, int(enable)))

    def set_decode_persistent(self, enable: bool):
        """single-env decode step as attention + ONE persistent launch per layer (svln_set_decode_persistent) instead of six launches"""
        _check(self._lib.svln_set_decode_persistent(self._h, int(enable)))

    def set_memory_prune(self, keep_tokens: int):
        """Opt-in extension (BASELINE configs[3]; no reference counterpart): `<memory>` expands to the `keep_tokens`
        memory tokens least similar to the mean memory token instead of all num_history x 196.  0 restores the reference behaviour."""
        _check(self._lib.svln_set_memory_prune(self._h, int(keep_tokens)))

    def set_fp8_decode(self, enable: bool):
        """Opt-in extension (the reference is bf16 only): decode steps and the lm_head read e4m3 copies of the LLM
        weights (per-row scale).  Prefill, vision and generate_batch keep bf16 (the batched paths have set_fp8_gemm and
        set_mxfp4_batched).  bf16 engines only; refused while set_mxfp4_decode or set_mxfp4_batched is on."""
        _check(self._lib.svln_set_fp8_decode(self._h, int(enable)))

    def set_mxfp4_decode(self, enable: bool):
        """Opt-in extension (the reference is bf16 only): decode steps and the lm_head read OCP MXFP4 copies of the LLM
        weights (E2M1 elements, one E8M0 scale per 32: 4.25 bits per weight).  Prefill and vision keep bf16; generate_batch and the
        scheduler keep bf16 too unless set_mxfp4_batched is on.  bf16 engines only; refused while set_fp8_decode is on (and the other
        way round)."""
        _check(self._lib.svln_set_mxfp4_decode(self._h, int(enable)))

    def set_packed_decode(self, enable: bool):
        """Lossless 12-bit packing of the bf16 weights that the single-env decode step's gate/up and down_proj GEMVs and the lm_head GEMV
        stream (svln_set_packed_decode): about 0.75 x the bytes, ids and hidden rows bit-identical.  On by default on bf16 engines;
        enabling is refused on fp32 engines.  set_fp8_decode / set_mxfp4_decode take precedence while they are on."""
        _check(self._lib.svln_set_packed_decode(self._h, int(enable)))

    def packed_stats(self):
        """{packed_bytes, bf16_bytes, blocks, fallback_blocks} over the packed weight matrices as encoded now (svln_packed_stats)"""
        v = [C.c_int64() for _ in range(4)]
        _check(self._lib.svln_packed_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("packed_bytes", "bf16_bytes", "blocks", "fallback_blocks"), (x.value for x in v)))

    def set_mxfp4_batched(self, enable: bool):
        """Opt-in extension (the reference is bf16 only): the decode steps of generate_batch / submit + step_batch (every batch size)
        and every lm_head product of the scheduler read the MXFP4 weight copies of set_mxfp4_decode on a weight-only MFMA kernel;
        prefill rows keep bf16, and an iteration that mixes prefill and decode rows is split so that each env is computed as in the
        single-env mode.  Independent of set_mxfp4_decode; bf16 engines only; refused while set_fp8_decode or set_fp8_gemm is on (and
        they are refused while it is on)."""
        _check(self._lib.svln_set_mxfp4_batched(self._h, int(enable)))

    def set_speculative(self, rows: int):
        """opt-in draft-verified greedy decode (svln_set_speculative): rows = 0 off, 2 / 4 / 8 = rows per verify pass.  Same ids as the
        plain greedy loop; a turn whose draft (generate(draft_ids=...) or set_auto_draft) is right takes one pass over the weights per
        `rows` tokens instead of one per token.  Refused while a reduced-precision or persistent decode mode is on."""
        _check(self._lib.svln_set_speculative(self._h, int(rows)))

    def set_auto_draft(self, enable: bool):
        """with no explicit draft_ids, generate() guesses that a turn repeats the env's previous turn; cleared by reset / reset_for_env"""
        self._auto_draft = bool(enable)
        self._last_out = {}

    def draft_stats(self, reset: bool = False):
        """(verify passes run, tokens they emitted, tokens emitted by ordinary decode steps) since the last reset"""
        v = [C.c_int64() for _ in range(3)]
        _check(self._lib.svln_draft_stats(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), int(reset)))
        return tuple(int(x.value) for x in v)

    def set_prefill_draft(self, enable: bool):
        """opt-in drafts inside the prefill pass (svln_set_prefill_draft): the first ids of a turn's draft (generate(draft_ids=...) or
        set_auto_draft) ride the prefill as extra rows, so a turn whose draft is right needs no decode pass at all.  Same ids as the plain
        greedy loop; independent of set_speculative.  Refused while a reduced-precision or persistent decode mode is on."""
        _check(self._lib.svln_set_prefill_draft(self._h, int(bool(enable))))

    def prefill_draft_stats(self, reset: bool = False):
        """(rides run, tokens they emitted -- token 0 included, draft rows they fed) since the last reset"""
        v = [C.c_int64() for _ in range(3)]
        _check(self._lib.svln_prefill_draft_stats(self._h, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), int(reset)))
        return tuple(int(x.value) for x in v)

    def drafts_stats(self):
        """counters of the multi-draft turns (generate(draft_set=...)) since the engine was created: (calls, passes run, tokens the passes
        emitted -- token 0 included, draft rows fed, turns finished in the pass, calls whose hints were ignored, page handovers, tokens of
        single steps)"""
        v = np.zeros(8, np.int64)
        _check(self._lib.svln_drafts_stats(self._h, v.ctypes.data_as(C.POINTER(C.c_int64))))
        return tuple(int(x) for x in v)

    def set_token_scores(self, enable: bool):
        """Opt-in, default off (svln_set_token_scores): while on, every GenerateOutput of generate / generate_batch / step_batch carries
        `token_logprobs`: fp32 [1, n_new] on the device of `sequences`, the log-probability (log softmax over the processed fp32 logits,
        after the repetition penalty) the model gave each id it emitted.  The lm_head kernels compute it beside their fused arg-max: no
        logits in memory, no second pass over the lm_head, the ids unchanged bit for bit.  While off the key is absent.  HF's
        `output_scores` / `output_logits` stay ignored: a [n_new, vocab] tensor is exactly what this engine exists not to build.
        Refused with set_speculative / set_prefill_draft / set_batch_draft, set_decode_persistent and set_mxfp4_batched (and they while
        it is on), and while scheduler turns are in flight."""
        _check(self._lib.svln_set_token_scores(self._h, int(bool(enable))))
        self._token_scores = bool(enable)

    def set_token_entropy(self, enable: bool):
        """Opt-in, default off (svln_token_entropy): while on, every GenerateOutput of generate / generate_batch / step_batch carries
        `token_entropies`: fp32 [1, n_new] on the device of `sequences`, aligned with it -- the entropy H = -sum_n p_n log p_n, in nats, of
        the distribution every id was taken from: softmax over the processed fp32 logits (after the repetition penalty), of logits / T under
        sampling, over the allowed set under set_allowed_tokens.  The lm_head kernels carry one more running sum beside their fused
        arg-max: no logits in memory, no second pass, ids and scores unchanged bit for bit.  Needs set_token_scores(True) first (which then
        cannot be switched off); refused together with set_top_logprobs(k > 0) and a sampling truncation, and group, beam, candidate and
        forced turns are refused while on (ValueError from the engine, naming the function)."""
        _check(self._lib.svln_token_entropy(self._h, int(bool(enable))))
        self._token_entropy = bool(enable)

    def set_top_logprobs(self, k: int):
        """Opt-in, default off (svln_top_logprobs; `logprobs=k` / `top_logprobs` of the serving stacks): while 1 <= k <= 8 every result of
        generate / generate_batch / step_batch carries `top_token_ids` int64 [1, n_new, k] and `top_logprobs` fp32 [1, n_new, k] on the device of `sequences`: per emitted
        id the k most probable ids (log-probability descending, then id ascending; under set_sampling of softmax(x / T), without the
        noise) -- padded with (-1, -inf) where fewer exist, e.g. under a shorter allowed list.  Greedy: entry 0 is the emitted id and its
        log-probability the bits of `token_logprobs`.  The lm_head kernels keep the candidates beside their fused arg-max: no logits in
        memory, no second pass, ids and scores unchanged bit for bit.  Needs set_token_scores(True) first (which then cannot be switched
        off); generate, generate_batch and step_batch carry the lists; group turns are refused while k > 0; a forced turn carries none.
        k = 0: off, the entries read as None."""
        _check(self._lib.svln_top_logprobs(self._h, int(k)))
        self.top_logprobs_k = int(k)

    def set_allowed_tokens(self, ids, add_eos: bool = True):
        """Opt-in, default off (svln_set_allowed_tokens; HF's prefix_allowed_tokens_fn with a constant set, vLLM's allowed_token_ids): while a
        list is set every turn chooses its ids among the listed ones only -- the lm_head product runs over those <= 256 weight rows
        instead of the whole vocabulary, and the arg-max, the sample and `token_logprobs` are taken over the processed logits of the set
        (HF's semantics when a logits processor puts -inf elsewhere).  `ids`: None or empty switches it off; otherwise the list is sorted,
        de-duplicated and, with add_eos (the default), joined with the generation config's EOS ids that lie in the vocabulary -- a list
        without an EOS id ends every turn at max_new_tokens.  The list in force is `self.allowed_token_ids` (a tuple; None when off).
        With set_token_scores on as well, every result of generate / generate_batch / step_batch carries `allowed_logprobs`, fp32
        [1, n_new, n_allowed] on the device of `sequences` -- log softmax over the allowed set for every emitted id -- and
        `allowed_token_ids`, int64 [n_allowed], the columns.  Composes with every other switch; refused while scheduler turns are in
        flight."""
        want = sorted({int(i) for i in ids}) if ids is not None else []
        if not want:
            _check(self._lib.svln_set_allowed_tokens(self._h, None, 0))
            self.allowed_token_ids = None
            return
        if add_eos:
            eos = self.generation_config.eos_token_id
            eos = eos if isinstance(eos, (list, tuple)) else [eos]
            want = sorted(set(want) | {int(e) for e in eos if e is not None and 0 <= int(e) < self.cfg.vocab})
        arr = np.asarray(want, dtype=np.int64)
        _check(self._lib.svln_set_allowed_tokens(self._h, arr.ctypes.data_as(C.POINTER(C.c_int64)), int(arr.size)))
        self.allowed_token_ids = tuple(want)

    @staticmethod
    def _check_truncation(top_k, top_p):
        """(top_k, top_p) -> None (off) or the pair the engine takes; the engine's own refusals, raised before any switch"""
        k = 0 if top_k is None else int(top_k)
        p = 1.0 if top_p is None else float(top_p)
        if not 0 <= k <= 8:
            raise ValueError(f"set_sampling_truncation: top_k must be None / 0 (off) or 1 .. 8, got {top_k!r}")
        if not (0.0 < p <= 1.0):
            raise ValueError(f"set_sampling_truncation: top_p must lie in (0, 1], got {top_p!r}")
        if k == 0 and p < 1.0:
            raise ValueError(f"set_sampling_truncation: top_p={top_p!r} needs top_k = 1 .. 8 (the nucleus is taken over at most 8 listed ids)")
        return (k, p) if k else None

    def _switch_sampling_on(self, t, sd):
        """the engine switch, then self.sampling_truncation (an "on" call keeps the engine's truncation; applying it again changes nothing)"""
        tr = self._check_truncation(*(self.sampling_truncation or (None, None)))
        _check(self._lib.svln_set_sampling(self._h, 1, t, sd & 0xFFFFFFFFFFFFFFFF))
        self._sampling = (t, sd)
        _check(self._lib.svln_sampling_truncation(self._h, *(tr or (0, 1.0))))

    def set_sampling_truncation(self, top_k: Optional[int] = None, top_p: Optional[float] = None):
        """Opt-in, default off (svln_sampling_truncation): truncated sampling, an attribute of set_sampling.  top_k in 1 .. 8, top_p in
        (0, 1] (with a top_k); no argument, or top_k None / 0 with top_p None / 1: off.  HF's warper order -- temperature, then the top_k
        most probable ids (an exact tie on the k-th value keeps the lowest ids, exactly k; HF keeps every tied id), then the smallest
        prefix of those whose mass under their own softmax reaches top_p.  The id is the untruncated sample conditioned on the kept set
        (the same noise: whenever the untruncated id is kept, it is the id), and `token_logprobs` / `top_logprobs` are taken over the
        kept set (HF's `scores` after the warpers; as under an allowed list).  The pair is held in self.sampling_truncation (None: off)
        and applied whenever Python switches sampling on -- set_sampling(T, seed) and the automatic flip of generate(do_sample=True),
        as self.sampling_seed is; while sampling is on, this call applies it at once (the draw counters go on).  set_sampling(None)
        clears it in the engine, not on the model.  Per-call `top_k=` / `top_p=` keys of generate stay refused.  Forced turns score the
        untruncated softmax.  Refused (nothing changes) on bad values, while scheduler turns are in flight and while a group is pending."""
        tr = self._check_truncation(top_k, top_p)
        if self._sampling is not None:
            _check(self._lib.svln_sampling_truncation(self._h, *(tr or (0, 1.0))))
        self.sampling_truncation = tr

    def set_sampling(self, temperature: Optional[float] = 1.0, seed: int = 0):
        """Opt-in, default off (svln_set_sampling).  set_sampling(T, seed): every turn samples its ids from softmax(processed logits / T)
        instead of taking the arg-max -- exactly, by the Gumbel-max identity: the lm_head kernels add noise G(seed, env slot, draw, column)
        to logit / T inside their fused arg-max, so there are still no logits in memory and no second pass over the lm_head.  The noise
        is a pure function of those four, so generate, generate_batch and the scheduler emit the same ids for the same seed wherever
        their logits agree, and a run is reproducible.  `draw` counts the ids the env has emitted since this call: EVERY call, also
        one that repeats the current setting, restarts the counters.  With set_token_scores on, `token_logprobs` is
        log softmax(processed / T)[id] (HF's `scores` under sampling).  set_sampling(None): off, the greedy path.
        Truncated (top-k / top-p) sampling is set_sampling_truncation: the pair it holds is applied after every switch-on here.
        generate / generate_batch / submit flip the switch themselves from `do_sample=` / `temperature=` (see _sync_sampling), with
        self.sampling_seed as the seed.  An explicit `do_sample=False` -- StreamingAgent's default request carries it -- switches the
        engine back to greedy: set_sampling alone samples only for calls that pass do_sample=True or leave the key out; build the agents
        with do_sample=True.  Refused with set_speculative / set_prefill_draft / set_batch_draft, set_decode_persistent and
        set_mxfp4_batched (and they while it is on), and while scheduler turns are in flight."""
        if temperature is None:
            _check(self._lib.svln_set_sampling(self._h, 0, 1.0, 0))
            self._sampling = None
            return
        t, sd = float(temperature), int(seed)
        if not (t > 0 and np.isfinite(t)):
            raise ValueError(f"set_sampling: the temperature must be finite and > 0, got {temperature!r}")
        self._switch_sampling_on(t, sd)

    def set_batch_draft(self, enable: bool):
        """opt-in drafts in the scheduler's prefill pass (svln_set_batch_draft): the first ids of a turn's draft (`draft_ids` of submit /
        of a generate_batch request, or set_auto_draft) ride the prefill rows of that env's segment, so a lockstep turn whose drafts
        are all right is one scheduler iteration.  Same ids as the plain scheduler on the fp32 engine; independent of set_speculative
        and set_prefill_draft; refused with the reduced-precision / persistent decode modes and while turns are in flight."""
        _check(self._lib.svln_set_batch_draft(self._h, int(bool(enable))))
        self._batch_draft = bool(enable)

    def batch_draft_stats(self, reset: bool = False):
        """(rides run, tokens they emitted -- token 0 included, draft rows they fed, scheduler iterations, decode rows fed one token at
        a time) since the last reset"""
        v = [C.c_int64() for _ in range(5)]
        _check(self._lib.svln_batch_draft_stats(self._h, *[C.byref(x) for x in v], int(reset)))
        return tuple(int(x.value) for x in v)

    def set_fp8_gemm(self, enable: bool):
        """Opt-in extension (SURVEY.md 8f-2 / BASELINE configs[4]): the LLM's multi-row products (prefill; decode steps of >= 4 batched
        envs) run as e4m3 MFMA products with per-row weight and activation scales.  bf16 engines only; reduced precision."""
        _check(self._lib.svln_set_fp8_gemm(self._h, int(enable)))

    def set_fp8_scaled_mfma(self, enable: bool):
        """Opt-in, default off: the products of set_fp8_gemm run on the block-scaled e4m3 MFMAs (neutral block scales: the same e4m3
        bytes, per-row scales and fp32 sums at twice the MFMA rate) and may take the 8-phase 256x256 schedule.  No effect while
        set_fp8_gemm is off; bf16 engines only; a change is refused while scheduler turns are in flight."""
        _check(self._lib.svln_set_fp8_scaled_mfma(self._h, int(enable)))

    def sync(self):
        _check(self._lib.svln_sync(self._h))

    def close(self):
        if getattr(self, "_h", None):
            proc = self._tower.image_processor
            if proc._ext_stream is not None:       # nothing on the torch side may still be ordered against the engine's stream
                dev = proc._ext_stream.device
                proc._ext_stream.synchronize()
                torch.cuda.current_stream(dev).synchronize()
                if torch.cuda.current_stream(dev).cuda_stream == proc._ext_stream.cuda_stream:
                    # the caller adopted the engine's stream (`torch_stream`): it is about to be destroyed, so torch goes back to its
                    # default stream (a later collective or kernel on a destroyed stream fails with hipErrorInvalidValue)
                    torch.cuda.set_stream(torch.cuda.default_stream(dev))
                proc._ext_stream = None
            proc._engine = None
            proc.backend = "closed"
            self._lib.svln_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
