"""Continuous batching serving engine (inference v2).

Parity: reference `inference/v2/ragged/*` + `mii` continuous batching:
requests enter and leave the running batch at token granularity — new
prompts prefill into free KV slots while in-flight sequences keep
decoding; every decode step runs ONE batched forward over all active
slots at their individual sequence lengths.

MI355X-native design: the KV pool is one tensor per layer
`[max_batch, max_seq, Hk, D]` (288 GB of HBM3E holds thousands of 8B
slots — paged/blocked KV is not needed to avoid fragmentation at this
scale, so slot granularity keeps the layout hipGraph-friendly). Ragged
lengths are handled with per-row RoPE positions (`positions` arg). On the
GPU (bf16, head_dim 64/128) decode attention runs the `ragged_decode` HIP
kernel straight over the pool; elsewhere an additive length mask goes
through SDPA.

`fused_step=True` (opt-in) is Dynamic SplitFuse proper: every step packs
its prefill chunks and one token per decoding request into ONE ragged
model call, described by a `RaggedBatch` and served by the
`ragged_prefill` HIP kernel, so the weights are read once per step.

`fused_kv_append=True` (opt-in) replaces, on the fused step and on the
batched decode step, the eager per-row RoPE of q and k and the pool / length
index_puts of every layer by one `ragged_rope_append` HIP launch.

`kv_dtype="fp8"` (opt-in, needs `fused_kv_append=True`, head_dim 64/128)
keeps the pool as OCP e4m3fn codes `[B, Smax, Hk, D]` plus one fp32 scale per
(slot, position, kv head): D + 4 bytes per cached row instead of 2 D. The
append quantizes (`ragged_rope_append_fp8`), decode and the fused step read
codes and scales directly (`ragged_decode_fp8`, `ragged_prefill_fp8`).
"""
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from .ragged_batch import RaggedBatch


@dataclass
class Request:
    prompt: torch.Tensor                 # 1-D token ids
    max_new_tokens: int = 32
    eos_token_id: Optional[int] = None
    temperature: float = 0.0             # 0 = greedy
    top_k: int = 0
    top_p: float = 1.0
    rid: int = -1
    slot: int = -1
    generated: List[int] = field(default_factory=list)
    done: bool = False

    @property
    def tokens(self):
        return torch.cat([self.prompt,
                          torch.tensor(self.generated,
                                       dtype=self.prompt.dtype)])


class RaggedKVCache:
    """One layer's slot-granular KV pool with per-slot lengths."""

    def __init__(self, max_batch, max_seq, n_kv, d, dtype, device,
                 rope=None, fp8=False):
        # fp8: e4m3fn codes plus one fp32 scale per (slot, position, kv head)
        # row -- ops.functional.kv_quantize. Needs `rope` (every ragged step
        # appends through rope_append) and head_dim 64 / 128.
        self.fp8 = fp8
        self.k_scale = self.v_scale = None
        if fp8:
            if rope is None:
                raise ValueError("fp8 KV pool needs fused_kv_append=True")
            if d not in (64, 128):
                raise ValueError("fp8 KV pool: head_dim must be 64 or 128, "
                                 f"got {d}")
            self.k_scale = torch.ones(max_batch, max_seq, n_kv,
                                      dtype=torch.float32, device=device)
            self.v_scale = torch.ones_like(self.k_scale)
        self.k = torch.zeros(max_batch, max_seq, n_kv, d,
                             dtype=torch.uint8 if fp8 else dtype,
                             device=device)
        self.v = torch.zeros_like(self.k)
        if fp8:                              # byte 0 is the code of 0.0
            self.k = self.k.view(torch.float8_e4m3fn)
            self.v = self.v.view(torch.float8_e4m3fn)
        self.lens = torch.zeros(max_batch, dtype=torch.long, device=device)
        self.rows = None        # active slot ids for this forward
        self.attn_mask = None
        # (kpool, vpool, rows, lens) for HIP decode; fp8: (kpool, vpool,
        # k_scale, v_scale, rows, lens)
        self.ragged = None
        self._prefill_slot = None
        self._prefill_off = 0   # chunked (SplitFuse-style) prefill offset
        self.fused = None       # RaggedBatch of a fused (one-call) step
        # fused_kv_append: full fp32 (cos, sin) tables [P, D/2]; the ragged
        # steps then go through rope_append() instead of RoPE + update()
        self.rope = rope
        self.pos = None         # decode: position of each row's new token
        self.new_lens = None    # decode: pos + 1, shared by all layers
        # ragged decode HIP kernel reads straight from the pool — no
        # per-token gather copies (ref inference/v2 ragged_ops role)
        from ..ops.loader import get_ext
        self._use_ragged = (device is not None
                            and torch.device(device).type == "cuda"
                            and dtype == torch.bfloat16
                            and d in (64, 128)
                            and get_ext(required=False) is not None)

    # -- model-facing update ------------------------------------------------
    @property
    def fuses_rope(self):
        """True on the steps rope_append() serves: the fused step and the
        batched decode step. Prompt prefill keeps RoPE + update()."""
        return self.rope is not None and (
            self.fused is not None
            or (self._prefill_slot is None and self.rows is not None))

    def rope_append(self, q, k, v):
        """RoPE of q and k plus update() in one `ragged_rope_append` call.
        Takes the un-rotated projections, returns (q_rot, k, v) with k/v as
        update() returns them (unused where attention reads the pool)."""
        from ..ops.functional import (ragged_rope_append,
                                      ragged_rope_append_fp8)
        cos, sin = self.rope
        if self.fp8:
            def append(q, k, v, slot, pos):
                return ragged_rope_append_fp8(
                    q, k, v, cos, sin, slot, pos, self.k, self.v,
                    self.k_scale, self.v_scale, self.lens)
        else:
            def append(q, k, v, slot, pos):
                return ragged_rope_append(q, k, v, cos, sin, slot, pos,
                                          self.k, self.v, self.lens)
        if self.fused is not None:           # [1, T, H, D] packed tokens
            b = self.fused
            q = append(q[0], k[0], v[0], b.tok_slot, b.tok_pos)
            self.ragged = None
            self.attn_mask = None
            return q.unsqueeze(0), k, v
        rows, pos = self.rows, self.pos      # decode: [n, 1, H, D]
        q = append(q[:, 0], k[:, 0], v[:, 0], rows, pos)
        q = q.unsqueeze(1)
        lens = self.new_lens
        if self.fp8:    # attention reads codes and scales; off the GPU the
            self.attn_mask = None            # fp8 op itself falls back
            self.ragged = (self.k, self.v, self.k_scale, self.v_scale, rows,
                           lens)
            return q, k, v
        if self._use_ragged:
            self.attn_mask = None
            self.ragged = (self.k, self.v, rows, lens)
            return q, k, v
        maxlen = int(lens.max())
        ar = torch.arange(maxlen, device=k.device)
        valid = ar.unsqueeze(0) < lens.unsqueeze(1)          # [n, maxlen]
        self.attn_mask = torch.where(
            valid, 0.0, float("-inf")).view(-1, 1, 1, maxlen).float()
        return q, self.k[rows, :maxlen], self.v[rows, :maxlen]

    def update(self, k, v):
        if self.fused is not None:           # [1, T, Hk, D] packed tokens
            b = self.fused
            self.k[b.tok_slot, b.tok_pos] = k[0]
            self.v[b.tok_slot, b.tok_pos] = v[0]
            self.lens[b.slots] = b.kv_lens
            self.ragged = None
            self.attn_mask = None
            return k, v  # attention reads the pool via ragged_prefill
        if self._prefill_slot is not None:   # [1, S, Hk, D] prompt chunk
            s = self._prefill_slot
            S = k.shape[1]
            o = self._prefill_off
            if self.fp8:                     # not the hot path: torch ops
                from ..ops.functional import kv_dequantize, kv_quantize
                self.k[s, o:o + S], self.k_scale[s, o:o + S] = \
                    kv_quantize(k[0])
                self.v[s, o:o + S], self.v_scale[s, o:o + S] = \
                    kv_quantize(v[0])
            else:
                self.k[s, o:o + S] = k[0]
                self.v[s, o:o + S] = v[0]
            self.lens[s] = o + S
            self.ragged = None
            if o == 0:
                self.attn_mask = None
                return k, v                  # causal prefill over itself
            # chunk at offset o attends to the cached prefix 0..o plus a
            # causal window within itself (Dynamic SplitFuse-style step)
            total = o + S
            q_pos = torch.arange(o, total, device=k.device).view(S, 1)
            k_pos = torch.arange(total, device=k.device).view(1, total)
            self.attn_mask = torch.where(k_pos <= q_pos, 0.0,
                                         float("-inf")) \
                .view(1, 1, S, total).to(torch.float32)
            if self.fp8:
                return (kv_dequantize(self.k[s:s + 1, :total],
                                      self.k_scale[s:s + 1, :total], k.dtype),
                        kv_dequantize(self.v[s:s + 1, :total],
                                      self.v_scale[s:s + 1, :total], v.dtype))
            return (self.k[s:s + 1, :total], self.v[s:s + 1, :total])
        rows = self.rows                     # decode: [n, 1, Hk, D]
        pos = self.lens[rows]
        self.k[rows, pos] = k[:, 0]
        self.v[rows, pos] = v[:, 0]
        self.lens[rows] = pos + 1
        lens = self.lens[rows]
        if self._use_ragged:
            self.attn_mask = None
            self.ragged = (self.k, self.v, rows.contiguous(),
                           lens.contiguous())
            return k, v  # attention reads from the pool via the kernel
        maxlen = int(lens.max())
        ar = torch.arange(maxlen, device=k.device)
        valid = ar.unsqueeze(0) < lens.unsqueeze(1)          # [n, maxlen]
        self.attn_mask = torch.where(
            valid, 0.0, float("-inf")).view(-1, 1, 1, maxlen).float()
        return self.k[rows, :maxlen], self.v[rows, :maxlen]


class ContinuousBatchingEngine:
    """Token-level continuous batching over a native model."""

    def __init__(self, model, max_batch=8, max_seq=None, device=None,
                 prefill_chunk=None, prefill_budget=None, fused_step=False,
                 fused_kv_append=False, kv_dtype=None):
        self.model = model
        cfg = model.cfg if hasattr(model, "cfg") else model.config
        self.cfg = cfg
        self.device = device or next(model.parameters()).device
        self.max_seq = max_seq or cfg.max_position_embeddings
        self.max_batch = max_batch
        dtype = next(model.parameters()).dtype
        # fused_kv_append (opt-in): the fused step and the decode step rotate
        # q/k and append K/V through one `ragged_rope_append` launch per
        # layer. The tables are the model's own buffers widened to fp32 --
        # the values the default path rotates with.
        self.fused_kv_append = fused_kv_append
        rope = None
        if fused_kv_append:
            core = next((m for m in model.modules()
                         if hasattr(m, "rope_cos")), None)
            if core is None:
                raise ValueError("fused_kv_append: the model has no "
                                 "rope_cos/rope_sin tables")
            rope = (core.rope_cos.to(self.device).float().contiguous(),
                    core.rope_sin.to(self.device).float().contiguous())
            if rope[0].shape[0] < self.max_seq:
                raise ValueError("fused_kv_append: max_seq exceeds the "
                                 "model's RoPE table")
        # kv_dtype (opt-in): None keeps the pool in the model's dtype; "fp8"
        # stores e4m3fn codes plus a per-row fp32 scale (half the bytes per
        # cached element, D + 4 bytes per row) and serves it with the
        # *_fp8 ragged kernels.
        if kv_dtype not in (None, "fp8", torch.float8_e4m3fn):
            raise ValueError(f"kv_dtype must be None or 'fp8', got "
                             f"{kv_dtype!r}")
        self.kv_fp8 = kv_dtype is not None
        if self.kv_fp8 and not fused_kv_append:
            raise ValueError("kv_dtype='fp8' needs fused_kv_append=True")
        self.caches = [RaggedKVCache(max_batch, self.max_seq,
                                     cfg.num_key_value_heads, cfg.head_dim,
                                     dtype, self.device, rope=rope,
                                     fp8=self.kv_fp8)
                       for _ in range(cfg.num_hidden_layers)]
        # Dynamic SplitFuse-style scheduling (ref FastGen): bound the
        # prompt tokens processed per step so long prompts stream in
        # chunks instead of stalling the decode batch. None = whole
        # prompt per step (legacy behavior). prefill_budget additionally
        # lets SEVERAL requests advance per step until the token budget
        # is spent (defaults to one chunk of one request).
        if prefill_budget and not prefill_chunk:
            prefill_chunk = prefill_budget  # budget implies chunking
        self.prefill_chunk = prefill_chunk
        self.prefill_budget = prefill_budget
        # fused_step: the step's prefill chunks and decode rows go through
        # ONE ragged model call instead of one call per chunk plus one for
        # the decode batch.
        if fused_step and not prefill_chunk:
            raise ValueError("fused_step=True needs prefill_chunk or "
                             "prefill_budget")
        self.fused_step = fused_step
        self.prefilling: List[Request] = []
        self.free_slots = list(range(max_batch))
        self.pending: List[Request] = []
        self.running: List[Request] = []
        self._next_rid = 0
        self._was_ckpt = getattr(cfg, "activation_checkpointing", False)
        cfg.activation_checkpointing = False

    def add_request(self, prompt, max_new_tokens=32, eos_token_id=None,
                    temperature=0.0, top_k=0, top_p=1.0):
        req = Request(prompt=prompt.to("cpu").long().view(-1),
                      max_new_tokens=max_new_tokens,
                      eos_token_id=eos_token_id, temperature=temperature,
                      top_k=top_k, top_p=top_p, rid=self._next_rid)
        self._next_rid += 1
        self.pending.append(req)
        return req.rid

    # -- internals ----------------------------------------------------------
    @torch.no_grad()
    def _prefill(self, req):
        if req.slot < 0:
            req.slot = self.free_slots.pop()
        for c in self.caches:
            c._prefill_slot = req.slot
        ids = req.prompt.view(1, -1).to(self.device)
        logits = self.model(ids, kv_caches=self.caches)
        for c in self.caches:
            c._prefill_slot = None
        req.generated.append(self._sample(logits[0, -1], req))
        self._check_done(req)

    @torch.no_grad()
    def _prefill_chunk_step(self, req):
        """Advance one request's prompt by at most prefill_chunk tokens;
        returns True when the prompt is fully ingested (and the first
        token sampled)."""
        pos = getattr(req, "prefill_pos", 0)
        n = len(req.prompt)
        take = min(self.prefill_chunk, n - pos)
        for c in self.caches:
            c._prefill_slot = req.slot
            c._prefill_off = pos
        ids = req.prompt[pos:pos + take].view(1, -1).to(self.device)
        logits = self.model(ids, kv_caches=self.caches, seq_offset=pos)
        for c in self.caches:
            c._prefill_slot = None
            c._prefill_off = 0
        req.prefill_pos = pos + take
        if req.prefill_pos >= n:
            req.generated.append(self._sample(logits[0, -1], req))
            self._check_done(req)
            return True
        return False

    @torch.no_grad()
    def _decode(self, active):
        rows = torch.tensor([r.slot for r in active], dtype=torch.long,
                            device=self.device)
        last = torch.tensor([[r.generated[-1]] for r in active],
                            dtype=torch.long, device=self.device)
        positions = self.caches[0].lens[rows].view(-1, 1)
        pos = positions.view(-1)
        new_lens = pos + 1 if self.fused_kv_append else None
        for c in self.caches:
            c.rows = rows
            c.pos = pos
            c.new_lens = new_lens
        logits = self.model(last, kv_caches=self.caches,
                            positions=positions)
        for c in self.caches:
            c.rows = None
            c.pos = None
            c.new_lens = None
        for r, row in zip(active, logits[:, -1]):
            r.generated.append(self._sample(row, r))
            self._check_done(r)

    @torch.no_grad()
    def _fused_step(self):
        """Prefill chunks (same budget loop as the unfused path) plus one
        token per running request, in one ragged model call."""
        chunks = []                          # (req, pos, take)
        budget = self.prefill_budget or self.prefill_chunk
        i = 0
        while i < len(self.prefilling) and budget > 0:
            req = self.prefilling[i]
            pos = req.prefill_pos
            take = 0
            # consecutive chunks of one prompt are one longer q range
            while budget > 0 and pos + take < len(req.prompt):
                c = min(self.prefill_chunk, len(req.prompt) - pos - take)
                budget -= c
                take += c
                if self.prefill_budget is None:
                    break  # one chunk of one request per step
            chunks.append((req, pos, take))
            if self.prefill_budget is None:
                break
            i += 1
        active = [r for r in self.running if not r.done]
        if not chunks and not active:
            return
        seqs, ids, sample = [], [], []       # sample: (req, token row)
        t = 0
        for req, pos, take in chunks:
            seqs.append((req.slot, t, take, pos + take))
            ids.append(req.prompt[pos:pos + take])
            t += take
            if pos + take >= len(req.prompt):
                sample.append((req, t - 1))
        for r in active:
            seqs.append((r.slot, t, 1, len(r.prompt) + len(r.generated)))
            ids.append(torch.tensor([r.generated[-1]], dtype=torch.long))
            sample.append((r, t))
            t += 1
        batch = RaggedBatch(seqs, self.max_batch, self.max_seq, self.device)
        for c in self.caches:
            c.fused = batch
        try:
            input_ids = torch.cat(ids).view(1, -1).to(self.device)
            # only rows that sample reach lm_head (none: an empty GEMM)
            rows = torch.tensor([i for _, i in sample], dtype=torch.long,
                                device=self.device)
            logits = self.model(input_ids, kv_caches=self.caches,
                                positions=batch.tok_pos.view(1, -1),
                                logits_rows=rows)
        finally:
            for c in self.caches:
                c.fused = None
        for req, pos, take in chunks:
            req.prefill_pos = pos + take
            if req.prefill_pos >= len(req.prompt):
                # by identity: Request.__eq__ would compare prompt tensors
                self.prefilling = [r for r in self.prefilling
                                   if r is not req]
                self.running.append(req)
        for i, (req, _) in enumerate(sample):
            req.generated.append(self._sample(logits[0, i], req))
            self._check_done(req)

    @staticmethod
    def _sample(logits, req):
        logits = logits.float()
        if req.temperature <= 0:
            return int(logits.argmax())
        logits = logits / req.temperature
        if req.top_k > 0:
            kth = torch.topk(logits, req.top_k).values[-1]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        probs = torch.softmax(logits, dim=-1)
        if req.top_p < 1.0:
            sp, idx = probs.sort(descending=True)
            cum = sp.cumsum(-1)
            keep = cum - sp < req.top_p  # keep until mass reaches top_p
            sp = sp * keep
            sp = sp / sp.sum()
            return int(idx[torch.multinomial(sp, 1)])
        return int(torch.multinomial(probs, 1))

    def _check_done(self, req):
        if len(req.generated) >= req.max_new_tokens or \
                (req.eos_token_id is not None
                 and req.generated[-1] == req.eos_token_id) or \
                len(req.prompt) + len(req.generated) >= self.max_seq:
            req.done = True

    # -- public loop --------------------------------------------------------
    @torch.no_grad()
    def step(self):
        """Admit + one decode step. Returns requests finished this step.

        With prefill_chunk set, at most ONE chunk of ONE prompt is
        ingested per step (bounded prefill work), interleaved with the
        decode batch — long prompts no longer stall running decodes.
        With fused_step the same chunks and the decode rows are ONE ragged
        model call; a prompt that completes starts decoding next step."""
        if self.prefill_chunk is None:
            while self.pending and self.free_slots:
                req = self.pending.pop(0)
                self._prefill(req)
                self.running.append(req)
        else:
            while self.pending and self.free_slots:
                req = self.pending.pop(0)
                req.slot = self.free_slots.pop()
                req.prefill_pos = 0
                self.prefilling.append(req)
            if self.fused_step:
                self._fused_step()
                return self._retire()
            budget = self.prefill_budget or self.prefill_chunk
            while self.prefilling and budget > 0:
                req = self.prefilling[0]
                remaining = len(req.prompt) - getattr(req, "prefill_pos", 0)
                budget -= min(self.prefill_chunk, remaining)
                if self._prefill_chunk_step(req):
                    self.prefilling.pop(0)
                    self.running.append(req)
                if self.prefill_budget is None:
                    break  # legacy: one chunk of one request per step
        active = [r for r in self.running if not r.done]
        if active:
            self._decode(active)
        return self._retire()

    def _retire(self):
        finished = [r for r in self.running if r.done]
        for r in finished:
            self.free_slots.append(r.slot)
        # by identity: Request.__eq__ would compare prompt tensors
        self.running = [r for r in self.running if not r.done]
        return finished

    def run(self, max_steps=10000):
        """Drain all pending/running requests; returns rid -> tokens."""
        out = {}
        steps = 0
        while (self.pending or self.prefilling or self.running) \
                and steps < max_steps:
            for r in self.step():
                out[r.rid] = r.tokens
            steps += 1
        return out

    def has_capacity(self):
        return bool(self.free_slots)

    def close(self):
        """Free the KV pool and restore the model's training config."""
        self.caches = []
        self.cfg.activation_checkpointing = self._was_ckpt

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
