"""Descriptor of one ragged serving step (prefill chunks + decode rows).

Parity: reference `inference/v2/ragged/ragged_wrapper.py` (RaggedBatchWrapper)
— the per-sequence "atoms" its blocked flash attention consumes. Here a
sequence is one row `(slot, q_start, q_len, kv_len)`: `q_len` packed tokens
starting at `q[q_start]`, attending to the first `kv_len` positions of KV
slot `slot` (kv_len counts this step's tokens). The `ragged_prefill` HIP
kernel cannot check descriptor CONTENT without a host sync, so it is
validated here, once per step, from Python ints before the upload.
`RaggedBatch` is the only supported way to produce a `desc`.
"""
import torch


class RaggedBatch:
    """Validated ragged batch.

    seqs: iterable of (slot, q_start, q_len, kv_len) Python ints.
    n_slots / max_seq: the pool's B and Smax.
    total_tokens: T of the packed q; defaults to sum(q_len).

    Holds `desc` [n,4] int64 on `device`, `max_qlen`, `max_kvlen`, and the
    per-token `tok_slot` / `tok_pos` int64 tensors [T] (used by the pool write
    and by RoPE).
    """

    def __init__(self, seqs, n_slots, max_seq, device="cpu",
                 total_tokens=None):
        seqs = [tuple(int(x) for x in s) for s in seqs]
        if not seqs:
            raise ValueError("RaggedBatch: no sequences")
        if any(len(s) != 4 for s in seqs):
            raise ValueError("RaggedBatch: each sequence is "
                             "(slot, q_start, q_len, kv_len)")
        T = sum(max(s[2], 0) for s in seqs) if total_tokens is None \
            else int(total_tokens)
        seen = set()
        for slot, q_start, q_len, kv_len in seqs:
            if not 0 <= slot < n_slots:
                raise ValueError(f"RaggedBatch: slot {slot} outside "
                                 f"[0, {n_slots})")
            if slot in seen:
                raise ValueError(f"RaggedBatch: slot {slot} appears twice")
            seen.add(slot)
            if q_len < 1:
                raise ValueError(f"RaggedBatch: q_len {q_len} < 1")
            if kv_len < q_len:
                raise ValueError(f"RaggedBatch: kv_len {kv_len} < q_len "
                                 f"{q_len}")
            if kv_len > max_seq:
                raise ValueError(f"RaggedBatch: kv_len {kv_len} exceeds the "
                                 f"pool's Smax {max_seq}")
        end = 0
        for _, q_start, q_len, _ in sorted(seqs, key=lambda s: s[1]):
            if q_start < end:
                raise ValueError("RaggedBatch: q ranges overlap (or start "
                                 f"below 0) at q_start {q_start}")
            if q_start > end:
                raise ValueError("RaggedBatch: q ranges leave a gap at "
                                 f"[{end}, {q_start})")
            end = q_start + q_len
        if end != T:
            raise ValueError(f"RaggedBatch: q ranges cover [0, {end}), "
                             f"not [0, {T})")
        self.seqs = seqs
        self.n = len(seqs)
        self.total_tokens = T
        self.n_slots = n_slots
        self.max_seq = max_seq
        self.max_qlen = max(s[2] for s in seqs)
        self.max_kvlen = max(s[3] for s in seqs)
        tok_slot = [0] * T
        tok_pos = [0] * T
        for slot, q_start, q_len, kv_len in seqs:
            tok_slot[q_start:q_start + q_len] = [slot] * q_len
            tok_pos[q_start:q_start + q_len] = range(kv_len - q_len, kv_len)
        # one upload: desc rows, then the two per-token vectors
        flat = [x for s in seqs for x in s] + tok_slot + tok_pos
        buf = torch.tensor(flat, dtype=torch.long).to(device)
        self.desc = buf[:4 * self.n].view(self.n, 4)
        self.tok_slot = buf[4 * self.n:4 * self.n + T]
        self.tok_pos = buf[4 * self.n + T:]
        # slot / kv_len columns for RaggedKVCache.lens
        self.slots = self.desc[:, 0]
        self.kv_lens = self.desc[:, 3]

    def last_rows(self):
        """Index in [0, T) of each sequence's last token, in seqs order."""
        return [s[1] + s[2] - 1 for s in self.seqs]
