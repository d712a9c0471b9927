"""float64 reference, derived bound and shared inputs for the ragged prefill
attention tests (conventions of attn_refs.py / edge_refs.py: nothing tuned).

A sequence is (slot, q_start, q_len, kv_len). Local token j lives at
q[q_start + j], has position p = kv_len - q_len + j and sees pool positions
0..p of its slot, i.e. L = p + 1 keys.

Bound, per token (derivation in the attn_refs docstring): ds and eta exactly
as in `attention_ref` with S -> L, INCLUDING the +8 deferred-max term, so an
eager or a deferred running max are both covered;
  slack = (2^-8 + eta + 4 * (L + D + EPI) * U24) * (P @ |V|)
where 2^-8 is P rounded to bf16 for the PV MFMA and 4 * (L + D + EPI) * U24
the ragged accumulate / rescale / merge term of `ragged_ref`; the final bf16
rounding comes from `bf16_tol`.
"""
import functools
import math

import torch

from attn_refs import HALF_BF16, RAGGED_LENS_A, SENT
from edge_refs import EPI, U24, bf16_tol

N_SLOTS, SMAX = 14, 300

# (q_len, kv_len): decode rows, fresh prompts (kv_len == q_len) on both sides
# of the 32-token q tile and the 64-row kv tile, chunks over a cached prefix
MIXED = [(1, 1), (1, 37), (5, 5), (31, 31), (32, 32), (33, 33), (33, 97),
         (64, 128), (65, 65), (1, 257), (40, 297), (96, 96)]
LONE = [(1, 1)]
DECODE = [(1, L) for L in RAGGED_LENS_A[:9]]
BATCHES = {"mixed": MIXED, "lone": LONE, "decode": DECODE}


def ragged_prefill_ref(q, kpool, vpool, seqs):
    """float64, per token. q [T,Hq,D], pools [B,Smax,Hk,D], seqs a list of
    (slot, q_start, q_len, kv_len). Returns out [T,Hq,D], slack and tol."""
    T, Hq, D = q.shape
    Hk = kpool.shape[2]
    G = Hq // Hk
    scale = 1.0 / math.sqrt(D)
    dev = q.device
    hmap = torch.arange(Hq, device=dev) // G
    out = torch.zeros(T, Hq, D, dtype=torch.float64, device=dev)
    slack = torch.zeros_like(out)
    for slot, q_start, q_len, kv_len in seqs:
        qs = q[q_start:q_start + q_len].double().transpose(0, 1)  # [Hq,q,D]
        kk = kpool[slot, :kv_len].double()[:, hmap].transpose(0, 1)
        vv = vpool[slot, :kv_len].double()[:, hmap].transpose(0, 1)
        pos = torch.arange(kv_len - q_len, kv_len, device=dev)
        adm = torch.arange(kv_len, device=dev).view(1, -1) <= pos.view(-1, 1)
        L = (pos + 1).double().view(1, -1, 1)                     # [1,q,1]
        s = qs @ kk.transpose(-1, -2) * scale                     # [Hq,q,kv]
        s_abs = qs.abs() @ kk.abs().transpose(-1, -2) * scale
        s = torch.where(adm, s, torch.full_like(s, float("-inf")))
        m = s.max(-1, keepdim=True).values
        p = torch.softmax(s, -1)                                  # 0 if masked
        o = p @ vv
        t = p @ vv.abs()
        zero = torch.zeros_like(s)
        gap = torch.where(adm, (s - m).abs(), zero)
        ds = U24 * ((D + EPI) * s_abs + 2.0 * (gap + 8.0))
        ds = torch.where(adm, ds, zero)
        eta = 2.0 * ds.max(-1, keepdim=True).values + (L + EPI) * U24
        sl = (HALF_BF16 + eta + 4.0 * (L + D + EPI) * U24) * t
        out[q_start:q_start + q_len] = o.transpose(0, 1)
        slack[q_start:q_start + q_len] = sl.transpose(0, 1)
    return dict(out=out, slack=slack, tol=bf16_tol(out, slack))


def make_ragged_prefill(pairs, G, D, Hk, n_slots=N_SLOTS, Smax=SMAX,
                        device="cpu", dtype=torch.bfloat16, poison=True,
                        seed=0):
    """q, pools and the sequence list for `pairs` of (q_len, kv_len), in the
    style of make_ragged. Slots are a random subset of the pool; q_start is
    assigned in a SHUFFLED order, not descriptor order. With `poison` both
    pools are NaN at every position >= kv_len of a named slot and everywhere
    in unnamed slots. V carries SENT at kv_len - 1 and at kv_len - q_len (the
    first new token's own column), so a dropped last column or a dropped
    diagonal fails."""
    g = torch.Generator().manual_seed(seed + 13 * G + D + Hk + 101 * len(pairs))
    n = len(pairs)
    Hq = G * Hk
    slots = torch.randperm(n_slots, generator=g)[:n].tolist()
    order = torch.randperm(n, generator=g).tolist()
    q_start = [0] * n
    t = 0
    for i in order:
        q_start[i] = t
        t += pairs[i][0]
    T = t
    hk = torch.arange(Hk).view(1, 1, Hk, 1)
    kpool = torch.randn(n_slots, Smax, Hk, D, generator=g) + 0.25 * (hk + 1)
    vpool = torch.randn(n_slots, Smax, Hk, D, generator=g) + 0.75 * (hk + 1)
    q = 0.5 * torch.randn(T, Hq, D, generator=g)
    fill = [0] * n_slots
    seqs = []
    for i, (q_len, kv_len) in enumerate(pairs):
        assert 1 <= q_len <= kv_len <= Smax
        seqs.append((slots[i], q_start[i], q_len, kv_len))
        fill[slots[i]] = kv_len
        vpool[slots[i], kv_len - 1] = SENT
        vpool[slots[i], kv_len - q_len] = SENT
    if poison:
        for s in range(n_slots):
            kpool[s, fill[s]:] = float("nan")
            vpool[s, fill[s]:] = float("nan")
    to = dict(device=device, dtype=dtype)
    return q.to(**to), kpool.to(**to), vpool.to(**to), seqs


@functools.lru_cache(maxsize=None)
def ragged_prefill_case(name, G, D, Hk, device):
    """Inputs and the float64 reference of one (batch, shape), computed once
    and shared; callers must not modify them."""
    q, kp, vp, seqs = make_ragged_prefill(BATCHES[name], G, D, Hk,
                                          device=device)
    return q, kp, vp, seqs, ragged_prefill_ref(q, kp, vp, seqs)
