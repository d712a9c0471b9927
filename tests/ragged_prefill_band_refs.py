"""Banded float64 reference and shared inputs for the `ragged_prefill_gqa`
tests. `ragged_prefill_band_ref` is ragged_prefill_refs.ragged_prefill_ref with
two changes: the admissible set is pos - window < col <= pos, and L in the
bound is the visible key count min(pos + 1, window). Same ds, eta, slack and
bf16_tol; nothing is tuned. With window >= kv_len it is ragged_prefill_ref."""
import functools
import math

import torch

from attn_refs import HALF_BF16, SENT
from edge_refs import EPI, U24, bf16_tol
from ragged_prefill_refs import MIXED, make_ragged_prefill, ragged_prefill_ref

# all 14 slots; with G = 3, (11, 43) is a 33-column sequence
BAND_PAIRS = MIXED + [(11, 43), (3, 200)]


def ragged_prefill_band_ref(q, kpool, vpool, seqs, window):
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
        col = torch.arange(kv_len, device=dev).view(1, -1)
        adm = (col <= pos.view(-1, 1)) & (col > pos.view(-1, 1) - window)
        L = (pos + 1).clamp(max=window).double().view(1, -1, 1)   # [1,q,1]
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


def greedy_no_cache(model, prompt, new):
    ids = prompt.view(1, -1)
    for _ in range(new):
        nxt = model(ids)[0, -1].float().argmax()
        ids = torch.cat([ids, nxt.view(1, 1)], dim=1)
    return ids[0]


@functools.lru_cache(maxsize=None)
def band_case(G, D, Hk, window, device):
    """BAND_PAIRS with poisoned pools, computed once and shared; callers must
    not modify it. Under a window (0 = none) K and V are also NaN below each
    sequence's lowest visible position lo(token 0), and V carries SENT at
    lo(token 0), at lo(last token) and just below it. The reference reads the
    same pools with NaN replaced by 0."""
    q, kp, vp, seqs = make_ragged_prefill(BAND_PAIRS, G, D, Hk, device=device)
    if window:
        for slot, _, q_len, kv_len in seqs:
            lo0 = max(0, kv_len - q_len - window + 1)
            kp[slot, :lo0] = float("nan")
            vp[slot, :lo0] = float("nan")
            vp[slot, lo0] = SENT
            vp[slot, max(0, kv_len - window)] = SENT
            if kv_len - 1 - window >= 0:
                vp[slot, kv_len - 1 - window] = SENT
    k0, v0 = torch.nan_to_num(kp, nan=0.0), torch.nan_to_num(vp, nan=0.0)
    ref = ragged_prefill_band_ref(q, k0, v0, seqs, window) if window \
        else ragged_prefill_ref(q, k0, v0, seqs)
    return q, kp, vp, seqs, ref
