"""The attention / ragged-decode bounds of attn_refs.py are VALID (a plain
torch emulation of what the kernels round stays inside them) and SHARP (the
emulation with one edge broken does not), on every case of the GPU
parametrisations. Runs without a GPU."""
import math

import pytest
import torch

from attn_refs import (ATTN_CASES, F32_MIN, RAGGED_CHUNKS, RAGGED_DUP,
                       RAGGED_LENS_A, RAGGED_LENS_B, RAGGED_SHAPES,
                       attention_ref, case_id, case_scale, check_attention,
                       make_inputs, make_ragged, ragged_ref)
from edge_refs import assert_within

BF = torch.bfloat16


def _r16(t):              # round to bf16, keep computing in fp32
    return t.to(BF).float()


def emulate_attention(q, k, v, causal, scale, kvmask, dout, mut=None,
                      fp32_grads=False):
    """What the kernels do, in plain torch: bf16 inputs, fp32 scores, P and
    dS rounded to bf16 before their matmuls, fp32 accumulation, Drow from the
    bf16 O, P recomputed from the saved fp32 lse, bf16 outputs. `mut` names
    one deliberately broken edge. fp32_grads: also return dq32 / dk32, the
    fp32 accumulators of dq / dk before their final rounding."""
    B, S, Hq, D = q.shape
    Hk = k.shape[2]
    G = Hq // Hk
    heads = torch.arange(Hq)
    hmap = heads % Hk if mut == "head_mod" else heads // G
    hd = lambda t: t.float().permute(0, 2, 1, 3)            # noqa: E731
    qf, kf, vf, do = hd(q), hd(k)[:, hmap], hd(v)[:, hmap], hd(dout)
    if mut == "batch0_kv":
        kf, vf = kf.clone(), vf.clone()
        kf[1], vf[1] = kf[0], vf[0]
    if mut == "default_scale":
        scale = 1.0 / math.sqrt(D)
    scale = float(torch.tensor(scale, dtype=torch.float32))
    s = (qf @ kf.transpose(-1, -2)) * scale
    adm = torch.ones(B, 1, S, S, dtype=torch.bool)
    if causal:
        adm = adm & torch.tril(torch.ones(S, S, dtype=torch.bool),
                               diagonal=-1 if mut == "causal_ge" else 0)
    if kvmask is not None and mut != "no_mask":
        mk = kvmask.float().view(B, 1, 1, S)
        adm = adm & (mk > F32_MIN)
        s = s + torch.where(mk > F32_MIN, mk, torch.zeros_like(mk))
        valid = kvmask > F32_MIN                            # [B,S]
    else:
        valid = torch.ones(B, S, dtype=torch.bool)
    drop = torch.zeros(B, S, dtype=torch.bool)
    for b in range(B):
        idx = torch.nonzero(valid[b]).flatten()
        if idx.numel() == 0:
            continue
        last = int(idx[-1])
        if mut == "drop_last":
            drop[b, last] = True
        if mut == "drop_tile_first":
            drop[b, 64 * (last // 64)] = True
    adm = (adm & ~drop.view(B, 1, 1, S)).expand(B, Hq, S, S)
    s = torch.where(adm, s, torch.full_like(s, float("-inf")))
    has = adm.any(-1)
    m = torch.where(has, s.max(-1).values, torch.zeros_like(s[..., 0]))
    p = torch.exp(s - m.unsqueeze(-1))
    l = p.sum(-1)
    lsafe = torch.where(has, l, torch.ones_like(l))
    out = ((_r16(p) @ vf) / lsafe.unsqueeze(-1)).to(BF)
    lse = torch.where(has, m + torch.log(lsafe),
                      torch.full_like(m, float("-inf")))
    # backward from the saved lse and the bf16 out
    sub = torch.where(has, lse, torch.full_like(lse, float("inf")))
    pb = torch.exp(s - sub.unsqueeze(-1))
    drow = (do * out.float()).sum(-1)
    dp = do @ vf.transpose(-1, -2)
    ds = pb * (dp - drow.unsqueeze(-1)) * scale
    dq32 = _r16(ds) @ kf
    dq = dq32.to(BF)
    dk_h = _r16(ds).transpose(-1, -2) @ qf                  # [B,Hq,S,D]
    dv_h = _r16(pb).transpose(-1, -2) @ do
    dk = torch.zeros(B, Hk, S, D)
    dv = torch.zeros(B, Hk, S, D)
    seen = set()
    for h in range(Hq):
        hk = int(hmap[h])
        if mut == "dkv_first_head" and hk in seen:
            continue
        seen.add(hk)
        dk[:, hk] += dk_h[:, h]
        dv[:, hk] += dv_h[:, h]
    perm = lambda t: t.permute(0, 2, 1, 3)                  # noqa: E731
    got = dict(out=perm(out), lse=lse, dq=perm(dq), dk=perm(dk).to(BF),
               dv=perm(dv).to(BF))
    if fp32_grads:
        got.update(dq32=perm(dq32), dk32=perm(dk))
    return got


# mutant -> which cases have the edge at all
MUTANTS = {
    "drop_last": lambda c: True,
    "drop_tile_first": lambda c: True,
    "no_mask": lambda c: c["mask"] is not None,
    "causal_ge": lambda c: c["causal"],
    "head_mod": lambda c: c["Hq"] > c["Hk"] > 1,
    "batch0_kv": lambda c: True,
    "default_scale": lambda c: c["custom"],
    "dkv_first_head": lambda c: c["Hq"] > c["Hk"],
}

_CACHE = {}


def _case(i):
    if i not in _CACHE:
        c = ATTN_CASES[i]
        q, k, v, do, mask = make_inputs(c)
        ref = attention_ref(q, k, v, c["causal"], case_scale(c), mask, do)
        _CACHE[i] = (q, k, v, do, mask, ref)
    return _CACHE[i]


@pytest.mark.parametrize("i", range(len(ATTN_CASES)),
                         ids=[case_id(c) for c in ATTN_CASES])
def test_emulation_within_bounds(i):
    c = ATTN_CASES[i]
    q, k, v, do, mask, ref = _case(i)
    assert not torch.isnan(ref["lse"]).any()
    got = emulate_attention(q, k, v, c["causal"], case_scale(c), mask, do)
    check_attention(got, ref, case_id(c))


def test_reference_matches_autograd():
    """The closed-form float64 gradients equal autograd's on a case where
    torch's own softmax is defined (no empty rows)."""
    c = ATTN_CASES[23]      # S257 D64 6x2 causal, tail mask
    q, k, v, do, mask, ref = _case(23)
    B, S, Hq, D = q.shape
    G = Hq // k.shape[2]
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    kk = kd.permute(0, 2, 1, 3).repeat_interleave(G, 1)
    vv = vd.permute(0, 2, 1, 3).repeat_interleave(G, 1)
    s = qd.permute(0, 2, 1, 3) @ kk.transpose(-1, -2) * case_scale(c)
    s = s + mask.double().view(B, 1, 1, S)
    s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1),
                      float("-inf"))
    o = (torch.softmax(s, -1) @ vv).permute(0, 2, 1, 3)
    o.backward(do.double())
    for name, got in (("out", o), ("dq", qd.grad), ("dk", kd.grad),
                      ("dv", vd.grad)):
        assert_within(got, ref[name], 1e-9 * (1 + ref[name].abs()), name)


def test_every_present_mutant_is_caught():
    pairs = skipped = 0
    missed = []
    for i, c in enumerate(ATTN_CASES):
        q, k, v, do, mask, ref = _case(i)
        args = (q, k, v, c["causal"], case_scale(c), mask, do)
        base = emulate_attention(*args)
        for mut, applies in MUTANTS.items():
            if not applies(c):
                continue
            pairs += 1
            got = emulate_attention(*args, mut=mut)
            if all(torch.equal(got[n].float().nan_to_num(),
                               base[n].float().nan_to_num()) for n in got):
                skipped += 1            # the broken edge is not in this case
                continue
            try:
                check_attention(got, ref, f"{case_id(c)} {mut}")
            except AssertionError:
                continue
            missed.append(f"{case_id(c)}: {mut}")
    print(f"mutants: {pairs} (case, mutant) pairs, {skipped} skipped as "
          f"'edge not present' ({100.0 * skipped / pairs:.1f} %)")
    assert not missed, "mutants inside the bounds:\n" + "\n".join(missed)
    assert skipped * 20 < pairs


# ------------------------------------------------------------ ragged decode
def emulate_ragged(q, kpool, vpool, rows, lens, chunk, mut=None):
    """fp32 throughout, split into chunks merged flash-decoding style."""
    n, _, Hq, D = q.shape
    Hk = kpool.shape[2]
    G = Hq // Hk
    heads = torch.arange(Hq)
    hmap = heads % Hk if mut == "head_mod" else heads // G
    scale = 1.0 / math.sqrt(D)
    out = torch.zeros(n, 1, Hq, D)
    for i in range(n):
        L, slot = int(lens[i]), int(rows[i])
        if mut == "drop_last":
            L -= 1
        if mut == "slot0":
            slot = int(rows[0])
        acc = torch.zeros(Hq, D)
        lsum = torch.zeros(Hq, 1)
        mrun = torch.full((Hq, 1), float("-inf"))
        for c0 in range(0, L, chunk):
            kk = kpool[slot, c0:min(L, c0 + chunk)].float()[:, hmap]
            vv = vpool[slot, c0:min(L, c0 + chunk)].float()[:, hmap]
            s = torch.einsum("hd,lhd->hl", q[i, 0].float() * scale, kk)
            mnew = torch.maximum(mrun, s.max(-1, keepdim=True).values)
            c = torch.exp(mrun - mnew)
            p = torch.exp(s - mnew)
            acc = acc * c + torch.einsum("hl,lhd->hd", p, vv)
            lsum = lsum * c + p.sum(-1, keepdim=True)
            mrun = mnew
        if L > 0:
            out[i, 0] = acc / lsum
    return out.to(BF)


@pytest.mark.parametrize("G,D,Hk", RAGGED_SHAPES)
def test_ragged_emulation_valid_and_sharp(G, D, Hk):
    for lens in (RAGGED_LENS_A, RAGGED_LENS_B):
        q, kp, vp, rows, ln = make_ragged(lens, RAGGED_DUP, G, D, Hk, 14, 300)
        ref = ragged_ref(q, kp, vp, rows, ln)
        assert not torch.isnan(ref["out"]).any()
        for chunk in RAGGED_CHUNKS:
            got = emulate_ragged(q, kp, vp, rows, ln, chunk)
            assert_within(got, ref["out"], ref["tol"], f"chunk {chunk}")
        muts = ["drop_last", "slot0"] + (["head_mod"] if G > 1 and Hk > 1
                                         else [])
        for mut in muts:
            got = emulate_ragged(q, kp, vp, rows, ln, 8, mut=mut)
            with pytest.raises(AssertionError):
                assert_within(got, ref["out"], ref["tol"], mut)
