"""References, derived bounds, inputs and a torch emulation shared by the fp8
KV slot-pool tests (conventions of edge_refs.py / attn_refs.py /
ragged_rope_append_refs.py: float64 references, nothing tuned).

Format (ops.functional.kv_quantize): a row x[0..D) is stored as e4m3fn codes
plus scale = amax / 448 (1.0 for an all-zero row); it reads back as
code * scale.

Append bound
------------
V, and K under an identity table (cos = 1, sin = 0: the rotation is exact
whatever the FMA contraction), must equal kv_quantize of the input row BIT FOR
BIT, codes and scale. For K under a random table let ref be the float64
rotation (rope_ref) and x the bf16 row the kernel quantizes:
  e_x = BF16_ULP * |ref| + slack                      (the existing rope bound)
so |x| <= x_hi = |ref| + e_x and |amax - amax_ref| <= e_amax = max_d e_x.
  scale: one correctly rounded division, so
      |scale - amax_ref / 448| <= e_amax / 448 + U24 * (amax_ref + e_amax) / 448
      =: scale_tol, and scale <= scale_hi = amax_ref / 448 + scale_tol;
      amax_ref == 0 means x == 0 exactly: scale must be 1.0 and the codes 0.
  code: y = fl(x * fl(1 / scale)) = (x / scale) * (1 + d), |d| <= 2 * U24 + U24^2
      (two roundings); e4m3fn RNE moves y by at most half a step, which is
      2^-4 * |y| for a normal result (3 mantissa bits) and 2^-10 in the
      subnormal range (|y| < 2^-6, where 2^-4 * |y| < 2^-10), i.e. by at most
      max(2^-4 * |y|, 2^-10); the clamp to +-448 only moves y towards x/scale.
  read back in float64, code * scale is exact, so
      |code * scale - x| <= max(2^-4 * x_hi, scale_hi * 2^-10) + 4 * U24 * x_hi
  (4 units: 2 for d, doubled once for d inside the half-step term), and
      |code * scale - ref| <= e_x + that.

Attention bound
---------------
The reference is the existing float64 ragged_ref / ragged_prefill_ref applied
to the DEQUANTIZED pool held in float64, where code * scale is exact, so no
quantization error enters. On top of their tolerance the fp8 kernels do
  * one more fp32 multiply on every score ((q . code) * k_scale): an absolute
    U24 * |s| <= U24 * s_abs on s, hence (relative, like eta = 2 * max ds)
    2 * U24 * max_j s_abs on every p;
  * `units` more fp32 roundings on the P @ V side, relative to P @ |V|:
      prefill: 1 (p * v_scale, before P is rounded to bf16),
      decode : 1 (p * v_scale) + 3 levels of merging the row groups of a wave
               (64 lanes / 8 lanes per D = 64 row = 8 groups), each two
               exps at 3 units and two multiply-adds at 1: 1 + 3 * 8 = 25.
  extra = (2 * max_j s_abs + units) * U24 * (P @ |V|).
"""
import math

import torch

from edge_refs import BF16_ULP, U24, assert_within
from ragged_rope_append_refs import check_call, pattern, rope_ref

FP8 = torch.float8_e4m3fn
HALF_STEP = 2.0 ** -4       # e4m3 RNE, normal range, relative
HALF_SUB = 2.0 ** -10       # e4m3 RNE, subnormal range, absolute (in codes)
NAN_CODE = 0x7F
UNITS_PREFILL = 1
UNITS_DECODE = 25


# ---------------------------------------------------------------- format
def quantize(x):
    from deepspeed_amd.ops.functional import kv_quantize
    return kv_quantize(x)


def dequant64(codes, scale):
    """code * scale in float64: exact."""
    return codes.cpu().double() * scale.cpu().double().unsqueeze(-1)


def quant_bound(ref, e_x):
    """ref [..., D] float64 row values, e_x how far the quantized row x may
    be from ref. Returns (tol on code*scale vs ref, scale_ref, scale_tol)."""
    ref = ref.double().abs()
    x_hi = ref + e_x
    amax = ref.amax(-1)
    e_amax = torch.as_tensor(e_x).broadcast_to(ref.shape).amax(-1)
    scale_ref = amax / 448.0
    scale_tol = e_amax / 448.0 + U24 * (amax + e_amax) / 448.0
    one = torch.ones_like(amax)
    scale_hi = torch.where(amax > 0, scale_ref + scale_tol, one)
    scale_ref = torch.where(amax > 0, scale_ref, one)
    scale_tol = torch.where(amax > 0, scale_tol, torch.zeros_like(amax))
    tol = e_x + torch.maximum(HALF_STEP * x_hi,
                              (scale_hi * HALF_SUB).unsqueeze(-1)) \
        + 4 * U24 * x_hi
    return tol, scale_ref, scale_tol


def code_bits(t):
    return t.cpu().view(torch.uint8)


def f32_bits(t):
    return t.cpu().view(torch.int32)


def pool_pattern(B, Smax, Hk, D, device, salt):
    """Non-constant fill of an fp8 pool: every byte value occurs, the NaN
    codes included, and the scales are a bf16-exact pattern."""
    n = B * Smax * Hk * D
    codes = ((torch.arange(n) * 7 + salt) % 256).to(torch.uint8) \
        .view(B, Smax, Hk, D).view(FP8).to(device)
    scale = pattern((B, Smax, Hk), torch.float32, device, salt=salt + 3)
    return codes, scale


def check_append_fp8(q_rot, q, k, v, cos, sin, tok_slot, tok_pos, pools,
                     pools0, lens, lens0, what, identity):
    """Everything one ragged_rope_append_fp8 call promises. pools = (kpool,
    vpool, k_scale, v_scale) after the call, pools0 copies from before.
    `identity`: cos = 1, sin = 0, so K must be bit-exact too."""
    kpool, vpool, ks, vs = pools
    kpool0, vpool0, ks0, vs0 = pools0
    B, Smax = kpool.shape[0], kpool.shape[1]
    P = cos.shape[0]
    slot, pos = tok_slot.cpu(), tok_pos.cpu()
    ok = (slot >= 0) & (slot < B) & (pos >= 0) & (pos < min(Smax, P))
    keep = ok.nonzero().squeeze(1)
    sl, ps = slot[keep], pos[keep]
    ulp = BF16_ULP if q.dtype == torch.bfloat16 else 0.0

    # q_rot and lens: the existing checks, on shadow pools that hold what a
    # correct bf16 append would have left
    kref, kslack = rope_ref(k.cpu()[keep], cos, sin, ps)
    shadow0 = pattern((B, Smax) + tuple(k.shape[1:]), q.dtype, "cpu", salt=9)
    kshadow, vshadow = shadow0.clone(), shadow0.clone()
    kshadow[sl, ps] = kref.to(q.dtype)
    vshadow[sl, ps] = v.cpu()[keep]
    check_call(q_rot, q, k, v, cos, sin, tok_slot, tok_pos, kshadow, vshadow,
               shadow0, shadow0, lens, lens0, what)

    # V (and K under an identity table): bit-exact kv_quantize
    exact = [("V", v, vpool, vs)] + ([("K", k, kpool, ks)] if identity
                                     else [])
    for name, x, pool, scale in exact:
        codes, sc = quantize(x.cpu()[keep])
        assert torch.equal(f32_bits(scale.cpu()[sl, ps]), f32_bits(sc)), \
            f"{what}: {name} scales differ from kv_quantize"
        assert torch.equal(code_bits(pool.cpu()[sl, ps]), code_bits(codes)), \
            f"{what}: {name} codes differ from kv_quantize"

    if not identity:
        e_x = ulp * kref.abs() + kslack
        tol, scale_ref, scale_tol = quant_bound(kref, e_x)
        got_scale = ks.cpu()[sl, ps]
        assert_within(got_scale, scale_ref, scale_tol, f"{what} k_scale")
        assert_within(dequant64(kpool.cpu()[sl, ps], got_scale), kref, tol,
                      f"{what} K rows")
        zero = kref.abs().amax(-1) == 0
        assert not code_bits(kpool.cpu()[sl, ps])[zero].bitwise_and(0x7F) \
            .any(), f"{what}: codes of an all-zero K row are not 0"

    named = torch.zeros(B, Smax, dtype=torch.bool)
    named[sl, ps] = True
    for name, got, before, bits in (("kpool", kpool, kpool0, code_bits),
                                    ("vpool", vpool, vpool0, code_bits),
                                    ("k_scale", ks, ks0, f32_bits),
                                    ("v_scale", vs, vs0, f32_bits)):
        assert torch.equal(bits(got)[~named], bits(before)[~named]), \
            f"{what}: {name} changed outside the rows the batch names"


# ------------------------------------------------------ attention inputs
def spread_quantize(kpool, vpool):
    """bf16 pools (NaN past each slot's fill, as make_ragged /
    make_ragged_prefill leave them) -> fp8 pools. Row magnitudes are spread
    over five binades, differently for K and V, with neighbouring positions
    and neighbouring heads always in different binades, so every scale
    differs per position and per head. Returns (clean, poisoned): in `clean`
    the rows past the fill are code 0 / scale 1, in `poisoned` NaN codes and
    NaN scales."""
    B, Smax, Hk, _ = kpool.shape
    pos = torch.arange(Smax).view(1, Smax, 1)
    hk = torch.arange(Hk).view(1, 1, Hk)
    ek = (3 * pos + 2 * hk) % 5 - 2
    ev = (2 * pos + hk + 1) % 5 - 2
    dev = kpool.device
    dead = kpool.isnan().any(-1)                             # [B,Smax,Hk]
    out = []
    for pool, e in ((kpool, ek), (vpool, ev)):
        x = pool.float() * torch.exp2(e.float()).unsqueeze(-1).to(dev)
        x = torch.where(dead.unsqueeze(-1), torch.zeros_like(x), x)
        codes, scale = quantize(x.to(pool.dtype))
        out.append((codes, scale))
    (kc, ks), (vc, vs) = out
    nan_code = torch.full_like(code_bits(kc), NAN_CODE).view(FP8).to(dev)
    d = dead.unsqueeze(-1)
    nan = torch.full_like(ks, float("nan"))
    clean = (kc, vc, ks, vs)
    poisoned = (torch.where(d, nan_code.view(torch.uint8),
                            kc.view(torch.uint8)).view(FP8),
                torch.where(d, nan_code.view(torch.uint8),
                            vc.view(torch.uint8)).view(FP8),
                torch.where(dead, nan, ks), torch.where(dead, nan, vs))
    return clean, poisoned


def decode_seqs(rows, lens):
    return [(int(s), i, 1, int(n)) for i, (s, n) in
            enumerate(zip(rows.tolist(), lens.tolist()))]


def fp8_extra_slack(q, k64, v64, seqs, units):
    """The `extra` term of the module docstring, [T,Hq,D] float64.
    q [T,Hq,D], k64/v64 the dequantized float64 pools."""
    T, Hq, D = q.shape
    G = Hq // k64.shape[2]
    scale = 1.0 / math.sqrt(D)
    hmap = torch.arange(Hq) // G
    q, k64, v64 = q.cpu(), k64.cpu(), v64.cpu()
    out = torch.zeros(T, Hq, D, dtype=torch.float64)
    for slot, q_start, q_len, kv_len in seqs:
        if kv_len == 0:
            continue
        qs = q[q_start:q_start + q_len].double().transpose(0, 1)
        kk = k64[slot, :kv_len][:, hmap].transpose(0, 1)
        vv = v64[slot, :kv_len][:, hmap].transpose(0, 1)
        p_ = torch.arange(kv_len - q_len, kv_len)
        adm = torch.arange(kv_len).view(1, -1) <= p_.view(-1, 1)
        s = qs @ kk.transpose(-1, -2) * scale
        s_abs = qs.abs() @ kk.abs().transpose(-1, -2) * scale
        s = torch.where(adm, s, torch.full_like(s, float("-inf")))
        t = torch.softmax(s, -1) @ vv.abs()
        smax = torch.where(adm, s_abs, torch.zeros_like(s_abs)) \
            .max(-1, keepdim=True).values
        out[q_start:q_start + q_len] = \
            ((2.0 * smax + units) * U24 * t).transpose(0, 1)
    return out


# ------------------------------------------------------------- emulation
MUTANTS = ("no_scale", "k_for_v", "prev_pos", "wrong_head", "v_in_sum")


def emulate_fp8(q, pools, seqs, round_p, mut=None):
    """What the fp8 kernels round, in plain fp32 torch: exact codes, fp32
    scores times k_scale, softmax with an UNSCALED row sum, p * v_scale
    (rounded to bf16 when `round_p`: the prefill MFMA), fp32 P @ codes, bf16
    output. `mut` names one deliberately broken edge."""
    kc, vc, ks, vs = (t.cpu() for t in pools)
    T, Hq, D = q.shape
    Hk = kc.shape[2]
    G = Hq // Hk
    hmap = torch.arange(Hq) // G
    smap = (hmap + 1) % Hk if mut == "wrong_head" else hmap
    scale = float(torch.tensor(1.0 / math.sqrt(D), dtype=torch.float32))
    out = torch.zeros(T, Hq, D)
    for slot, q_start, q_len, kv_len in seqs:
        if kv_len == 0:
            continue
        idx = torch.arange(kv_len)
        sidx = (idx - 1).clamp(min=0) if mut == "prev_pos" else idx
        qs = q.cpu()[q_start:q_start + q_len].float().transpose(0, 1)
        kk = kc[slot, :kv_len].float()[:, hmap].transpose(0, 1)
        vv = vc[slot, :kv_len].float()[:, hmap].transpose(0, 1)
        ksc = ks[slot, sidx][:, smap].t().unsqueeze(1)       # [Hq,1,kv]
        vsc = vs[slot, sidx][:, smap].t().unsqueeze(1)
        if mut == "no_scale":
            ksc, vsc = torch.ones_like(ksc), torch.ones_like(vsc)
        if mut == "k_for_v":
            vsc = ksc
        p_ = torch.arange(kv_len - q_len, kv_len)
        adm = idx.view(1, -1) <= p_.view(-1, 1)
        s = (qs @ kk.transpose(-1, -2)) * ksc * scale
        s = torch.where(adm, s, torch.full_like(s, float("-inf")))
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        pw = p * vsc
        l = (pw if mut == "v_in_sum" else p).sum(-1, keepdim=True)
        if round_p:
            pw = pw.to(torch.bfloat16).float()
        out[q_start:q_start + q_len] = ((pw @ vv) / l).transpose(0, 1)
    return out.to(torch.bfloat16)


def mutant_applies(mut, seqs, Hk):
    if mut == "prev_pos":
        return any(kv_len > 1 for _, _, _, kv_len in seqs)
    if mut == "wrong_head":
        return Hk > 1
    return True


# ------------------------------------------------------------ the cases
_CASES = {}


def decode_case(lens_name, G, D, Hk):
    """q [n,1,Hq,D] bf16, rows, lens, (clean, poisoned) pools, float64
    reference out and tol [n,1,Hq,D]; computed once and shared, callers must
    not modify them."""
    from attn_refs import (RAGGED_DUP, RAGGED_LENS_A, RAGGED_LENS_B,
                           make_ragged, ragged_ref)
    key = ("decode", lens_name, G, D, Hk)
    if key not in _CASES:
        lens = {"A": RAGGED_LENS_A, "B": RAGGED_LENS_B}[lens_name]
        q, kp, vp, rows, ln = make_ragged(lens, RAGGED_DUP, G, D, Hk, 14, 300)
        clean, poisoned = spread_quantize(kp, vp)
        k64 = dequant64(clean[0], clean[2])
        v64 = dequant64(clean[1], clean[3])
        ref = ragged_ref(q, k64, v64, rows, ln)
        seqs = decode_seqs(rows, ln)
        extra = fp8_extra_slack(q[:, 0], k64, v64, seqs, UNITS_DECODE)
        _CASES[key] = dict(q=q, rows=rows, lens=ln, clean=clean,
                           poisoned=poisoned, seqs=seqs, out=ref["out"],
                           tol=ref["tol"] + extra.unsqueeze(1))
    return _CASES[key]


def prefill_case(name, G, D, Hk):
    """q [T,Hq,D] bf16, seqs, (clean, poisoned) pools, float64 reference out
    and tol [T,Hq,D]; computed once and shared."""
    from ragged_prefill_refs import (BATCHES, make_ragged_prefill,
                                     ragged_prefill_ref)
    key = ("prefill", name, G, D, Hk)
    if key not in _CASES:
        q, kp, vp, seqs = make_ragged_prefill(BATCHES[name], G, D, Hk)
        clean, poisoned = spread_quantize(kp, vp)
        k64 = dequant64(clean[0], clean[2])
        v64 = dequant64(clean[1], clean[3])
        ref = ragged_prefill_ref(q, k64, v64, seqs)
        extra = fp8_extra_slack(q, k64, v64, seqs, UNITS_PREFILL)
        _CASES[key] = dict(q=q, seqs=seqs, clean=clean, poisoned=poisoned,
                           out=ref["out"], tol=ref["tol"] + extra)
    return _CASES[key]


# --------------------------------------------------------------- engine
def tiny_llama(device, dtype):
    """The tiny llama of test_serving.py with 4 q / 2 kv heads instead of
    8 / 4: head_dim 64, the smallest the fp8 pool takes."""
    import dataclasses

    from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
    cfg = dataclasses.replace(LLAMA_CONFIGS["llama-tiny"],
                              num_attention_heads=4, num_key_value_heads=2)
    assert cfg.head_dim == 64
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(device, dtype).eval()


def check_engine(device, dtype, fused_step):
    """5 requests over 3 slots with kv_dtype="fp8"; layer 0 against a bf16
    engine after the same first step. Returns the greedy-token agreement with
    the bf16-pool engine (reported by the caller, not asserted)."""
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine
    model = tiny_llama(device, dtype)
    cfg = model.cfg
    torch.manual_seed(1)
    prompts = [torch.randint(0, 2000, (n,)) for n in (21, 13, 5, 30, 9)]
    new, B = 6, 3

    def engine(kv_dtype):
        cb = ContinuousBatchingEngine(model, max_batch=B, prefill_chunk=8,
                                      prefill_budget=16,
                                      fused_step=fused_step,
                                      fused_kv_append=True,
                                      kv_dtype=kv_dtype)
        return cb, [cb.add_request(p, max_new_tokens=new) for p in prompts]

    cb, rids = engine("fp8")
    reqs = list(cb.pending)
    ref, ref_rids = engine(None)
    Smax, Hk, D = cb.max_seq, cfg.num_key_value_heads, cfg.head_dim
    for c in cb.caches:
        assert c.k.dtype == FP8 and c.v.dtype == FP8
        assert c.k_scale.dtype == torch.float32
        nbytes = sum(t.numel() * t.element_size()
                     for t in (c.k, c.v, c.k_scale, c.v_scale))
        assert nbytes == 2 * B * Smax * Hk * (D + 4)

    # first step: 16 tokens of the first prompt (longer than the budget), no
    # sampled token yet, so layer 0 saw identical inputs in both engines
    cb.step()
    ref.step()
    c0, r0 = cb.caches[0], ref.caches[0]
    slot = cb.prefilling[0].slot
    assert slot == ref.prefilling[0].slot
    assert int(c0.lens[slot]) == int(r0.lens[slot]) == 16
    codes, scale = quantize(r0.v[slot, :16].cpu())
    assert torch.equal(code_bits(c0.v[slot, :16]), code_bits(codes))
    assert torch.equal(f32_bits(c0.v_scale[slot, :16]), f32_bits(scale))
    x = r0.k[slot, :16].cpu().double()
    # both engines round the same rotation; allow one ulp of the pool dtype
    e_x = (BF16_ULP if dtype == torch.bfloat16 else 8 * U24) * x.abs()
    tol, scale_ref, scale_tol = quant_bound(x, e_x)
    assert_within(c0.k_scale[slot, :16], scale_ref, scale_tol,
                  "engine layer-0 k_scale")
    assert_within(dequant64(c0.k[slot, :16], c0.k_scale[slot, :16]), x, tol,
                  "engine layer-0 K")

    out, ref_out = cb.run(), ref.run()
    assert sorted(cb.free_slots) == list(range(B))
    assert not cb.running and not cb.pending and not cb.prefilling
    assert len(out) == len(prompts) > B                     # slots reused
    for rid, p in zip(rids, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
    # lens: a slot keeps the length of the last request it served (the last
    # sampled token is never appended)
    want = {}
    for r in reqs:                                          # in rid order
        want[r.slot] = len(r.prompt) + new - 1
    assert sorted(want) == list(range(B))
    for c in cb.caches:
        assert c.lens.tolist() == [want[s] for s in range(B)]
    agree = [float((out[a] == ref_out[b]).float().mean())
             for a, b in zip(rids, ref_rids)]
    return sum(agree) / len(agree)
