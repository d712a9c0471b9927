"""Autograd wrappers for the gfx950 kernel set.

GPU path: hand-written HIP kernels (required — no silent eager fallback).
CPU path (unit tests / no-GPU container): equivalent fp32 torch math.
"""
import torch

from .loader import get_ext


# --------------------------------------------------------------- RMSNorm
class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        # the kernels index rows as base + row*H: save the contiguous
        # tensors, so backward reads the same memory forward did
        x = x.contiguous()
        weight = weight.contiguous()
        if x.is_cuda and x.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            y, rstd = ext.rmsnorm_fwd(x, weight, eps)
        else:
            x32 = x.float()
            rstd = torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + eps)
            y = (x32 * rstd * weight.float()).to(x.dtype)
            rstd = rstd.reshape(-1)
        ctx.save_for_backward(x, weight, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        if x.is_cuda and x.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            dx, dw = ext.rmsnorm_bwd(dy.contiguous(), x, weight, rstd)
        else:
            H = x.shape[-1]
            x32 = x.float()
            dy32 = dy.float()
            rs = rstd.reshape(*x.shape[:-1], 1).float()
            w32 = weight.float()
            g = dy32 * w32
            dot = (g * x32).sum(-1, keepdim=True)
            dx = (rs * (g - x32 * dot * rs * rs / H)).to(x.dtype)
            dw = (dy32 * x32 * rs).reshape(-1, H).sum(0)
        return dx, dw.to(weight.dtype), None


def rms_norm(x, weight, eps=1e-5):
    return _RMSNormFn.apply(x, weight, eps)


# -------------------------------------------------------------- LayerNorm
class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x = x.contiguous()
        weight = weight.contiguous()
        if x.is_cuda and x.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            y, mean, rstd = ext.layernorm_fwd(x, weight,
                                              bias.contiguous()
                                              if bias is not None else None,
                                              eps)
        else:
            x32 = x.float()
            mean = x32.mean(-1, keepdim=True)
            var = x32.var(-1, unbiased=False, keepdim=True)
            rstd = torch.rsqrt(var + eps)
            xhat = (x32 - mean) * rstd
            y = (xhat * weight.float() +
                 (bias.float() if bias is not None else 0)).to(x.dtype)
            mean = mean.reshape(-1)
            rstd = rstd.reshape(-1)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        if x.is_cuda and x.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            dx, dw, db = ext.layernorm_bwd(dy.contiguous(), x, weight, mean,
                                           rstd)
        else:
            H = x.shape[-1]
            x32 = x.float()
            dy32 = dy.float()
            mu = mean.reshape(*x.shape[:-1], 1)
            rs = rstd.reshape(*x.shape[:-1], 1)
            xhat = (x32 - mu) * rs
            g = dy32 * weight.float()
            c1 = g.mean(-1, keepdim=True)
            c2 = (g * xhat).mean(-1, keepdim=True)
            dx = ((g - c1 - xhat * c2) * rs).to(x.dtype)
            dw = (dy32 * xhat).reshape(-1, H).sum(0)
            db = dy32.reshape(-1, H).sum(0)
        return (dx, dw.to(weight.dtype),
                db.to(weight.dtype) if ctx.has_bias else None, None)


def layer_norm(x, weight, bias=None, eps=1e-5):
    return _LayerNormFn.apply(x, weight, bias, eps)


# ------------------------------------------------------------------ RoPE
class _RoPEFn(torch.autograd.Function):
    """Rotates [B,S,H,D] with precomputed cos/sin [S, D/2] (rotate-half)."""

    @staticmethod
    def forward(ctx, t, cos, sin):
        # engine-wide .to(bf16) casts buffers; the table must stay fp32
        cos = cos.float()
        sin = sin.float()
        ctx.save_for_backward(cos, sin)
        if t.is_cuda and t.dtype == torch.bfloat16 and cos.dim() == 2:
            ext = get_ext(required=True)
            t = t.contiguous()
            out = torch.empty_like(t)
            ext.rope(out, t, cos, sin, 0, False)
        else:  # eager path also serves per-row positions (cos [B,S,half])
            out = _rope_torch(t, cos, sin, sign=1.0)
        return out

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        if dy.is_cuda and dy.dtype == torch.bfloat16 and cos.dim() == 2:
            ext = get_ext(required=True)
            dy = dy.contiguous()
            dx = torch.empty_like(dy)
            ext.rope(dx, dy, cos, sin, 0, True)
        else:
            dx = _rope_torch(dy, cos, sin, sign=-1.0)
        return dx, None, None


def _rope_torch(t, cos, sin, sign):
    B, S, H, D = t.shape
    half = D // 2
    t32 = t.float()
    x1 = t32[..., :half]
    x2 = t32[..., half:]
    if cos.dim() == 3:  # per-row positions: [B, S, half]
        c = cos.reshape(B, S, 1, half)
        s = sin.reshape(B, S, 1, half) * sign
    else:
        c = cos[:S].reshape(1, S, 1, half)
        s = sin[:S].reshape(1, S, 1, half) * sign
    o1 = x1 * c - x2 * s
    o2 = x2 * c + x1 * s
    return torch.cat([o1, o2], dim=-1).to(t.dtype)


def apply_rope(t, cos, sin):
    return _RoPEFn.apply(t, cos, sin)


def build_rope_cache(seq_len, head_dim, base=500000.0, device="cpu",
                     scaling=None):
    """Host-precomputed cos/sin table (guide Appendix B: no device trig)."""
    half = head_dim // 2
    inv_freq = 1.0 / (base ** (torch.arange(0, half, dtype=torch.float32,
                                            device=device) / half))
    pos = torch.arange(seq_len, dtype=torch.float32, device=device)
    freqs = torch.outer(pos, inv_freq)
    return freqs.cos().contiguous(), freqs.sin().contiguous()


# ---------------------------------------------------------------- SwiGLU
class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, u):
        g = g.contiguous()
        u = u.contiguous()
        ctx.save_for_backward(g, u)
        if g.is_cuda and g.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            return ext.swiglu_fwd(g, u)
        g32 = g.float()
        return (torch.nn.functional.silu(g32) * u.float()).to(g.dtype)

    @staticmethod
    def backward(ctx, dy):
        g, u = ctx.saved_tensors
        if g.is_cuda and g.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            dg, du = ext.swiglu_bwd(dy.contiguous(), g, u)
            return dg, du
        g32, u32, dy32 = g.float(), u.float(), dy.float()
        sig = torch.sigmoid(g32)
        silu = g32 * sig
        dg = (dy32 * u32 * (sig + silu * (1 - sig))).to(g.dtype)
        du = (dy32 * silu).to(u.dtype)
        return dg, du


def swiglu(g, u):
    return _SwiGLUFn.apply(g, u)


# ---------------------------------------------------------- CrossEntropy
class _FusedCrossEntropyFn(torch.autograd.Function):
    """Mean CE over non-ignored rows; logits [N, V] 16-bit, targets [N]."""

    @staticmethod
    def forward(ctx, logits, targets, ignore_index):
        logits = logits.contiguous()
        targets = targets.contiguous()
        if logits.is_cuda and logits.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            loss, lse = ext.cross_entropy_fwd(logits, targets, ignore_index)
        else:
            l32 = logits.float()
            lse = torch.logsumexp(l32, dim=-1)
            picked = l32.gather(
                1, targets.clamp(min=0).unsqueeze(1)).squeeze(1)
            loss = lse - picked
            loss = torch.where(targets == ignore_index,
                               torch.zeros_like(loss), loss)
        valid = (targets != ignore_index)
        n_valid = valid.sum().clamp(min=1)
        ctx.save_for_backward(logits, targets, lse, n_valid)
        ctx.ignore_index = ignore_index
        return loss.sum() / n_valid.to(loss.dtype)

    @staticmethod
    def backward(ctx, dloss):
        logits, targets, lse, n_valid = ctx.saved_tensors
        scale = (dloss.float() / n_valid.float())
        dloss_rows = scale.expand(logits.shape[0]).contiguous()
        if logits.is_cuda and logits.dtype == torch.bfloat16:
            ext = get_ext(required=True)
            dlogits = ext.cross_entropy_bwd(logits, targets, lse, dloss_rows,
                                            ctx.ignore_index)
        else:
            p = torch.softmax(logits.float(), dim=-1)
            onehot = torch.zeros_like(p)
            valid = targets != ctx.ignore_index
            idx = targets.clamp(min=0)
            onehot.scatter_(1, idx.unsqueeze(1), 1.0)
            g = (p - onehot) * dloss_rows.unsqueeze(1)
            g = torch.where(valid.unsqueeze(1), g, torch.zeros_like(g))
            dlogits = g.to(logits.dtype)
        return dlogits, None, None


def fused_cross_entropy(logits, targets, ignore_index=-100):
    """logits [..., V] (bf16 on GPU), targets [...] int64 -> scalar mean."""
    V = logits.shape[-1]
    return _FusedCrossEntropyFn.apply(logits.reshape(-1, V),
                                      targets.reshape(-1), ignore_index)


# ------------------------------------------------ ragged prefill attention
def _ragged_prefill_torch(q, kpool, vpool, batch):
    """Plain loop over the sequences: SDPA per sequence with an explicit
    causal-offset mask (token j of a sequence sees pool positions
    0..kv_len-q_len+j of its slot)."""
    T, Hq, D = q.shape
    G = Hq // kpool.shape[2]
    out = torch.empty_like(q)
    for slot, q_start, q_len, kv_len in batch.seqs:
        qs = q[q_start:q_start + q_len].transpose(0, 1)         # [Hq,q,D]
        ks = kpool[slot, :kv_len].transpose(0, 1)               # [Hk,kv,D]
        vs = vpool[slot, :kv_len].transpose(0, 1)
        if G > 1:
            ks = ks.repeat_interleave(G, dim=0)
            vs = vs.repeat_interleave(G, dim=0)
        pos = torch.arange(kv_len - q_len, kv_len, device=q.device)
        col = torch.arange(kv_len, device=q.device)
        mask = col.view(1, -1) <= pos.view(-1, 1)               # [q,kv]
        o = torch.nn.functional.scaled_dot_product_attention(
            qs.unsqueeze(0), ks.unsqueeze(0), vs.unsqueeze(0),
            attn_mask=mask)
        out[q_start:q_start + q_len] = o[0].transpose(0, 1)
    return out


def ragged_prefill_attention(q, kpool, vpool, batch):
    """Attention of one ragged serving step straight over the KV slot pool.

    q [T,Hq,D] packed tokens of all sequences in `batch` (a RaggedBatch),
    kpool/vpool [B,Smax,Hk,D] with this step's K/V rows already written.
    Returns [T,Hq,D]. bf16 on the GPU with D in {64,128} runs the
    `ragged_prefill` HIP kernel (no host sync); anything else the torch loop.
    """
    if q.is_cuda and q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128):
        ext = get_ext(required=True)
        return ext.ragged_prefill(q.contiguous(), kpool, vpool, batch.desc,
                                  batch.max_qlen, batch.max_kvlen)
    return _ragged_prefill_torch(q, kpool, vpool, batch)


# --------------------------------------------- ragged RoPE + KV append
def _ragged_rope_append_torch(q, k, v, cos, sin, tok_slot, tok_pos, kpool,
                              vpool, lens, put=None):
    """The pieces the unfused serving path uses: `_rope_torch` with the
    gathered table rows, then the pool and `lens` index_puts. Out-of-range
    tokens are dropped first (a host sync on a device, only when present)."""
    T = q.shape[0]
    B, Smax = kpool.shape[0], kpool.shape[1]
    limit = min(Smax, cos.shape[0])
    ok = ((tok_slot >= 0) & (tok_slot < B)
          & (tok_pos >= 0) & (tok_pos < limit))
    # a sequence is one contiguous q range with its own slot
    last = torch.ones(T, dtype=torch.bool, device=tok_slot.device)
    last[:-1] = tok_slot[1:] != tok_slot[:-1]
    q_rot = None
    if not bool(ok.all()):
        keep = ok.nonzero().squeeze(1)
        tok_slot, tok_pos, last = tok_slot[keep], tok_pos[keep], last[keep]
        q_rot = torch.zeros_like(q)
        q, k, v = q[keep], k[keep], v[keep]
    c = cos[tok_pos].float().unsqueeze(0)
    s = sin[tok_pos].float().unsqueeze(0)
    q_new = _rope_torch(q.unsqueeze(0), c, s, sign=1.0)[0]
    k_rot = _rope_torch(k.unsqueeze(0), c, s, sign=1.0)[0]
    if q_rot is None:
        q_rot = q_new
    else:
        q_rot[keep] = q_new
    if put is not None:          # fp8 pool: quantizing write
        put(tok_slot, tok_pos, k_rot, v)
    else:
        kpool[tok_slot, tok_pos] = k_rot
        vpool[tok_slot, tok_pos] = v
    if lens is not None:
        lens[tok_slot[last]] = tok_pos[last] + 1
    return q_rot


def ragged_rope_append(q, k, v, cos, sin, tok_slot, tok_pos, kpool, vpool,
                       lens=None):
    """RoPE of one ragged serving step fused with its KV-pool append.

    q [T,Hq,D], k/v [T,Hk,D] packed tokens; cos/sin [P,D/2] fp32 full tables;
    tok_slot/tok_pos [T] int64 (pool slot and position of each token);
    kpool/vpool [B,Smax,Hk,D]; lens [B] int64 or None. Returns q rotated at
    table row tok_pos[t] and writes kpool[tok_slot[t], tok_pos[t]] = rope(k[t])
    and vpool[...] = v[t]; with `lens`, the last token of each sequence sets
    lens[slot] = pos + 1. A token with slot outside [0,B) or pos outside
    [0, min(Smax,P)) is skipped (nothing written, q row zero).

    bf16 on the GPU runs the `ragged_rope_append` HIP kernel (one launch, no
    host sync); anything else the torch composition.
    """
    if q.is_cuda and q.dtype == torch.bfloat16:
        ext = get_ext(required=True)
        return ext.ragged_rope_append(q.contiguous(), k.contiguous(),
                                      v.contiguous(), cos, sin, tok_slot,
                                      tok_pos, kpool, vpool, lens)
    return _ragged_rope_append_torch(q, k, v, cos, sin, tok_slot, tok_pos,
                                     kpool, vpool, lens)


# ------------------------------------------------------ fp8 KV slot pool
KV_FP8_MAX = 448.0          # largest finite e4m3fn value
KV_FP8_HEAD_DIMS = (64, 128)


def kv_quantize(x):
    """One e4m3fn row per (..., D) row of `x`: returns (codes, scale) with
    codes [..., D] float8_e4m3fn and scale [...] fp32, the storage format of
    the fp8 KV slot pool:

        amax  = max |x[d]|                       (exact)
        scale = amax / 448 if amax > 0 else 1.0  (fp32, correctly rounded)
        inv   = 1.0 / scale                      (fp32, correctly rounded)
        code  = e4m3fn_rne(clamp(x[d] * inv, -448, 448))   (fp32 product)

    The clamp matters: x * inv can round just above 448 and torch's float8
    cast does not saturate. An all-zero row gives scale 1.0 and codes 0.

    Non-finite input (not produced by the serving path): an inf in the row
    makes scale = inf, so every element of the row reads back as NaN; a NaN
    element without an inf makes amax NaN, scale falls back to 1.0, that
    element gets the NaN code and the others are clamped to +-448.

    This composition is what the `ragged_rope_append_fp8` kernel computes bit
    for bit; it is the CPU fallback and the tests' reference.
    """
    xf = x.float()
    amax = xf.abs().amax(dim=-1)
    # The two divisions go through float64: torch's fp32 division on the GPU
    # is not correctly rounded (a scalar divisor becomes a multiply by its
    # reciprocal), while a float64 quotient of two fp32 values rounded once
    # more to fp32 IS the correctly rounded fp32 quotient (53 >= 2*24 + 2
    # bits), on every device.
    scale = torch.where(amax > 0, (amax.double() / KV_FP8_MAX).float(),
                        torch.ones_like(amax))
    inv = (1.0 / scale.double()).float()
    y = (xf * inv.unsqueeze(-1)).clamp(-KV_FP8_MAX, KV_FP8_MAX)
    return y.to(torch.float8_e4m3fn), scale


def kv_dequantize(codes, scale, dtype=torch.float32):
    """float(code) * scale, computed in fp32 (or in float64 when asked for,
    where the product is exact) and returned as `dtype`."""
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    return (codes.to(wide) * scale.to(wide).unsqueeze(-1)).to(dtype)


def _check_kv_fp8(kpool, vpool, k_scale, v_scale):
    if kpool.dtype != torch.float8_e4m3fn or \
            vpool.dtype != torch.float8_e4m3fn:
        raise ValueError("fp8 KV pool: kpool/vpool must be float8_e4m3fn")
    if kpool.shape[-1] not in KV_FP8_HEAD_DIMS:
        raise ValueError("fp8 KV pool: head_dim must be 64 or 128, got "
                         f"{kpool.shape[-1]}")
    if k_scale.shape != kpool.shape[:-1] or v_scale.shape != vpool.shape[:-1]:
        raise ValueError("fp8 KV pool: scales must be [B,Smax,Hk]")


def ragged_rope_append_fp8(q, k, v, cos, sin, tok_slot, tok_pos, kpool,
                           vpool, k_scale, v_scale, lens=None):
    """`ragged_rope_append` into the fp8 KV slot pool.

    Arguments and rules as `ragged_rope_append`, except kpool/vpool
    [B,Smax,Hk,D] float8_e4m3fn and k_scale/v_scale [B,Smax,Hk] fp32: the
    rotated K row (rounded to q's dtype, as the bf16 pool stores it) and the V
    row are written as `kv_quantize` codes plus scale. A skipped token writes
    neither codes nor scales nor lens. D must be 64 or 128. Non-finite rows:
    see `kv_quantize`.

    bf16 on the GPU runs the `ragged_rope_append_fp8` HIP kernel (one launch,
    no host sync); anything else the torch composition.
    """
    _check_kv_fp8(kpool, vpool, k_scale, v_scale)
    if q.is_cuda and q.dtype == torch.bfloat16:
        ext = get_ext(required=True)
        return ext.ragged_rope_append_fp8(
            q.contiguous(), k.contiguous(), v.contiguous(), cos, sin,
            tok_slot, tok_pos, kpool, vpool, k_scale, v_scale, lens)
    def put(slot, pos, k_rot, v_new):    # the in-range tokens only
        for pool, scales, x in ((kpool, k_scale, k_rot),
                                (vpool, v_scale, v_new)):
            codes, scale = kv_quantize(x)
            pool.view(torch.uint8)[slot, pos] = codes.view(torch.uint8)
            scales[slot, pos] = scale

    return _ragged_rope_append_torch(q, k, v, cos, sin, tok_slot, tok_pos,
                                     kpool, vpool, lens, put=put)


class _DecodeRows:
    """The decode rows as the sequence list `_ragged_prefill_torch` walks."""

    def __init__(self, rows, lens):
        self.seqs = [(int(s), i, 1, int(n)) for i, (s, n) in
                     enumerate(zip(rows.tolist(), lens.tolist())) if n > 0]


def ragged_decode_attention_fp8(q, kpool, vpool, k_scale, v_scale, rows,
                                lens, chunk=512):
    """Decode attention of q [n,1,Hq,D] (or [n,Hq,D]) over the first lens[i]
    positions of fp8 pool slot rows[i]; returns [n,1,Hq,D].

    bf16 on the GPU runs the `ragged_decode_fp8` HIP kernel; anything else
    dequantizes the pool and runs the torch loop of the prefill fallback."""
    _check_kv_fp8(kpool, vpool, k_scale, v_scale)
    if q.is_cuda and q.dtype == torch.bfloat16:
        ext = get_ext(required=True)
        return ext.ragged_decode_fp8(q.contiguous(), kpool, vpool, k_scale,
                                     v_scale, rows, lens, chunk)
    n, Hq, D = q.shape[0], q.shape[-2], q.shape[-1]
    out = _ragged_prefill_torch(q.reshape(n, Hq, D),
                                kv_dequantize(kpool, k_scale, q.dtype),
                                kv_dequantize(vpool, v_scale, q.dtype),
                                _DecodeRows(rows, lens))
    out[lens.to(out.device) == 0] = 0    # an empty row is defined as 0
    return out.view(n, 1, Hq, D)


def ragged_prefill_attention_fp8(q, kpool, vpool, k_scale, v_scale, batch):
    """`ragged_prefill_attention` over the fp8 KV slot pool (this step's rows
    already appended as codes plus scales). Returns [T,Hq,D].

    bf16 on the GPU runs the `ragged_prefill_fp8` HIP kernel; anything else
    dequantizes the pool and runs the torch loop."""
    _check_kv_fp8(kpool, vpool, k_scale, v_scale)
    if q.is_cuda and q.dtype == torch.bfloat16:
        ext = get_ext(required=True)
        return ext.ragged_prefill_fp8(q.contiguous(), kpool, vpool, k_scale,
                                      v_scale, batch.desc, batch.max_qlen,
                                      batch.max_kvlen)
    return _ragged_prefill_torch(q, kv_dequantize(kpool, k_scale, q.dtype),
                                 kv_dequantize(vpool, v_scale, q.dtype),
                                 batch)


def gds_handle(*a, **kw):
    """Parity stub for reference ops/aio GDS (GPUDirect Storage) builder.

    NVMe<->HBM direct DMA on ROCm ships as hipGDS/KFD DMA-BUF in ROCm
    enterprise stacks and is not present in this image; the in-tree
    O_DIRECT aio thread pool (ops/csrc/aio.cpp) covers the NVMe swap
    path through pinned host bounce buffers at NVMe line rate. Raises
    so GDS-dependent configs fail loudly.
    """
    raise RuntimeError(
        "GDS is unavailable on this ROCm stack; use aio_handle "
        "(O_DIRECT thread pool) — swap paths accept it interchangeably.")
