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
def _ragged_prefill_torch(q, kpool, vpool, batch, window=None):
    """Plain loop over the sequences: SDPA per sequence with an explicit
    causal-offset mask (token j of a sequence sees pool positions
    0..kv_len-q_len+j of its slot; under `window` only the last `window` of
    them, itself included)."""
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
        if window is not None:
            mask &= col.view(1, -1) > pos.view(-1, 1) - window
        o = torch.nn.functional.scaled_dot_product_attention(
            qs.unsqueeze(0), ks.unsqueeze(0), vs.unsqueeze(0),
            attn_mask=mask)
        out[q_start:q_start + q_len] = o[0].transpose(0, 1)
    return out


def ragged_prefill_attention(q, kpool, vpool, batch, window=None,
                             mfma=False):
    """Attention of one ragged serving step straight over the KV slot pool.

    q [T,Hq,D] packed tokens of all sequences in `batch` (a RaggedBatch),
    kpool/vpool [B,Smax,Hk,D] with this step's K/V rows already written.
    Returns [T,Hq,D]. Under `window` a token sees its last `window`
    positions, itself included.

    bf16 on the GPU with D in {64,128} (no host sync): `ragged_prefill` serves
    the shapes it was built for (no window, G in 1/2/4/8) unless `mfma` asks
    for the new kernel; `ragged_prefill_gqa` serves every other G <= 32 and
    every window. Anything else runs the torch loop."""
    if window is not None and window < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    G = q.shape[1] // kpool.shape[2]
    if q.is_cuda and q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128):
        ext = get_ext(required=True)
        if window is None and not mfma and G in (1, 2, 4, 8):
            return ext.ragged_prefill(q.contiguous(), kpool, vpool,
                                      batch.desc, batch.max_qlen,
                                      batch.max_kvlen)
        if G > 32:
            raise NotImplementedError(
                f"ragged prefill: GQA group {G} > 32 has no HIP kernel")
        return ext.ragged_prefill_gqa(q.contiguous(), kpool, vpool,
                                      batch.desc, batch.max_qlen,
                                      batch.max_kvlen, window or 0)
    return _ragged_prefill_torch(q, kpool, vpool, batch, window=window)


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


def ragged_decode_attention(q, kpool, vpool, rows, lens, window=None,
                            max_len=None, mfma=False):
    """Decode attention of q [n,1,Hq,D] (or [n,Hq,D]) over pool positions
    [lo_i, lens[i]) of slot rows[i], lo_i = max(0, lens[i] - window) under a
    window, else 0; returns [n,1,Hq,D]. An empty row is 0.

    bf16 on the GPU with D in {64,128}: `ragged_decode` serves the shapes it
    was built for (no window, G in 1/2/4/8) unless `mfma` asks for the new
    kernel; `ragged_decode_gqa` serves every other G <= 32 and every window.
    `max_len` (a host-side bound on lens) spares that kernel its one
    device-to-host read. Anything else runs the torch loop."""
    if window is not None and window < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    n, Hq, D = q.shape[0], q.shape[-2], q.shape[-1]
    G = Hq // kpool.shape[2]
    if q.is_cuda and q.dtype == torch.bfloat16 and D in (64, 128):
        ext = get_ext(required=True)
        if window is None and not mfma and G in (1, 2, 4, 8):
            return ext.ragged_decode(q.contiguous(), kpool, vpool, rows, lens)
        if G > 32:
            raise NotImplementedError(
                f"ragged decode: GQA group {G} > 32 has no HIP kernel")
        return ext.ragged_decode_gqa(q.contiguous(), kpool, vpool, rows, lens,
                                     window or 0, max_len or 0)
    out = _ragged_prefill_torch(q.reshape(n, Hq, D), kpool, vpool,
                                _DecodeRows(rows, lens), window=window)
    out[lens.to(out.device) == 0] = 0    # an empty row is defined as 0
    return out.view(n, 1, Hq, D)


def ragged_decode_attention_fp8(q, kpool, vpool, k_scale, v_scale, rows,
                                lens, chunk=512, window=None, max_len=None,
                                mfma=False):
    """Decode attention of q [n,1,Hq,D] (or [n,Hq,D]) over pool positions
    [lo_i, lens[i]) of fp8 pool slot rows[i], lo_i as in
    `ragged_decode_attention`; returns [n,1,Hq,D]. An empty row is 0.

    bf16 on the GPU: `ragged_decode_fp8` serves the shapes it was built for
    (no window, G in 1/2/4/8) unless `mfma` asks for the new kernel;
    `ragged_decode_gqa_fp8` serves every other G <= 32 and every window, and
    `max_len` (a host-side bound on lens) spares it its one device-to-host
    read. Anything else dequantizes the pool and runs the torch loop of the
    prefill fallback."""
    _check_kv_fp8(kpool, vpool, k_scale, v_scale)
    if window is not None and window < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    n, Hq, D = q.shape[0], q.shape[-2], q.shape[-1]
    if q.is_cuda and q.dtype == torch.bfloat16:
        ext = get_ext(required=True)
        G = Hq // kpool.shape[2]
        if window is None and not mfma and G in (1, 2, 4, 8):
            return ext.ragged_decode_fp8(q.contiguous(), kpool, vpool,
                                         k_scale, v_scale, rows, lens, chunk)
        if G > 32:
            raise NotImplementedError(
                f"ragged decode: GQA group {G} > 32 has no HIP kernel")
        return ext.ragged_decode_gqa_fp8(q.contiguous(), kpool, vpool,
                                         k_scale, v_scale, rows, lens,
                                         window or 0, max_len or 0)
    out = _ragged_prefill_torch(q.reshape(n, Hq, D),
                                kv_dequantize(kpool, k_scale, q.dtype),
                                kv_dequantize(vpool, v_scale, q.dtype),
                                _DecodeRows(rows, lens), window=window)
    out[lens.to(out.device) == 0] = 0    # an empty row is defined as 0
    return out.view(n, 1, Hq, D)


def ragged_prefill_attention_fp8(q, kpool, vpool, k_scale, v_scale, batch,
                                 window=None, mfma=False):
    """`ragged_prefill_attention` over the fp8 KV slot pool (this step's rows
    already appended as codes plus scales). Returns [T,Hq,D]. Under `window`
    a token sees its last `window` positions, itself included.

    bf16 on the GPU (no host sync): `ragged_prefill_fp8` serves the shapes it
    was built for (no window, G in 1/2/4/8) unless `mfma` asks for the new
    kernel; `ragged_prefill_gqa_fp8` serves every other G <= 32 and every
    window. Anything else dequantizes the pool and runs the torch loop."""
    _check_kv_fp8(kpool, vpool, k_scale, v_scale)
    if window is not None and window < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    if q.is_cuda and q.dtype == torch.bfloat16:
        ext = get_ext(required=True)
        G = q.shape[1] // kpool.shape[2]
        if window is None and not mfma and G in (1, 2, 4, 8):
            return ext.ragged_prefill_fp8(q.contiguous(), kpool, vpool,
                                          k_scale, v_scale, batch.desc,
                                          batch.max_qlen, batch.max_kvlen)
        if G > 32:
            raise NotImplementedError(
                f"ragged prefill: GQA group {G} > 32 has no HIP kernel")
        return ext.ragged_prefill_gqa_fp8(q.contiguous(), kpool, vpool,
                                          k_scale, v_scale, batch.desc,
                                          batch.max_qlen, batch.max_kvlen,
                                          window or 0)
    return _ragged_prefill_torch(q, kv_dequantize(kpool, k_scale, q.dtype),
                                 kv_dequantize(vpool, v_scale, q.dtype),
                                 batch, window=window)


# ------------------------------------------------------------ MoE routing
MOE_MAX_K = 8
MOE_MAX_EXPERTS = 256


def moe_gate_block_tokens(num_experts):
    """Tokens per workgroup of the HIP gate kernels (`block_tokens` in
    moe_routing.hip): the fp32 logits tile stays near 33 KB of LDS."""
    E = num_experts
    return 256 if E <= 32 else 128 if E <= 64 else 64 if E <= 128 else 32


def _moe_slot_token(idx, loc, keep, num_experts, capacity):
    """Inverse of the routing, without a host sync: slot e*C + c -> the flat
    choice index s*k + j that owns it, -1 for an empty slot."""
    n = num_experts * capacity
    pos = torch.where(keep, idx.long() * capacity + loc.long(), n).reshape(-1)
    st = torch.full((n + 1,), -1, dtype=torch.int32, device=idx.device)
    st.scatter_(0, pos, torch.arange(pos.numel(), dtype=torch.int32,
                                     device=idx.device))
    return st[:n]


def _moe_gate_topk_torch(logits, k, capacity, drop_tokens, ep_group):
    from ..moe.sharded_moe import gating_indices_at_capacity
    l_aux, idx, weights, loc, keep, capacity, mask = \
        gating_indices_at_capacity(logits, k, capacity, drop_tokens, ep_group)
    idx, loc = idx.to(torch.int32), loc.to(torch.int32)
    return (l_aux, idx, weights, loc, keep, mask.sum(dim=0).to(torch.int32),
            _moe_slot_token(idx, loc, keep, logits.shape[1], capacity))


def _moe_nodrop_capacity(counts, capacity, ep_group):
    """No-drop capacity: the longest queue, agreed on across the EP group so
    the all-to-all shapes match. The one host sync of the no-drop mode."""
    from .. import comm as dist
    capacity = max(capacity, int(counts.max().item()))
    if ep_group is not None and dist.get_world_size(ep_group) > 1:
        t = torch.tensor([capacity], device=counts.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=ep_group)
        capacity = int(t.item())
    return capacity


class _MoEGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, k, capacity, drop_tokens, ep_group):
        ext = get_ext(required=True)
        logits = logits.contiguous()
        idx, vals, rank, blocks, gsum = ext.moe_gate_rank(logits, k)
        # `blocks` turns from per-block counts into per-block offsets
        counts, l_aux = ext.moe_gate_scan(blocks, gsum, logits.shape[0], k)
        if not drop_tokens:
            capacity = _moe_nodrop_capacity(counts, capacity, ep_group)
        loc, keep, weights, slot_token = ext.moe_gate_finish(
            idx, vals, rank, blocks, counts, capacity, drop_tokens)
        ctx.save_for_backward(logits, idx, keep, counts)
        ctx.mark_non_differentiable(idx, loc, keep, counts, slot_token)
        return l_aux, idx, weights, loc, keep, counts, slot_token

    @staticmethod
    def backward(ctx, dl_aux, _idx, dweights, *_):
        logits, idx, keep, counts = ctx.saved_tensors
        ext = get_ext(required=True)
        if dl_aux is None:
            dl_aux = logits.new_zeros(())
        if dweights is None:
            dweights = logits.new_zeros(idx.shape)
        dlogits = ext.moe_gate_topk_bwd(
            logits, idx, keep, counts, dweights.float().contiguous(),
            dl_aux.float().contiguous())
        return dlogits, None, None, None, None


def moe_gate_topk(logits, k, capacity, drop_tokens=True, ep_group=None):
    """Index-form top-k gate of fp32 logits [S, E] at capacity C.

    Returns (l_aux, idx, weights, loc, keep, counts, slot_token):
      idx [S,k] int32      the k experts of largest softmax gate; among equal
                           gates the LOWER expert index wins on the HIP path
                           (torch.topk, the fallback, promises no order);
      loc [S,k] int32      tokens t < s that chose the same expert;
      keep [S,k] bool      loc < C when dropping, all true otherwise;
      weights [S,k] fp32   gates[idx] * keep / max(sum of kept, 1e-9);
      counts [E] int32     tokens that chose each expert, before dropping;
      l_aux                E*E/k * sum_e mean_s(gates) * mean_s(mask);
      slot_token [E*C] int32   the choice s*k + j that owns slot e*C + loc,
                           -1 for an empty slot.
    With `drop_tokens=False` C grows to the longest queue (one host sync, and
    a MAX all-reduce over `ep_group`); read it back as len(slot_token) // E.
    Differentiable in `weights` and `l_aux`, the mask held constant.

    fp32 on the GPU with 1 <= k <= 8 and k <= E <= 256 runs the HIP gate
    (three launches, backward one); anything else
    `moe.sharded_moe.gating_indices_at_capacity`, the definition both share.
    S = 0 gives empty outputs and l_aux = 0.
    """
    S, E = logits.shape
    hip = (logits.is_cuda and logits.dtype == torch.float32 and S > 0
           and 1 <= k <= MOE_MAX_K and k <= E <= MOE_MAX_EXPERTS
           and capacity >= 1 and S * MOE_MAX_K < 2 ** 31)
    if not hip:
        out = _moe_gate_topk_torch(logits, k, capacity, drop_tokens, ep_group)
        if S == 0:      # a mean over no tokens is NaN
            out = (logits.sum() * 0.0,) + out[1:]
        return out
    return _MoEGateFn.apply(logits, k, capacity, drop_tokens, ep_group)


def _moe_rows_ok(*tensors):
    """The row kernels' contract: bf16 / fp32 on the GPU, contiguous 2-d,
    16-byte aligned, rows a whole number of 16-byte vectors."""
    first = tensors[0]
    return all(
        t.is_cuda and t.dtype == first.dtype
        and t.dtype in (torch.bfloat16, torch.float32) and t.dim() == 2
        and t.is_contiguous() and t.shape[1] > 0
        and (t.shape[1] * t.element_size()) % 16 == 0
        and t.data_ptr() % 16 == 0 for t in tensors)


def _moe_grad_rows(g):
    g = g.contiguous()
    return g if g.data_ptr() % 16 == 0 else g.clone()


def _moe_routing_i32(idx, loc, keep):
    return (idx.to(torch.int32).contiguous(), loc.to(torch.int32).contiguous(),
            keep.contiguous())


class _MoEDispatchFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, loc, keep, slot_token, capacity, out):
        ext = get_ext(required=True)
        if out is None:
            out = x.new_empty(slot_token.numel(), x.shape[1])
        else:
            ctx.mark_dirty(out)
        ext.moe_scatter_rows(out.view(-1, x.shape[1]), x, slot_token, None,
                             idx.shape[1])
        ctx.save_for_backward(idx, loc, keep)
        ctx.capacity = capacity
        return out

    @staticmethod
    def backward(ctx, g):
        idx, loc, keep = ctx.saved_tensors
        ext = get_ext(required=True)
        g = _moe_grad_rows(g.reshape(-1, g.shape[-1]))
        dx = g.new_empty(idx.shape[0], g.shape[1])
        ext.moe_gather_rows(dx, g, idx, loc, keep, None, ctx.capacity)
        return dx, None, None, None, None, None, None


def _moe_dispatch_torch(x, idx, loc, keep, num_experts, capacity):
    S, k = idx.shape
    n = num_experts * capacity
    pos = torch.where(keep, idx.long() * capacity + loc.long(), n).reshape(-1)
    tok = torch.arange(S, device=x.device).repeat_interleave(k)
    # dropped choices land on row n, which is cut off
    return x.new_zeros(n + 1, x.shape[1]).index_copy(
        0, pos, x.index_select(0, tok))[:n]


def moe_dispatch(x, idx, loc, keep, slot_token, num_experts, capacity,
                 out=None):
    """Rows of x [S, M] to their expert slots: returns [E, C, M] with
    out[e, c] = x[s] for the kept choice (s, j) at idx = e, loc = c, and 0 in
    every empty slot. `out` ([E, C, M] or [E*C, M]) supplies the storage;
    every row of it is written.

    bf16 / fp32 on the GPU, contiguous 16-byte-aligned rows that are a
    multiple of 16 bytes wide: the `moe_scatter_rows` HIP kernel, one launch,
    a bit-exact copy; backward is `moe_gather_rows`. Anything else runs torch
    index ops (no host sync either).
    """
    M = x.shape[1]
    n = num_experts * capacity
    out2 = out.view(n, M) if out is not None else None
    rows = (x,) if out2 is None else (x, out2)
    if _moe_rows_ok(*rows) and idx.shape[1] <= MOE_MAX_K and n > 0:
        idx, loc, keep = _moe_routing_i32(idx, loc, keep)
        # `out` itself, not a view of it: autograd tracks the written tensor
        res = _MoEDispatchFn.apply(x, idx, loc, keep, slot_token.contiguous(),
                                   capacity, out)
    else:
        res = _moe_dispatch_torch(x, idx, loc, keep, num_experts, capacity)
        if out2 is not None:
            res = out2.copy_(res)
    return res.view(num_experts, capacity, M)


class _MoECombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, expert_out, idx, loc, keep, weights, slot_token,
                capacity, out):
        ext = get_ext(required=True)
        if out is None:
            out = expert_out.new_empty(idx.shape[0], expert_out.shape[1])
        else:
            ctx.mark_dirty(out)
        ext.moe_gather_rows(out, expert_out, idx, loc, keep, weights,
                            capacity)
        ctx.save_for_backward(expert_out, idx, loc, keep, weights, slot_token)
        ctx.capacity = capacity
        return out

    @staticmethod
    def backward(ctx, g):
        expert_out, idx, loc, keep, weights, slot_token = ctx.saved_tensors
        ext = get_ext(required=True)
        g = _moe_grad_rows(g)
        d_expert = dw = None
        if ctx.needs_input_grad[0]:
            d_expert = torch.empty_like(expert_out)
            ext.moe_scatter_rows(d_expert, g, slot_token, weights,
                                 idx.shape[1])
        if ctx.needs_input_grad[4]:
            dw = ext.moe_gather_dot(g, expert_out, idx, loc, keep,
                                    ctx.capacity)
        return d_expert, None, None, None, dw, None, None, None


def _moe_combine_torch(expert_flat, idx, loc, keep, weights, capacity):
    S, k = idx.shape
    safe_pos = (idx.long() * capacity + loc.long()).reshape(-1) \
        .clamp_(max=expert_flat.shape[0] - 1)
    gathered = expert_flat.index_select(0, safe_pos) \
        .reshape(S, k, expert_flat.shape[1])
    wk = (weights * keep).to(gathered.dtype).unsqueeze(-1)
    return (wk * gathered).sum(dim=1)


def moe_combine(expert_out, idx, loc, keep, weights, out=None,
                slot_token=None):
    """Gate-weighted sum of each token's kept expert rows: expert_out
    [E, C, M] -> [S, M], out[s] = sum_j weights[s, j] * expert_out[idx, loc]
    over the kept choices. `out` [S, M] supplies the storage. `slot_token`
    (from `moe_gate_topk`) spares backward rebuilding it.

    Same requirements as `moe_dispatch`: the `moe_gather_rows` HIP kernel
    (fp32 weights and accumulation, one rounding), backward
    `moe_scatter_rows` scaled by the weights plus `moe_gather_dot` for the
    weights' gradient. Anything else runs torch index ops, with the weights
    rounded to the activation dtype first.
    """
    E, C, M = expert_out.shape
    flat = expert_out.reshape(E * C, M)
    rows = (flat,) if out is None else (flat, out)
    if _moe_rows_ok(*rows) and idx.shape[1] <= MOE_MAX_K and idx.shape[0] > 0:
        idx, loc, keep = _moe_routing_i32(idx, loc, keep)
        if slot_token is None:
            slot_token = _moe_slot_token(idx, loc, keep, E, C)
        return _MoECombineFn.apply(flat, idx, loc, keep,
                                   weights.float().contiguous(),
                                   slot_token.contiguous(), C, out)
    res = _moe_combine_torch(flat, idx, loc, keep, weights, C)
    return res if out is None else out.copy_(res)


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
