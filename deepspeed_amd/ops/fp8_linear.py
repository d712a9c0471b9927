"""fp8 (OCP e4m3/e5m2) Linear through hipBLASLt tensorwise _scaled_mm.

Measured on MI355X (profiles/gemm_probe_fp8_vs_bf16.log): tensorwise fp8
_scaled_mm runs at ~2x the bf16 GEMM rate on the Llama-8B bench shapes
(2.4-3.3 PF vs 1.3-1.6 PF). Non-scaled fp8 MFMA is bf16-rate on CDNA4, so
hipBLASLt's scaled path is the only fp8 win; torch's MX-block (e8m0) path
measured SLOWER than bf16 — not used.

Recipe (transformer-engine-style, dynamic scaling):
  forward: x,w -> e4m3 with per-tensor amax scales; y = x8 @ w8^T (bf16 out)
  backward: dy -> e5m2; dx = dy8 @ w8 ; dw = dy8^T @ x8 (bf16 out)
Master weights stay bf16/fp32 in the optimizer — fp8 is a compute
format only. Reference role: deepspeed/ops/fp_quantizer fp8 gemm
(Triton there; hipBLASLt here), deepspeed/linear/quantization.py.
"""
import os

import torch

E4M3_MAX = 448.0
E5M2_MAX = 57344.0

_HAS_FP8 = hasattr(torch, "float8_e4m3fn")

# Weight contents change only at optimizer steps (ZeRO re-gathers fresh
# BUFFERS each micro-batch, but the bytes are identical within a step), so
# w8/sw/wT8 are cached per layer and invalidated by a global version the
# engine bumps after every optimizer step / checkpoint load. Measured: the
# uncached path LOST 6% end-to-end because re-quantizing W per call reads
# every weight again (profiles/tunableop_verdict.md round-2 bench).
_VERSION = [1]


def bump_fp8_version():
    _VERSION[0] += 1


def _fp8_ok(x, w):
    if not (_HAS_FP8 and x.is_cuda and x.dtype in (torch.bfloat16,
                                                   torch.float16)):
        return False
    m = x.numel() // x.shape[-1]
    k = x.shape[-1]
    n = w.shape[0]
    return m % 16 == 0 and k % 16 == 0 and n % 16 == 0


def _quant(t, dtype, fmax):
    """Per-tensor dynamic scale: t = t8 * scale (torch-op fallback).

    The arithmetic of the HIP kernels, in fp32 whatever t's dtype: the
    reciprocal of an fp16 scale overflows to inf for amax < fmax / 65504
    (every realistic dy), and one rounded to bf16 moves ~4 % of the codes,
    so the two arms of _quant_hip would disagree on the same tensor."""
    amax = torch.linalg.vector_norm(t.detach(), float("inf")).float()
    scale = (amax / fmax).clamp(min=1e-12)
    inv = 1.0 / scale
    t8 = (t.detach().float() * inv).clamp(-fmax, fmax).to(dtype)
    return t8, scale


def _quant_hip(t, e5m2, transpose):
    """Fused HIP path: amax (1 read) + cast[+transpose] (1 read, fp8
    writes) — replaces the 4-kernel torch sequence that measured ~24% of
    the fp8 step. Returns (t8, t8T-or-None, scale)."""
    from .loader import get_ext
    ext = get_ext(required=False)
    fmax = E5M2_MAX if e5m2 else E4M3_MAX
    dt = torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn
    if ext is None or not t.is_cuda or t.dtype != torch.bfloat16 \
            or t.numel() % 8 != 0 or t.data_ptr() % 16 != 0:
        t8, scale = _quant(t, dt, fmax)
        return t8, (_t8(t8) if transpose else None), scale
    amax = ext.fp8_amax(t)
    scale = (amax[0] / fmax).clamp(min=1e-12)
    if transpose:
        y, yt = ext.fp8_cast_transpose(t, scale, e5m2)
        return y.view(dt), yt.view(dt), scale
    return ext.fp8_cast(t, scale, e5m2).view(dt), None, scale


def _t8(t8):
    """fp8 transpose via int8 view (fp8 copy kernels exist, but the int8
    view is dependable across torch builds)."""
    return t8.view(torch.int8).t().contiguous().view(t8.dtype)


class _Fp8LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, w8, sw, wt8):
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        # x^T is produced here for free (wgrad needs it in backward)
        x8, xt8, sx = _quant_hip(x2, e5m2=False, transpose=True)
        y = torch._scaled_mm(x8, w8.t(), scale_a=sx, scale_b=sw,
                             out_dtype=x.dtype)
        if bias is not None:
            y = y + bias
        ctx.save_for_backward(xt8, sx, sw, wt8)
        ctx.has_bias = bias is not None
        ctx.in_dtype = x.dtype
        return y.reshape(*shp[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        xt8, sx, sw, wt8 = ctx.saved_tensors
        shp = dy.shape
        dy2 = dy.reshape(-1, shp[-1]).contiguous()
        dy8, dyt8, sdy = _quant_hip(dy2, e5m2=True, transpose=True)
        # dx[M,K] = dy[M,N] @ w[N,K]: b must be column-major => wT8.t()
        dx = torch._scaled_mm(dy8, wt8.t(), scale_a=sdy, scale_b=sw,
                              out_dtype=ctx.in_dtype)
        # dw[N,K] = dy^T[N,M] @ x[M,K]: a row-major dyT8; b col-major xT8.t()
        dw = torch._scaled_mm(dyt8, xt8.t(), scale_a=sdy, scale_b=sx,
                              out_dtype=ctx.in_dtype)
        db = dy2.sum(0) if ctx.has_bias else None
        return (dx.reshape(shp[:-1] + (wt8.shape[0],)), dw, db,
                None, None, None)


class Fp8Linear(torch.nn.Linear):
    """Drop-in nn.Linear computing fwd+bwd GEMMs in fp8 when eligible
    (CUDA, 16-divisible M/N/K); falls back to the bf16 path otherwise.
    `convert(module)` swaps every nn.Linear whose name matches `include`."""

    _w8 = None
    _sw = None
    _wt8 = None
    _wv = -1

    def forward(self, x):
        if _fp8_ok(x, self.weight) and not _disabled():
            if self._w8 is None or self._wv != _VERSION[0]:
                with torch.no_grad():  # cache is a constant; dw flows via
                    w8, wt8, sw = _quant_hip(  # the Function
                        self.weight.detach().contiguous(),
                        e5m2=False, transpose=True)
                    self._w8, self._sw, self._wt8 = w8, sw, wt8
                self._wv = _VERSION[0]
            return _Fp8LinearFn.apply(x, self.weight, self.bias,
                                      self._w8, self._sw, self._wt8)
        return super().forward(x)

    @classmethod
    def convert(cls, module, include=None):
        """Re-class matching nn.Linear instances in place (no copies)."""
        n_conv = 0
        for name, child in module.named_modules():
            if type(child) is torch.nn.Linear and \
                    (include is None or any(tag in name for tag in include)):
                child.__class__ = cls
                n_conv += 1
        return n_conv


def _disabled():
    return os.environ.get("DSAMD_FP8", "1") == "0"
