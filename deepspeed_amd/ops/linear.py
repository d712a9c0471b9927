"""bf16 Linear whose weight-gradient GEMM gets its operands in a fast layout.

dW[N,K] = dY^T X reduces over the T tokens, and X[T,K], dY[T,N] are both
row-major, so neither operand is contiguous along the reduction; hipBLASLt
answers with a slower kernel class than the forward's. Writing dY^T and/or
X^T with the HIP transpose kernel (ops/csrc/transpose.hip, one read + one
write at HBM rate) and handing those to the GEMM is faster where the table
below says so (profiles/README.md, "Weight-gradient GEMMs in the fast
layout"; measured by tools/wgrad_probe.py).

Forward, dx and db are exactly what F.linear computes under autograd. The
transposed operands are temporaries of the backward; nothing extra is saved
from the forward.

Who takes this path: exact-type nn.Linear modules of a model handed to
deepspeed_amd.initialize (re-classed in place by WgradLinear.convert, after
the user's own conversions such as Fp8Linear.convert). Fp8Linear, the
compression layers, the tensor-parallel layers and MoE experts that own raw
weight tensors are other classes and keep their own GEMMs. Activation
checkpointing and Ulysses leave the Linear modules as they are, so those
take it too, at the shapes and token counts of the table below.
"""
import os

import torch
import torch.nn.functional as F

from .loader import get_ext

# Fewest tokens at which a transposed arrangement was measured to win: every
# figure in the table below is at T = 16384, the bench's 4 x 4096 tokens;
# below it nothing is measured, so nothing is rerouted.
MIN_TOKENS = 16384

# dW shape (N, K) -> (transpose dY, transpose X). tools/wgrad_probe.py on
# MI355X, T = 16384, ms per call: today's dy.t() @ x against the best of the
# three other arrangements, GEMM plus the transpose_bf16 calls it needs, and
# the round-to-round spread of today's figure (profiles/README.md has all
# four arrangements per shape):
#   q / o      4096 x  4096   0.445 -> 0.412  both      spread 0.021
#   gate / up 14336 x  4096   1.811 -> 1.726  X only    spread 0.032
#   down       4096 x 14336   1.845 -> 1.746  dY only   spread 0.024
#   lm_head  128256 x  4096  14.229 -> 12.553 X only    spread 0.077
#   k / v      1024 x  4096   0.157 -> 0.153: inside the spread of 0.018,
#                             so it keeps today's path, as does every shape
#                             that was not measured.
WGRAD_ARRANGEMENT = {
    (4096, 4096): (True, True),
    (14336, 4096): (False, True),
    (4096, 14336): (True, False),
    (128256, 4096): (False, True),
}


def _disabled():
    return os.environ.get("DSAMD_WGRAD_TN", "1") == "0"


def _eligible(x, w):
    return (x.is_cuda and x.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16 and w.requires_grad
            and torch.is_grad_enabled() and not _disabled()
            and x.numel() // max(x.shape[-1], 1) >= MIN_TOKENS
            and tuple(w.shape) in WGRAD_ARRANGEMENT
            and get_ext(required=False) is not None)


class _LinearWgradFn(torch.autograd.Function):
    """t_dy, t_x: which dW operand goes through transpose_bf16."""

    @staticmethod
    def forward(ctx, x, w, bias, t_dy, t_x):
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.t_dy, ctx.t_x = t_dy, t_x
        return F.linear(x, w, bias)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        ext = get_ext(required=True)
        dy2 = dy.reshape(-1, dy.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dy2.mm(w).reshape(x.shape)
        if ctx.needs_input_grad[1]:
            a = ext.transpose_bf16(dy2.contiguous()) if ctx.t_dy else dy2.t()
            b = ext.transpose_bf16(x2.contiguous()).t() if ctx.t_x else x2
            dw = a.mm(b)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy2.sum(0)
        return dx, dw, db, None, None


def linear(x, w, bias=None):
    """F.linear; on the eligible bf16 GPU case dW is computed from
    transposed operands."""
    if _eligible(x, w):
        return _LinearWgradFn.apply(x, w, bias,
                                    *WGRAD_ARRANGEMENT[tuple(w.shape)])
    return F.linear(x, w, bias)


class WgradLinear(torch.nn.Linear):
    """nn.Linear calling `linear` above; same parameters, same state_dict."""

    def forward(self, x):
        return linear(x, self.weight, self.bias)

    @classmethod
    def convert(cls, module):
        """Re-class every exact-type nn.Linear in place (no copies, hooks
        and parameter names stay). Returns how many were re-classed."""
        n = 0
        for child in module.modules():
            if type(child) is torch.nn.Linear:
                child.__class__ = cls
                n += 1
        return n
