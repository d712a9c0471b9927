"""float64 reference and derived bound for the weight gradient of a bf16
Linear, shared by test_linear_wgrad_gpu.py and test_linear_wgrad_cpu.py.

dw[N,K] = dy^T x: products of two bf16 values are exact in fp32, the sum
over the T rows is an fp32 sum in some order, and the result is rounded once
to bf16. So (tests/README.md, edge_refs.py) a dw element may differ from the
float64 reference by 1 bf16 ulp plus T * 2^-24 * sum|terms|."""
import torch

from edge_refs import U24, bf16_tol

# (T, K, N) of the issue: below, at and across the 64 x 64 transpose tile,
# K and N multiples of 8 (vector arms) with T odd (element-by-element arm)
CASES = [(16, 8, 8), (130, 72, 40), (257, 264, 136)]


def make_inputs(T, K, N, device, seed=0, lead=None):
    """x [T,K] (or lead + [K] when lead is given), w [N,K], dy like y."""
    g = torch.Generator().manual_seed(seed + T * 7 + K * 3 + N)
    shape = (T,) if lead is None else tuple(lead)
    x = torch.randn(*shape, K, generator=g).to(torch.bfloat16).to(device)
    w = (torch.randn(N, K, generator=g) * 0.5).to(torch.bfloat16).to(device)
    dy = (torch.randn(*shape, N, generator=g) * 2.0).to(torch.bfloat16) \
        .to(device)
    return x, w, dy


def dw_reference(x, dy):
    """(dw_ref, tol), float64, from the bf16 inputs themselves."""
    x64 = x.detach().double().reshape(-1, x.shape[-1]).cpu()
    dy64 = dy.detach().double().reshape(-1, dy.shape[-1]).cpu()
    ref = dy64.t() @ x64
    terms = dy64.abs().t() @ x64.abs()
    return ref, bf16_tol(ref, x64.shape[0] * U24 * terms)
