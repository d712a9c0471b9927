"""float64 references, derived bounds and shared cases for Fp8Linear.

The layer quantizes x and w to e4m3 and dy to e5m2 with one dynamic scale per
tensor and runs three library GEMMs on the CODES:

    Y  = deq(x8)  @ deq(w8)^T (+ bias)        deq(c) = c * scale
    dX = deq(dy8) @ deq(w8)
    dW = deq(dy8)^T @ deq(x8)
    db = dy.sum(0)                            (from the unquantized dy)

`ref_codes` is the quantizer (the arithmetic of the HIP kernels, proven equal
to them bit for bit by test_fp8_edges_gpu.py and
test_fp8_quant_kernels_match_torch): amax exact, scale = max(amax / fmax,
1e-12), inv = 1 / scale, codes = rne(clamp(t * inv, +-fmax)), all in fp32.
`linear_ref` evaluates the four lines above in float64 FROM THOSE CODES, so
quantization error is in the reference, not in the tolerance: what is left
between the layer and the reference is the GEMM's own arithmetic only.

Bound on a GEMM output element, ref = sa * sb * sum_k a_k b_k, n terms,
terms = sa * sb * sum_k |a_k b_k|  (never tuned, in the style of
edge_refs.py):

  * a product of two fp8 values has at most 4 + 4 significant bits: exact in
    fp32, so the only error of the dot product is its accumulation;
  * the products are NOT summed in fp32 one by one. Measured on the MI355X
    with fp32 output and unit scales (so neither the scale multiplies nor the
    output rounding take part): the residual reached 2^-14.4 * terms at
    n = 16 (18x the fp32 accumulate term below) and FELL with n (2^-17.0 at
    n = 256, 2^-19.1 at n = 4096), and it was the same with and without the
    scales, so the accumulation itself is what differs. A probe with one
    product of 2^16 and n - 1 equal small ones showed how, identically for
    K = 16 .. 1024 and both signs: exactly 7 of the small products, those
    sharing a group of 8 consecutive k with the large one, are cut toward
    zero to a multiple of 2^-13 of the large one (they vanish below it: 15
    products of 4 summed to 32, 15 of 28 to 8 * 28 + 7 * 24), while every
    other group of 8 reaches the accumulator intact down to 2^-23 of it.
    So each product is aligned to the largest product of its group of 8 and
    truncated at 2^-13 of it: 7 errors below 2^-13 * (group maximum) per
    group, in sum below 7 * 2^-13 * (sum of the group maxima)
    <= U_ALIGN * terms with U_ALIGN = 2^-10, whatever n is;
  * the group sums then enter an fp32 accumulator: n * u_acc * terms in any
    order. u_acc = U_ACC = 2^-23, not 2^-24: the probe shows that adder
    truncating (2^16 minus anything small gave the next fp32 below 2^16).
    Both terms rest on these measurements of the GEMM library and the matrix
    unit, not on a documented property;
  * EPI = 8 fixed fp32 roundings (units of 2^-24, on terms >= |ref|) cover
    the two scale multiplies, in either order and on either side of the sum;
  * ONE rounding to the output dtype: BF16_ULP * |ref| for bf16,
    2^-10 * |ref| + 2^-24 for fp16 (2^-10 bounds one fp16 ulp / |value|; the
    absolute term is the fp16 subnormal step, which dX reaches: dy ~ 1e-3
    times w ~ 1e-2);
  * with bias, Y is rounded once more after the add: one more output
    rounding, of |ref| including the bias (the first is of |ref - bias|; the
    bias itself is a value of the output dtype, hence exact);
  * db is torch's own column sum: M terms accumulated in fp32,
    M * 2^-24 * sum|dy|, then one output rounding.

Every bound is elementwise, so a cancelling element (|ref| << terms) is held
to its accumulate terms and a plain one mostly to its output rounding. The
alignment term is what the hardware can do at worst; on the cases below it
is about 20x the largest residual seen (2^-14.4 * terms).
"""
import functools

import torch

from edge_refs import EPI, U24, bf16_tol

E4M3_MAX = 448.0
E5M2_MAX = 57344.0
U_ACC = 2.0 ** -23        # per-term roundoff of the GEMM accumulator
U_ALIGN = 2.0 ** -10      # 7 addends per group of 8 cut at 2^-13 of its top
FP16_ULP = 2.0 ** -10     # upper bound on (1 fp16 ulp) / |value|
FP16_SUB = 2.0 ** -24     # fp16 subnormal step


def ref_codes(t, e5m2):
    """(codes, scale): the quantizer of the HIP kernels, fp32 arithmetic."""
    fmax = E5M2_MAX if e5m2 else E4M3_MAX
    dt = torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn
    t = t.detach()
    amax = t.abs().amax().float()
    scale = (amax / fmax).clamp(min=1e-12)
    inv = 1.0 / scale
    return (t.float() * inv).clamp(-fmax, fmax).to(dt), scale


def deq(codes, scale):
    return codes.float().double() * scale.double()


def _mm(a, b):
    """float64 a @ b and the sum of |terms| of every output element."""
    return a @ b, a.abs() @ b.abs()


def linear_ref(x, w, bias, dy):
    """float64 Y / dX / dW / db from the codes of x, w (e4m3) and dy (e5m2),
    with `<name>_terms` = sum|terms| per output element and the codes and
    scales themselves. x and dy may have leading dimensions; every result is
    2-d ([M, N], [M, K], [N, K]) or 1-d (db)."""
    x2 = x.detach().reshape(-1, x.shape[-1])
    dy2 = dy.detach().reshape(-1, dy.shape[-1])
    x8, sx = ref_codes(x2, False)
    w8, sw = ref_codes(w, False)
    dy8, sdy = ref_codes(dy2, True)
    xd, wd, dyd = deq(x8, sx), deq(w8, sw), deq(dy8, sdy)
    y0, y_terms = _mm(xd, wd.t())
    dx, dx_terms = _mm(dyd, wd)
    dw, dw_terms = _mm(dyd.t(), xd)
    r = dict(x8=x8, sx=sx, w8=w8, sw=sw, dy8=dy8, sdy=sdy,
             y0=y0, y=y0, y_terms=y_terms, dx=dx, dx_terms=dx_terms,
             dw=dw, dw_terms=dw_terms, M=x2.shape[0], K=x2.shape[1],
             N=w.shape[0])
    if bias is not None:
        r["y"] = y0 + bias.detach().double()
        r["db"] = dy2.double().sum(0)
        r["db_terms"] = dy2.double().abs().sum(0)
    return r


def out_tol(ref, dtype):
    """One rounding of |ref| to the output dtype."""
    if dtype == torch.bfloat16:
        return bf16_tol(ref)
    assert dtype == torch.float16, dtype
    return FP16_ULP * ref.abs() + FP16_SUB


def gemm_tol(ref, terms, n, dtype):
    return out_tol(ref, dtype) + (U_ALIGN + n * U_ACC + EPI * U24) * terms


def tolerances(r, dtype):
    """Bounds for every output of `linear_ref`'s result r (see the module
    docstring): y (with bias when r has one), dx, dw, db."""
    tol = dict(y=gemm_tol(r["y0"], r["y_terms"], r["K"], dtype),
               dx=gemm_tol(r["dx"], r["dx_terms"], r["N"], dtype),
               dw=gemm_tol(r["dw"], r["dw_terms"], r["M"], dtype))
    if "db" in r:
        tol["y"] = tol["y"] + out_tol(r["y"], dtype)
        tol["db"] = out_tol(r["db"], dtype) + r["M"] * U24 * r["db_terms"]
    return tol


# ------------------------------------------------------------------ cases
# (M, K, N): the smallest shape _fp8_ok admits; a second small one; one that
# crosses the 64-wide transpose tile in both directions with all three sizes
# distinct; a multi-tile one.
CASES = ((16, 16, 16), (16, 32, 48), (80, 144, 48), (128, 256, 64))
X_AMAX, W_AMAX, DY_AMAX = 40.0, 0.02, 1e-3


def make_tensor(g, rows, cols, amax, sign, dtype):
    """randn at amax / 4 kept inside 0.9 amax, a few exact zeros, and the
    amax itself as a +-sentinel on the last row and column: a quantizer that
    misses the last element gets the scale wrong."""
    t = (torch.randn(rows, cols, generator=g) * (amax / 4)) \
        .clamp(-0.9 * amax, 0.9 * amax)
    t[0, 0] = 0.0
    t[rows // 2, cols - 1] = 0.0
    t[rows - 1, 0] = 0.0
    t[rows - 1, cols - 1] = sign * amax
    return t.to(dtype)


@functools.lru_cache(maxsize=None)
def inputs(shape, dtype):
    """CPU inputs of one case, shared and never modified: x [M, K], w [N, K],
    bias [N], dy [M, N] with amax about 40 / 0.02 / 1e-3, so that any scale
    in the place of another is wrong by at least 1000x; `w_prev`, the weight
    one sign-SGD step of 2e-3 earlier (a stale cache), and `x_other`, another
    call's activation (a wrong saved tensor)."""
    M, K, N = shape
    g = torch.Generator().manual_seed(1000 * M + 10 * K + N)
    x = make_tensor(g, M, K, X_AMAX, 1.0, dtype)
    w = make_tensor(g, N, K, W_AMAX, -1.0, dtype)
    dy = make_tensor(g, M, N, DY_AMAX, -1.0, dtype)
    bias = (torch.randn(N, generator=g) * 0.25).to(dtype)
    step = 2e-3 * torch.sign(torch.randn(N, K, generator=g))
    w_prev = (w.float() + step).to(dtype)
    x_other = make_tensor(g, M, K, X_AMAX, -1.0, dtype)
    return dict(x=x, w=w, dy=dy, bias=bias, w_prev=w_prev, x_other=x_other)


@functools.lru_cache(maxsize=None)
def reference(shape, dtype, with_bias, device="cpu"):
    """linear_ref and its bounds for one case, computed once per device.
    A GPU test takes the reference from its own device: torch divides by a
    Python number as `amax * (1 / fmax)` there and as `amax / fmax` on the
    CPU, so the two scales can differ in the last bit (seen for e5m2), which
    is no property of the layer."""
    c = {k: v.to(device) for k, v in inputs(shape, dtype).items()}
    r = linear_ref(c["x"], c["w"], c["bias"] if with_bias else None, c["dy"])
    r = {k: v.cpu() if torch.is_tensor(v) else v for k, v in r.items()}
    return r, tolerances(r, dtype)
