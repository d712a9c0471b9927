"""float64 references, tolerances and shared cases for the kernel edge tests.

Every bound below is derived from the number formats, never tuned:
  * a bf16 output is ONE RNE rounding of an fp32 result, so it may differ
    from the float64 reference by 1 bf16 ulp (2^-7 * |ref| bounds one ulp)
    plus whatever the fp32 evaluation itself is off by (`slack`);
  * an fp32 sum of n terms is off by at most n * 2^-24 * sum|terms|
    (any summation order); reductions add a fixed epilogue of EPI = 8
    roundings (divide, add eps, rsqrt / exp / log at <= 1 ulp = 2 units).
"""
import torch

U24 = 2.0 ** -24          # fp32 unit roundoff
BF16_ULP = 2.0 ** -7      # upper bound on (1 bf16 ulp) / |value|
EPI = 8                   # fixed fp32 roundings after a reduction
C_LOG = 4                 # native log: log2 at 1 ulp (2) times ln 2 (2)


def assert_within(got, ref, tol, what):
    """Elementwise |got - ref| <= tol over the whole tensor, no NaN."""
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.numel() == ref.numel(), \
        f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    tol = torch.as_tensor(tol, dtype=torch.float64).cpu() \
        .broadcast_to(ref.shape).reshape(-1)
    got, ref = got.reshape(-1), ref.reshape(-1)
    assert not torch.isnan(got).any(), f"{what}: NaN in output"
    err = (got - ref).abs()
    bad = err > tol
    if bad.any():
        i = int(torch.nonzero(bad)[0])
        t = tol[i]
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} off; first at {i}: "
            f"got {got[i].item()!r} ref {ref[i].item()!r} "
            f"err {err[i].item():.3e} tol {float(t):.3e}")


def bf16_tol(ref, slack=0.0):
    return BF16_ULP * ref.abs() + slack


# ------------------------------------------------------------ references
def rmsnorm_ref(x, w, dy, eps):
    """All float64. Returns dict of references and condition terms."""
    x, w, dy = x.double(), w.double(), dy.double()
    H = x.shape[-1]
    rstd = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    y = x * rstd * w
    g = dy * w
    dot = (g * x).sum(-1, keepdim=True)
    dot_abs = (g * x).abs().sum(-1, keepdim=True)
    dx = rstd * (g - x * dot * rstd * rstd / H)
    dx_terms = rstd * (g.abs() + x.abs() * dot_abs * rstd * rstd / H)
    dw = (dy * x * rstd).reshape(-1, H).sum(0)
    dw_abs = (dy * x * rstd).abs().reshape(-1, H).sum(0)
    return dict(rstd=rstd.reshape(-1), y=y, dx=dx, dx_terms=dx_terms, dw=dw,
                dw_abs=dw_abs)


def layernorm_ref(x, w, b, dy, eps):
    x, w, dy = x.double(), w.double(), dy.double()
    H = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    mean_abs = x.abs().mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)     # two-pass
    rstd = torch.rsqrt(var + eps)
    xhat = (x - mean) * rstd
    # |xhat| widened by what an fp32 mean can be off by (times rstd)
    xhat_w = xhat.abs() + mean_abs * rstd
    y = xhat * w + (b.double() if b is not None else 0.0)
    y_terms = xhat_w * w.abs() + (b.double().abs() if b is not None else 0.0)
    g = dy * w
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * xhat).mean(-1, keepdim=True)
    dx = (g - c1 - xhat * c2) * rstd
    dx_terms = (g.abs() + g.abs().mean(-1, keepdim=True) +
                xhat_w * (g.abs() * xhat_w).mean(-1, keepdim=True)) * rstd
    dw = (dy * xhat).reshape(-1, H).sum(0)
    dw_abs = (dy.abs() * xhat_w).reshape(-1, H).sum(0)
    db = dy.reshape(-1, H).sum(0)
    db_abs = dy.abs().reshape(-1, H).sum(0)
    return dict(mean=mean.reshape(-1), mean_abs=mean_abs.reshape(-1),
                rstd=rstd.reshape(-1), y=y, y_terms=y_terms, dx=dx,
                dx_terms=dx_terms, dw=dw, dw_abs=dw_abs, db=db,
                db_abs=db_abs)


def swiglu_ref(g, u, dy):
    g, u, dy = g.double(), u.double(), dy.double()
    sig = torch.sigmoid(g)
    silu = g * sig
    y = silu * u
    dg = dy * u * (sig + silu * (1 - sig))
    dg_terms = (dy * u).abs() * (sig.abs() + (silu * (1 - sig)).abs())
    du = dy * silu
    return dict(y=y, dg=dg, dg_terms=dg_terms, du=du)


def ce_ref(logits, targets, ignore_index=-100):
    """Per-row float64 lse / loss / softmax and the lse tolerance.

    lse = m + log(sum exp(x - m)): the sum has V positive terms (condition
    1), so its relative error is <= (V + EPI) * 2^-24, which is the ABSOLUTE
    error of the log. On top, in units of 2^-24:
      * exp(t) is evaluated as exp2(t * log2 e): rounding the argument costs
        2 * |t| relative per term, i.e. 2 * E_p[m - x] on the sum;
      * C_LOG = 4 on |lse - m|: native log is log2 (<= 1 ulp = 2 units)
        times ln 2 (constant and product rounding, 2 units);
      * 1 on |lse| for the final add. m is a bf16 value, hence exact.
    """
    x = logits.double()
    V = x.shape[-1]
    m = x.max(-1).values
    lse = torch.logsumexp(x, dim=-1)
    valid = targets != ignore_index
    picked = x.gather(1, targets.clamp(min=0).unsqueeze(1)).squeeze(1)
    loss = torch.where(valid, lse - picked, torch.zeros_like(lse))
    p = torch.softmax(x, dim=-1)
    finite = torch.isfinite(x)
    gap = torch.where(finite, m.unsqueeze(1) - x, torch.zeros_like(x))
    lse_tol = U24 * ((V + EPI) + 2.0 * (p * gap).sum(-1) +
                     C_LOG * (lse - m).abs() + lse.abs())
    loss_tol = lse_tol + U24 * (lse.abs() + picked.abs())
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, targets.clamp(min=0).unsqueeze(1), 1.0)
    return dict(lse=lse, loss=loss, lse_tol=lse_tol, loss_tol=loss_tol, p=p,
                onehot=onehot, valid=valid)


def ce_grad_ref(r, dloss_rows):
    """dlogits reference and fp32 slack: p inherits lse's absolute error as a
    relative one; p - onehot cancels, so 1e-6 * sum|terms| on top."""
    dl = dloss_rows.double().unsqueeze(1)
    g = dl * (r["p"] - r["onehot"])
    g = torch.where(r["valid"].unsqueeze(1), g, torch.zeros_like(g))
    slack = dl.abs() * (r["p"] * r["lse_tol"].unsqueeze(1) +
                        1e-6 * (r["p"] + r["onehot"]))
    return g, slack


# ------------------------------------------- strided wrapper-level cases
def strided_cases(device, dtype):
    """Non-contiguous inputs through the autograd wrappers, forward and
    backward, vs float64 on the same view. Each view's data pointer plus
    numel stays inside its storage. Returns a list of failures (strings)."""
    from deepspeed_amd.ops import functional as Fops
    torch.manual_seed(1234)
    rows, H, pad = 24, 64, 24
    fails = []

    def check(name, got, ref, tol):
        try:
            assert_within(got, ref, tol, name)
        except AssertionError as e:
            fails.append(str(e))

    def leaf(*shape, scale=1.0, shift=0.0):
        t = (torch.randn(*shape, device=device) * scale + shift).to(dtype)
        return t.requires_grad_(True)

    # a 16-bit result is one rounding of fp32 math; an fp32 result (CPU
    # fallback on fp32 inputs) is held to the fp32 slack alone
    ulp = BF16_ULP if dtype == torch.bfloat16 else 0.0

    def tol_of(ref, slack):
        return ulp * ref.abs() + slack

    # --- RMSNorm on the transpose of a [H, rows] tensor
    base = leaf(H, rows, scale=1.5)
    w = leaf(H, scale=0.7, shift=1.0)
    dy = (torch.randn(rows, H, device=device) * 2.0).to(dtype)
    x = base.t()
    assert not x.is_contiguous()
    y = Fops.rms_norm(x, w, 1e-5)
    y.backward(dy)
    r = rmsnorm_ref(x.detach(), w.detach(), dy, 1e-5)
    k = (H + EPI + 2) * U24
    check("rms_norm strided y", y, r["y"], tol_of(r["y"], k * r["y"].abs()))
    check("rms_norm strided dx", base.grad.t(), r["dx"],
          tol_of(r["dx"], 4 * (H + EPI) * U24 * r["dx_terms"]))
    check("rms_norm strided dw", w.grad, r["dw"],
          tol_of(r["dw"], (rows + H + 2 * EPI) * U24 * r["dw_abs"]))

    # --- LayerNorm: transposed x, every-other-element weight, offset +8
    base = leaf(H, rows, shift=8.0)
    wbuf = leaf(2 * H, scale=0.7, shift=1.0)
    b = leaf(H, scale=0.3)
    x, w = base.t(), wbuf[::2]
    assert not x.is_contiguous() and not w.is_contiguous()
    y = Fops.layer_norm(x, w, b, 1e-5)
    y.backward(dy)
    r = layernorm_ref(x.detach(), w.detach(), b.detach(), dy, 1e-5)
    check("layer_norm strided y", y, r["y"],
          tol_of(r["y"], (H + EPI + 3) * U24 * r["y_terms"]))
    check("layer_norm strided dx", base.grad.t(), r["dx"],
          tol_of(r["dx"], 4 * (H + EPI) * U24 * r["dx_terms"]))
    check("layer_norm strided dw", wbuf.grad[::2], r["dw"],
          tol_of(r["dw"], (rows + H + 2 * EPI) * U24 * r["dw_abs"]))
    check("layer_norm strided db", b.grad, r["db"],
          tol_of(r["db"], (rows + EPI) * U24 * r["db_abs"]))

    # --- SwiGLU: transposed g, u = padded[:, :H]
    gbase = leaf(H, rows, scale=2.0)
    ubuf = leaf(rows, H + pad, scale=0.5, shift=0.25)
    g, u = gbase.t(), ubuf[:, :H]
    assert not g.is_contiguous() and not u.is_contiguous()
    y = Fops.swiglu(g, u)
    y.backward(dy)
    r = swiglu_ref(g.detach(), u.detach(), dy)
    check("swiglu strided y", y, r["y"], tol_of(r["y"], 1e-6 * r["y"].abs()))
    check("swiglu strided dg", gbase.grad.t(), r["dg"],
          tol_of(r["dg"], 1e-6 * r["dg_terms"]))
    check("swiglu strided du", ubuf.grad[:, :H], r["du"],
          tol_of(r["du"], 1e-6 * r["du"].abs()))

    # --- cross-entropy on padded[:, :V] of a wider buffer
    N, V = 6, 1000
    lbuf = leaf(N, V + pad, scale=3.0)
    logits = lbuf[:, :V]
    assert not logits.is_contiguous()
    targets = torch.randint(0, V, (N,), device=device)
    targets[2] = -100
    loss = Fops.fused_cross_entropy(logits, targets)
    loss.backward()
    r = ce_ref(logits.detach(), targets)
    n_valid = int(r["valid"].sum())
    ref_loss = r["loss"].sum() / n_valid
    check("fused_cross_entropy strided loss", loss, ref_loss,
          r["loss_tol"].sum() / n_valid + (N + 1) * U24 * ref_loss.abs())
    dl = torch.full((N,), 1.0 / n_valid, device=device, dtype=torch.float64)
    gref, gslack = ce_grad_ref(r, dl)
    check("fused_cross_entropy strided dlogits", lbuf.grad[:, :V], gref,
          tol_of(gref, gslack))
    return fails
