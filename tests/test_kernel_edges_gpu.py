"""HIP kernels at tail, strided, masked and misaligned edges (needs MI355X).

References are plain torch in float64 on the same bf16-rounded / fp32
inputs; every comparison is elementwise over the whole tensor. Tolerances
and their derivations live in edge_refs.py. Tail / last elements carry
sentinels (a dominant value) so that one dropped element cannot hide.
"""
import itertools
import math

import pytest
import torch

from edge_refs import (EPI, U24, assert_within, bf16_tol, ce_grad_ref, ce_ref,
                       layernorm_ref, rmsnorm_ref, strided_cases, swiglu_ref)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
SIZES = [1, 7, 8, 9, 2055, 256 * 8 * 3 + 5]
SENT = 1000.0


def _ext():
    return get_ext(required=True)


def _flat(n, off, dtype, scale=1.0, shift=0.0, vec=8):
    """Contiguous [n] tensor whose base is 16-byte aligned (off=0) or one
    element past it (off=1): buf[off:off+n] of a larger buffer. The first
    element of the scalar tail and the last element are returned too."""
    buf = (torch.randn(n + 8, device=DEV) * scale + shift).to(dtype)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + n]
    assert t.is_contiguous() and t.numel() == n
    return t, sorted({(n // vec) * vec if n % vec else n - 1, n - 1})


# ------------------------------------------------------------ elementwise
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_swiglu_tail_and_offset(n, off):
    torch.manual_seed(n + off)
    g, sent = _flat(n, off, BF, scale=2.0)
    u, _ = _flat(n, off, BF, scale=0.5, shift=0.25)
    dy, _ = _flat(n, off, BF, scale=3.0)
    for i in sent:           # silu(8) * 100 ~ 800: unmistakable
        g[i], u[i], dy[i] = 8.0, 100.0, 50.0
    r = swiglu_ref(g, u, dy)
    y = _ext().swiglu_fwd(g, u)
    dg, du = _ext().swiglu_bwd(dy, g, u)
    assert_within(y, r["y"], bf16_tol(r["y"], 1e-6 * r["y"].abs()), "y")
    assert_within(dg, r["dg"], bf16_tol(r["dg"], 1e-6 * r["dg_terms"]), "dg")
    assert_within(du, r["du"], bf16_tol(r["du"], 1e-6 * r["du"].abs()), "du")


@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_accum_bf16_to_f32_exact(n, off, scale):
    """scale is a power of two, so src*scale is exact and dst + it is ONE
    fp32 rounding whether or not the kernel fuses the multiply-add."""
    torch.manual_seed(n + off)
    dst, sent = _flat(n, off, torch.float32, scale=3.0, shift=1.0, vec=4)
    src, _ = _flat(n, off, BF, scale=0.7, vec=4)
    for i in sent:
        src[i] = SENT
    ref = dst + src.float() * scale
    _ext().accum_bf16_to_f32(dst, src, scale)
    assert torch.equal(dst, ref), (dst - ref).abs().max().item()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("with_other", [False, True])
@pytest.mark.parametrize("lead", [(2, 5), (1, 1)])
@pytest.mark.parametrize("C", [3, 8, 320])
def test_spatial_bias_add(C, lead, with_other, off):
    """off=1: `a` (and `other`) start one element past a 16-byte boundary,
    as a view into a flat buffer does -> the kernel's scalar arm."""
    torch.manual_seed(C)
    n = lead[0] * lead[1] * C
    a = _flat(n, off, BF, scale=2.0)[0].view(*lead, C)
    bias = (torch.randn(C, device=DEV) * 0.5 + 0.25).to(BF)
    other = _flat(n, off, BF, scale=4.0)[0].view(*lead, C) \
        if with_other else None
    a.view(-1)[-1] = SENT
    a.view(-1)[(a.numel() // 8) * 8 - (0 if a.numel() % 8 else 1)] = -SENT
    ref = a.double() + bias.double()
    terms = a.double().abs() + bias.double().abs()
    if with_other:
        ref = ref + other.double()
        terms = terms + other.double().abs()
    y = _ext().spatial_bias_add(a, bias, other)
    assert y.shape == a.shape
    assert_within(y, ref, bf16_tol(ref, 1e-6 * terms), "y")


def test_spatial_bias_add_contract():
    a = torch.randn(2, 5, 8, device=DEV).to(BF)
    bias = torch.randn(8, device=DEV)
    with pytest.raises(RuntimeError):
        _ext().spatial_bias_add(a, bias, None)          # fp32 bias
    with pytest.raises(RuntimeError):
        _ext().spatial_bias_add(a, bias.to(BF), a.float())  # fp32 other
    with pytest.raises(RuntimeError):
        _ext().spatial_bias_add(a, bias.to(BF),
                                a.transpose(0, 1))      # strided other


def _rope_ref(t, cos, sin, pos0, sign):
    B, S, H, D = t.shape
    half = D // 2
    t = t.double()
    a, b = t[..., :half], t[..., half:]
    c = cos[pos0:pos0 + S].double().reshape(1, S, 1, half)
    s = sin[pos0:pos0 + S].double().reshape(1, S, 1, half) * sign
    ref = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    terms = torch.cat([(a * c).abs() + (b * s).abs(),
                       (b * c).abs() + (a * s).abs()], dim=-1)
    return ref, terms


ROPE_SHAPES = [(2, 5, 3, D) for D in (128, 64, 16, 24, 6)] + \
    [(1, 257, 1, 16), (1, 257, 1, 6)]


@pytest.mark.parametrize("pos0", [0, 3])
@pytest.mark.parametrize("shape", ROPE_SHAPES)
def test_rope_shapes_and_pos0(shape, pos0):
    from deepspeed_amd.ops.functional import build_rope_cache
    B, S, H, D = shape
    torch.manual_seed(D + S)
    cos, sin = build_rope_cache(S + 5, D, base=10000.0, device=DEV)
    t = (torch.randn(*shape, device=DEV) * 2.0).to(BF)
    t.view(-1)[-1] = SENT
    t.view(-1)[D // 2 - 1] = -SENT
    for backward in (False, True):
        ref, terms = _rope_ref(t, cos, sin, pos0, -1.0 if backward else 1.0)
        out = torch.empty_like(t)
        _ext().rope(out, t, cos, sin, pos0, backward)
        assert_within(out, ref, bf16_tol(ref, 1e-6 * terms),
                      f"rope backward={backward}")
        inp = t.clone()
        _ext().rope_inplace(inp, cos, sin, pos0, backward)
        assert torch.equal(inp, out), "rope_inplace != out-of-place"


def test_rope_contract():
    from deepspeed_amd.ops.functional import build_rope_cache
    B, S, H, D = 2, 5, 3, 16
    cos, sin = build_rope_cache(S + 2, D, device=DEV)
    t = torch.randn(B, S, H, D, device=DEV).to(BF)
    out = torch.empty_like(t)
    _ext().rope(out, t, cos, sin, 2, False)            # exactly fits
    for bad_pos0 in (3, -1):
        with pytest.raises(RuntimeError):
            _ext().rope(out, t, cos, sin, bad_pos0, False)
    with pytest.raises(RuntimeError):
        _ext().rope(out.float(), t, cos, sin, 0, False)
    with pytest.raises(RuntimeError):
        _ext().rope(out, t.transpose(1, 2), cos, sin, 0, False)


# --------------------------------------------------------- row reductions
NORM_SHAPES = [(3, H) for H in (1, 7, 8, 250, 1000, 1001, 2056)] + \
    [(513, 64), (4097, 64)]     # dgamma arms: gy = 1 / 16 / 64


def _norm_inputs(rows, H, shift):
    torch.manual_seed(rows * 10000 + H)
    x = (torch.randn(rows, H, device=DEV) * 1.5 + shift).to(BF)
    w = (torch.randn(H, device=DEV) * 0.7 + 1.0).to(BF)
    b = (torch.randn(H, device=DEV) * 0.3).to(BF)
    dy = (torch.randn(rows, H, device=DEV) * 2.0).to(BF)
    # sentinels only in the last row (they swamp that row's statistics)
    x[-1, H - 1] = SENT
    x[-1, (H // 8) * 8 if H % 8 else H - 1] = SENT
    dy[-1, H - 1] = 64.0
    return x, w, b, dy


@pytest.mark.parametrize("rows,H", NORM_SHAPES)
def test_rmsnorm_rows(rows, H):
    x, w, _, dy = _norm_inputs(rows, H, 0.0)
    r = rmsnorm_ref(x, w, dy, 1e-5)
    y, rstd = _ext().rmsnorm_fwd(x, w, 1e-5)
    # rstd: positive-term sum (condition 1): relative (H + EPI) * 2^-24
    assert_within(rstd, r["rstd"], (H + EPI) * U24 * r["rstd"], "rstd")
    assert_within(y, r["y"], bf16_tol(r["y"], (H + EPI + 2) * U24 *
                                      r["y"].abs()), "y")
    dx, dw = _ext().rmsnorm_bwd(dy, x, w, rstd)
    # rstd enters cubed and the row dot once: 4 * (H + EPI) roundings
    assert_within(dx, r["dx"], bf16_tol(r["dx"], 4 * (H + EPI) * U24 *
                                        r["dx_terms"]), "dx")
    assert dw.dtype == torch.float32
    assert_within(dw, r["dw"], (rows + H + 2 * EPI) * U24 * r["dw_abs"], "dw")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,H", NORM_SHAPES)
def test_layernorm_rows_mean_offset(rows, H, bias):
    x, w, b, dy = _norm_inputs(rows, H, 8.0)
    b = b if bias else None
    r = layernorm_ref(x, w, b, dy, 1e-5)
    y, mean, rstd = _ext().layernorm_fwd(x, w, b, 1e-5)
    # mean: (H + EPI) * 2^-24 * sum|x| / H; var = sum (x - mean)^2 / H is a
    # positive-term sum (condition 1) -> rstd relative (H + EPI) * 2^-24
    assert_within(mean, r["mean"], (H + EPI) * U24 * r["mean_abs"], "mean")
    assert_within(rstd, r["rstd"], (H + EPI) * U24 * r["rstd"], "rstd")
    assert_within(y, r["y"], bf16_tol(r["y"], (H + EPI + 3) * U24 *
                                      r["y_terms"]), "y")
    dx, dw, db = _ext().layernorm_bwd(dy, x, w, mean, rstd)
    assert_within(dx, r["dx"], bf16_tol(r["dx"], 4 * (H + EPI) * U24 *
                                        r["dx_terms"]), "dx")
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    assert_within(dw, r["dw"], (rows + H + 2 * EPI) * U24 * r["dw_abs"], "dw")
    assert_within(db, r["db"], (rows + EPI) * U24 * r["db_abs"], "db")


def _ce_check(logits, targets, what):
    r = ce_ref(logits, targets)
    loss, lse = _ext().cross_entropy_fwd(logits, targets, -100)
    v = r["valid"]
    assert_within(lse[v], r["lse"][v], r["lse_tol"][v], what + " lse")
    assert_within(loss, r["loss"], r["loss_tol"], what + " loss")
    dl = torch.linspace(0.25, 1.0, logits.shape[0], device=DEV)
    g = _ext().cross_entropy_bwd(logits, targets, lse, dl, -100)
    gref, slack = ce_grad_ref(r, dl)
    assert_within(g, gref, bf16_tol(gref, slack), what + " dlogits")
    return r, loss, g


CE_SHAPES = [(N, V) for V in (5, 8, 1000, 1001, 50257) for N in (1, 3)] + \
    [(2, 128256), (70000, 8)]   # last: rows beyond one gridDim.y


@pytest.mark.parametrize("N,V", CE_SHAPES)
def test_cross_entropy_sizes(N, V):
    torch.manual_seed(N + V)
    logits = (torch.randn(N, V, device=DEV) * 3.0 + 0.5).to(BF)
    targets = torch.randint(0, V, (N,), device=DEV)
    targets[0] = V - 1
    logits[-1, V - 1] = 30.0            # sentinel in the last column
    _ce_check(logits, targets, f"ce N={N} V={V}")


@pytest.mark.parametrize("V", [1000, 1001])
def test_cross_entropy_edge_rows(V):
    torch.manual_seed(V)
    logits = (torch.randn(5, V, device=DEV) * 2.0).to(BF)
    targets = torch.tensor([0, V - 1, V - 3, -100, 17], device=DEV)
    logits[3] = 100.0                   # ignored row with huge logits
    logits[4] = torch.randn(V, device=DEV).to(BF)
    logits[4, 500] = 60.0               # one huge logit among N(0, 1)
    r, loss, g = _ce_check(logits, targets, f"edge V={V}")
    assert loss[3].item() == 0.0
    assert torch.count_nonzero(g[3]).item() == 0, "ignored row grad != 0"


@pytest.mark.parametrize("V", [1000, 1001])
def test_cross_entropy_masked_columns(V):
    """-inf on columns [0:8] and [V-3:], target elsewhere: finite loss equal
    to torch's, and exactly zero gradient on the masked columns."""
    torch.manual_seed(V)
    logits = (torch.randn(3, V, device=DEV) * 2.0).to(BF)
    logits[:, :8] = float("-inf")
    logits[:, V - 3:] = float("-inf")
    targets = torch.tensor([8, V - 4, 500], device=DEV)
    r, loss, g = _ce_check(logits, targets, f"masked V={V}")
    assert torch.isfinite(loss).all()
    tref = torch.nn.functional.cross_entropy(logits.double(), targets,
                                             reduction="none")
    assert_within(loss, tref, r["loss_tol"], "loss vs torch")
    assert torch.count_nonzero(g[:, :8]).item() == 0
    assert torch.count_nonzero(g[:, V - 3:]).item() == 0


def test_cross_entropy_all_ignored():
    from deepspeed_amd.ops import functional as Fops
    torch.manual_seed(0)
    logits = (torch.randn(4, 1001, device=DEV) * 2.0).to(BF)
    logits[1] = 100.0
    logits.requires_grad_(True)
    targets = torch.full((4,), -100, device=DEV)
    loss = Fops.fused_cross_entropy(logits, targets)
    loss.backward()
    assert loss.item() == 0.0
    assert torch.count_nonzero(logits.grad).item() == 0
    assert not torch.isnan(logits.grad).any()


# ------------------------------------------------------------------- gemv
@pytest.mark.parametrize("N,K,B", [(1, 8, 1), (5, 1001, 2), (4095, 64, 1),
                                   (4096, 64, 3), (4099, 264, 2),
                                   (8, 4096, 4)])
def test_gemv_bf16(N, K, B):
    torch.manual_seed(N + K)
    rowscale = 0.5 + torch.arange(N, device=DEV, dtype=torch.float32) / N
    W = (torch.randn(N, K, device=DEV) * rowscale[:, None]).to(BF)
    x = (torch.randn(B, K, device=DEV) * 0.5 + 0.1).to(BF)
    x[:, -1] = 64.0                     # sentinel in the last element
    ref = x.double() @ W.double().t()
    terms = x.double().abs() @ W.double().abs().t()
    y = _ext().gemv_bf16(W, x)
    assert y.shape == (B, N)
    assert_within(y, ref, bf16_tol(ref, K * U24 * terms), "y")


# ------------------------------------------------------------------- misc
def test_l2norm_sq_list_tail_offset():
    torch.manual_seed(0)
    sizes = [1, 3, 4, 1023, 100003]
    tensors, adds, blocks = [], 0, 0
    for j, n in enumerate(sizes):
        t, sent = _flat(n, 1 if n == 1023 else 0, torch.float32,
                        scale=1.0 + j, vec=4)
        for i in sent:
            t[i] = SENT
        tensors.append(t)
        # launch geometry of the kernel: 256-thread blocks, one thread per
        # 4 elements, capped at 2048 blocks, then grid-stride
        grid = min(2048, max(1, ((n // 4 + 1) + 255) // 256))
        adds = max(adds, math.ceil(n / (grid * 256)))
        blocks += grid
    ref = sum(t.double().pow(2).sum() for t in tensors)
    out = _ext().l2norm_sq(tensors)
    # positive terms: (adds per thread + 8 tree steps + atomics) * 2^-24
    assert_within(out, ref, (adds + 8 + blocks) * U24 * ref, "l2norm_sq")


# ------------------------------------------------------------- optimizers
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def _opt_state(n, off, seed):
    torch.manual_seed(seed)
    p, _ = _flat(n, off, torch.float32, scale=1.0, shift=0.3, vec=4)
    g, _ = _flat(n, off, torch.float32, scale=2.0, vec=4)
    m, _ = _flat(n, off, torch.float32, scale=0.1, vec=4)
    v, _ = _flat(n, off, torch.float32, vec=4)
    v.abs_().mul_(0.01)
    o, _ = _flat(n, off, BF, vec=4)
    p[-1], g[-1] = 100.0, -30.0         # sentinel in the last element
    return p, g, m, v, o


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 7777])
def test_adam_all_arms_vs_float64(n, off):
    """Every adamw_mode / bias_correction / grad_scale / step / out16 arm
    against a float64 step on the fp32-rounded hyper-parameters. fp32
    state within a few fp32 ulps (2^-23) of its term magnitudes: m and v
    are 2-3 roundings, p is the decay multiply, the final subtract and a
    ~10-rounding update chain; out16 must be the RNE of the new p."""
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 0.01
    lrf, b1f, b2f, epsf, wdf = map(_f32, (lr, b1, b2, eps, wd))
    ulp = 2.0 ** -23
    for adamw, bc, gs, step, use16 in itertools.product(
            (0, 1), (0, 1), (1.0, 1.0 / 1024), (1, 1000), (False, True)):
        p, g, m, v, o = _opt_state(n, off, n + step)
        if gs != 1.0:
            g.mul_(1024.0)
        p0, g0, m0, v0 = (t.double() for t in (p, g, m, v))
        _ext().multi_tensor_adam([p], [g], [m], [v], lr, b1, b2, eps, step,
                                 adamw, bc, wd, [o] if use16 else [], gs)
        bc1 = 1.0 - _f32(b1f ** step) if bc else 1.0
        bc2 = 1.0 - _f32(b2f ** step) if bc else 1.0
        gk = g0 * gs
        pk = p0
        if adamw:
            pk = pk * (1.0 - _f32(lrf * wdf))
        else:
            gk = gk + wdf * p0
        mr = m0 * b1f + gk * (1.0 - b1f)
        vr = v0 * b2f + gk * gk * (1.0 - b2f)
        upd = (lrf / bc1) * mr / (vr.sqrt() / math.sqrt(bc2) + epsf)
        pr = pk - upd
        what = f"adamw={adamw} bc={bc} gs={gs} step={step} out16={use16}"
        assert_within(m, mr, 3 * ulp * ((m0 * b1f).abs() +
                                        (gk * (1 - b1f)).abs()), what + " m")
        assert_within(v, vr, 4 * ulp * vr.abs(), what + " v")
        assert_within(p, pr, ulp * (3 * p0.abs() + 8 * upd.abs()),
                      what + " p")
        if use16:
            assert torch.equal(o, p.to(BF)), what + " out16 != RNE(p)"


@pytest.mark.parametrize("n", [1, 1000])
def test_lion_out16(n):
    lr, b1, b2, wd = 1e-3, 0.9, 0.99, 0.1
    lrf, b1f, b2f, wdf = map(_f32, (lr, b1, b2, wd))
    p, g, m, _, o = _opt_state(n, 0, n)
    p0, g0, m0 = (t.double() for t in (p, g, m))
    u = m0 * b1f + g0 * (1 - b1f)
    assert u.abs().min() > 1e-6, "sign(u) must be unambiguous in fp32"
    _ext().multi_tensor_lion([p], [g], [m], lr, b1, b2, wd, [o])
    pr = p0 * (1.0 - _f32(lrf * wdf)) - lrf * torch.sign(u)
    mr = m0 * b2f + g0 * (1 - b2f)
    ulp = 2.0 ** -23
    assert_within(p, pr, ulp * (2 * p0.abs() + lrf), "p")
    assert_within(m, mr, 3 * ulp * ((m0 * b2f).abs() +
                                    (g0 * (1 - b2f)).abs()), "m")
    assert torch.equal(o, p.to(BF))


@pytest.mark.parametrize("n", [1, 1000])
def test_adagrad_out16(n):
    lr, eps, wd = 1e-2, 1e-8, 0.01
    lrf, epsf, wdf = map(_f32, (lr, eps, wd))
    p, g, _, h, o = _opt_state(n, 0, n)
    p0, g0, h0 = (t.double() for t in (p, g, h))
    _ext().multi_tensor_adagrad([p], [g], [h], lr, eps, wd, [o])
    gk = g0 + wdf * p0
    hr = h0 + gk * gk
    upd = lrf * gk / (hr.sqrt() + epsf)
    ulp = 2.0 ** -23
    assert_within(h, hr, 4 * ulp * hr.abs(), "h")
    assert_within(p, p0 - upd, ulp * (p0.abs() + 8 * upd.abs()), "p")
    assert torch.equal(o, p.to(BF))


@pytest.mark.parametrize("sizes", [(1,), (1000, 5000)])
def test_lamb_trust_ratio_and_out16(sizes):
    """Two tensors of very different norms in one call: tensor t must use
    workspace slots [2t, 2t+1]. Trust ratio vs float64."""
    lr, b1, b2, eps, wd, step = 1e-2, 0.9, 0.999, 1e-6, 0.01, 3
    lrf, b1f, b2f, epsf, wdf = map(_f32, (lr, b1, b2, eps, wd))
    bc1 = 1.0 - _f32(b1f ** step)
    bc2 = 1.0 - _f32(b2f ** step)
    ps, gs, us, ms, vs, os_ = [], [], [], [], [], []
    for j, n in enumerate(sizes):
        p, g, m, v, o = _opt_state(n, 0, n)
        p.mul_(1e-3 if j == 0 else 1e2)
        for lst, t in ((ps, p), (gs, g), (ms, m), (vs, v), (os_, o),
                       (us, torch.empty_like(p))):
            lst.append(t)
    p0s = [p.double() for p in ps]
    urs = []
    for p0, g, m, v in zip(p0s, gs, ms, vs):
        mr = m.double() * b1f + g.double() * (1 - b1f)
        vr = v.double() * b2f + g.double() ** 2 * (1 - b2f)
        urs.append((mr / bc1) / ((vr / bc2).sqrt() + epsf) + wdf * p0)
    ws = torch.zeros(2 * len(sizes), device=DEV)
    _ext().multi_tensor_lamb(ps, gs, us, ms, vs, ws, lr, b1, b2, eps, step,
                             1, wd, os_, 1.0)
    ulp = 2.0 ** -23
    for t, n in enumerate(sizes):
        grid = min(2048, (n + 255) // 256)
        k = (math.ceil(n / (grid * 256)) + 8 + grid) * U24   # positive sums
        psq, usq = p0s[t].pow(2).sum(), urs[t].pow(2).sum()
        assert_within(ws[2 * t], psq, k * psq, f"ws[{2 * t}] = |p|^2")
        # u itself carries ~8 roundings, squared: 16 more units
        assert_within(ws[2 * t + 1], usq, (k + 16 * U24) * usq,
                      f"ws[{2 * t + 1}] = |u|^2")
        ratio = (psq / usq).sqrt()
        upd = lrf * ratio * urs[t]
        # ratio: half of both sums' errors + sqrt, divide; u: ~8 roundings;
        # lr * ratio * u: 2 more -> k + 20 units on the update
        assert_within(ps[t], p0s[t] - upd,
                      ulp * p0s[t].abs() + (k + 20 * U24) * upd.abs(),
                      f"p[{t}]")
        assert torch.equal(os_[t], ps[t].to(BF))


# ------------------------------------------------------------- quantizers
ZERO_G = 2      # index of the all-zero group in _quant_groups


def _int_ties(group, qmax):
    """(k + 0.5) for k in -(qmax-1)..(qmax-1), cycled; last element qmax."""
    ks = torch.arange(group) % int(2 * qmax - 1) - (qmax - 1)
    t = ks.float() + 0.5
    t[-1] = qmax
    return t


def _fp8_ties(group):
    """Mid-points of adjacent e4m3 values (odd/16 * 2^e), cycled, both
    signs; last element 448 (the format maximum)."""
    mids = [(2 * m + 1) / 16.0 * 2.0 ** e * sgn
            for e in range(-6, 8) for m in range(8, 16) for sgn in (1, -1)]
    t = torch.tensor([mids[i % len(mids)] for i in range(group)])
    t[-1] = 448.0
    return t


def _quant_groups(group, ties):
    """CPU bf16 [random | random*37 | zero | outlier | half-way ties].

    The ties group is `ties` * 2^-3 with max |ties| = the format maximum,
    so its scale is exactly 2^-3, every element is an exact bf16 value and
    its quotient by the scale is exactly the half-way point -- this pins
    round-to-nearest-EVEN."""
    torch.manual_seed(group)
    rnd = torch.randn(group)
    outl = torch.randn(group) * 0.01
    outl[group // 2] = 300.0
    ties = ties * 0.125
    x = torch.cat([rnd, rnd.flip(0) * 37.0, torch.zeros(group), outl,
                   ties]).to(BF)
    assert torch.equal(x[4 * group:].float(), ties)     # exact in bf16
    return x


def _int_codes_ref(x, group, qmax):
    """Codes by the defining formula rint(x / scale) in fp32 on the CPU,
    and the count of elements where the kernel's x * (1 / scale) form
    rounds differently (must be 0 on the chosen inputs)."""
    g = x.float().reshape(-1, group)
    amax = g.abs().amax(1, keepdim=True)
    scale = torch.where(amax > 0, amax / qmax, torch.ones_like(amax))
    div = torch.clamp(torch.round(g / scale), -qmax, qmax)
    mul = torch.clamp(torch.round(g * (1.0 / scale)), -qmax, qmax)
    return div.to(torch.int32), scale.reshape(-1), int((div != mul).sum())


def _fp8_codes_ref(x, group):
    g = x.float().reshape(-1, group)
    amax = g.abs().amax(1, keepdim=True)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    div = (g / scale).to(torch.float8_e4m3fn).view(torch.uint8)
    mul = (g * (1.0 / scale)).to(torch.float8_e4m3fn).view(torch.uint8)
    return div, scale.reshape(-1), int((div != mul).sum())


def _zero_group_ok(q, s, group, per=1):
    lo, hi = ZERO_G * group // per, (ZERO_G + 1) * group // per
    return s[ZERO_G].item() == 1.0 and \
        torch.count_nonzero(q[lo:hi].to(torch.int32)).item() == 0


@pytest.mark.parametrize("group", [2, 64, 512, 4096])
def test_quantize_int8_exact(group):
    x = _quant_groups(group, _int_ties(group, 127))
    codes, scale, differ = _int_codes_ref(x, group, 127.0)
    assert differ == 0, "inputs must not hit x*inv vs x/scale tie splits"
    q, s = _ext().quantize_int8(x.to(DEV), group)
    assert torch.equal(s.cpu(), scale), "scale != amax / 127 in fp32"
    assert _zero_group_ok(q, s, group)
    assert torch.equal(q.cpu().to(torch.int32).reshape(-1, group), codes)
    deq = _ext().dequantize_int8(q, s, group)
    ref = (codes.float() * scale[:, None]).reshape(-1).to(BF)
    assert torch.equal(deq.cpu(), ref)


@pytest.mark.parametrize("group", [2, 64, 512, 4096])
def test_quantize_fp8_exact(group):
    """Codes decoded by torch's float8_e4m3fn == torch's own cast of
    x / scale; scales == amax / 448 in fp32."""
    x = _quant_groups(group, _fp8_ties(group))
    codes, scale, differ = _fp8_codes_ref(x, group)
    assert differ == 0, "inputs must not hit x*inv vs x/scale tie splits"
    q, s = _ext().quantize_fp8(x.to(DEV), group)
    assert torch.equal(s.cpu(), scale), "scale != amax / 448 in fp32"
    assert _zero_group_ok(q, s, group)
    got = q.cpu().reshape(-1, group).view(torch.float8_e4m3fn).float()
    assert torch.equal(got, codes.view(torch.float8_e4m3fn).float())
    deq = _ext().dequantize_fp8(q, s, group)
    ref = (codes.view(torch.float8_e4m3fn).float() *
           scale[:, None]).reshape(-1).to(BF)
    assert torch.equal(deq.cpu(), ref)


def _ragged(numel, group):
    x = _quant_groups(group, _int_ties(group, 7))
    reps = (numel + x.numel() - 1) // x.numel()
    return x.repeat(reps)[:numel].contiguous()


INT4_CASES = [(g, 5 * g) for g in (2, 64, 512, 4096)] + \
    [(64, 1), (64, 129), (64, 4096 + 3)]


@pytest.mark.parametrize("group,numel", INT4_CASES)
def test_quantize_int4_exact_and_ragged(group, numel):
    x = _ragged(numel, group)
    pad = (-numel) % group
    xp = torch.nn.functional.pad(x, (0, pad))
    codes, scale, differ = _int_codes_ref(xp, group, 7.0)
    assert differ == 0, "inputs must not hit x*inv vs x/scale tie splits"
    q, s = _ext().quantize_int4(x.to(DEV), group)
    assert torch.equal(s.cpu(), scale), "scale != amax / 7 in fp32"
    if numel >= (ZERO_G + 1) * group:
        assert _zero_group_ok(q, s, group, per=2)
    flat = codes.reshape(-1)
    packed = ((flat[0::2] & 0xF) | ((flat[1::2] & 0xF) << 4)).to(torch.uint8)
    nbytes = (numel + 1) // 2          # bytes past the ragged end are unset
    assert torch.equal(q.cpu()[:nbytes], packed[:nbytes])
    deq = _ext().dequantize_int4(q, s, group, numel)
    ref = (codes.float() * scale[:, None]).reshape(-1)[:numel].to(BF)
    assert torch.equal(deq.cpu(), ref)


@pytest.mark.parametrize("qbits", [4, 6, 12])
@pytest.mark.parametrize("group,numel", INT4_CASES)
def test_quantize_fp_em_codes_and_ragged(group, numel, qbits):
    from deepspeed_amd.ops.fp_quantizer import (_FMT, _decode_torch,
                                                _encode_torch, _fmt_max)
    E, M = _FMT[qbits]
    x = _ragged(numel, group)
    pad = (-numel) % group
    g = torch.nn.functional.pad(x.float(), (0, pad)).reshape(-1, group)
    amax = g.abs().amax(1)
    scale = torch.where(amax > 0, amax / _fmt_max(E, M),
                        torch.ones_like(amax))
    codes = _encode_torch(g / scale[:, None], E, M).reshape(-1)[:numel]
    q, s = _ext().quantize_fp_em(x.to(DEV), qbits, group)
    assert torch.equal(s.cpu(), scale), "scale != amax / fmt_max in fp32"
    assert torch.equal(q.cpu().to(torch.int32), codes.to(torch.int32))
    if numel >= (ZERO_G + 1) * group:
        assert _zero_group_ok(q.cpu(), s, group)
    deq = _ext().dequantize_fp_em(q, s, qbits, group, [numel])
    dec = torch.nn.functional.pad(_decode_torch(codes, E, M), (0, pad))
    ref = (dec.reshape(-1, group) * scale[:, None]).reshape(-1)[:numel].to(BF)
    assert torch.equal(deq.cpu(), ref)


# -------------------------------------------------- strides and contracts
def test_strided_inputs_fwd_bwd_gpu():
    fails = strided_cases(torch.device(DEV), BF)
    assert not fails, "\n".join(fails)


def test_raw_entry_points_reject_bad_arguments():
    """Wrong dtype or non-contiguous arguments raise instead of being
    reinterpreted. Every argument would be in bounds anyway."""
    e = _ext()
    rows, H = 8, 64
    x = torch.randn(rows, H, device=DEV).to(BF)
    xt = torch.randn(H, rows, device=DEV).to(BF).t()       # strided [rows,H]
    w = torch.randn(H, device=DEV).to(BF)
    st = torch.ones(rows, device=DEV)
    tg = torch.zeros(rows, dtype=torch.long, device=DEV)
    tg_strided = torch.zeros(2 * rows, dtype=torch.long, device=DEV)[::2]
    q16 = torch.zeros(rows * H, dtype=torch.int16, device=DEV)
    f = torch.randn(rows * H, device=DEV)
    q8 = torch.zeros(rows * H, dtype=torch.int8, device=DEV)
    sc = torch.ones(rows, device=DEV)
    bad_calls = [
        lambda: e.rmsnorm_fwd(xt, w, 1e-5),
        lambda: e.rmsnorm_fwd(x, w.float(), 1e-5),
        lambda: e.rmsnorm_bwd(x, xt, w, st),
        lambda: e.rmsnorm_bwd(x.float(), x, w, st),
        lambda: e.layernorm_fwd(xt, w, None, 1e-5),
        lambda: e.layernorm_fwd(x, w, w.float(), 1e-5),
        lambda: e.layernorm_bwd(x, xt, w, st, st),
        lambda: e.layernorm_bwd(x, x, w, st.double(), st),
        lambda: e.swiglu_fwd(x, xt),
        lambda: e.swiglu_fwd(x, x.float()),
        lambda: e.swiglu_bwd(xt, x, x),
        lambda: e.swiglu_bwd(x, x, x.float()),
        lambda: e.cross_entropy_fwd(xt, tg, -100),
        lambda: e.cross_entropy_fwd(x, tg_strided, -100),
        lambda: e.cross_entropy_bwd(xt, tg, st, st, -100),
        lambda: e.cross_entropy_bwd(x, tg, st.double(), st, -100),
        lambda: e.gemv_bf16(xt, w.reshape(1, H)),
        lambda: e.gemv_bf16(x, w.float().reshape(1, H)),
        lambda: e.accum_bf16_to_f32(f, f, 1.0),
        lambda: e.accum_bf16_to_f32(f.reshape(rows, H).t(), x, 1.0),
        lambda: e.l2norm_sq([f, f.double()]),
        lambda: e.l2norm_sq([f.reshape(H, rows).t()]),
        lambda: e.dequantize_int8(q8.view(torch.uint8), sc, H),
        lambda: e.dequantize_int8(q8, sc.double(), H),
        lambda: e.dequantize_fp8(q8, sc, H),
        lambda: e.dequantize_int4(q8, sc, H, rows * H),
        lambda: e.dequantize_fp_em(q16, sc, 4, H, [rows * H]),
        lambda: e.quantize_int8(xt, H),
        lambda: e.multi_tensor_adam([f], [f.clone().double()], [f.clone()],
                                    [f.clone()], 1e-3, 0.9, 0.999, 1e-8, 1,
                                    1, 1, 0.0, [], 1.0),
        lambda: e.multi_tensor_adam([f], [f.clone()], [f.clone()],
                                    [f.clone()], 1e-3, 0.9, 0.999, 1e-8, 1,
                                    1, 1, 0.0, [f.clone()], 1.0),
        lambda: e.multi_tensor_lion([f], [f.reshape(H, rows).t()],
                                    [f.clone()], 1e-3, 0.9, 0.99, 0.0, []),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"bad call #{i} did not raise")
