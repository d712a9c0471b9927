"""rope_qk: q and k rotated by one launch (needs MI355X). Must be bit-identical
to two `rope` calls and within the float64 rotation bound of
test_kernel_edges_gpu.test_rope_shapes_and_pos0 at every head width the entry
point admits; also what the fused attention function of the training path
returns and differentiates to, checked against the float64 attention
reference un-rotated by attn_refs.unrotate_ref."""
import math

import pytest
import torch

from attn_refs import (attention_ref, make_inputs, make_rope_tables,
                       unrotated_grads)
from edge_refs import assert_within, bf16_tol
from test_kernel_edges_gpu import _rope_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("Hq,Hk", [(4, 1), (6, 2), (3, 5)])
def test_one_launch_equals_two_rope_calls(D, S, Hq, Hk):
    from deepspeed_amd.ops.functional import build_rope_cache
    ext = get_ext(required=True)
    B = 2
    torch.manual_seed(D + 10 * S + Hq)
    q = torch.randn(B, S, Hq, D, device=DEV).to(BF)
    k = (torch.randn(B, S, Hk, D, device=DEV) * 3.0).to(BF)
    q[-1, -1, -1, -1] = 1000.0          # last element of each tensor
    k[-1, -1, -1, -1] = -1000.0
    cos, sin = build_rope_cache(S + 2, D, device=DEV)   # longer than S
    q0, k0 = q.clone(), k.clone()
    qo, ko = ext.rope_qk(q, k, cos, sin)
    qr, kr = torch.empty_like(q), torch.empty_like(k)
    ext.rope(qr, q, cos, sin, 0, False)
    ext.rope(kr, k, cos, sin, 0, False)
    assert torch.equal(_bits(qo), _bits(qr))
    assert torch.equal(_bits(ko), _bits(kr))
    assert torch.equal(_bits(q), _bits(q0)) and torch.equal(_bits(k), _bits(k0))


def test_rope_qk_contract():
    from deepspeed_amd.ops.functional import build_rope_cache
    ext = get_ext(required=True)
    q = torch.randn(2, 5, 4, 64, device=DEV).to(BF)
    k = torch.randn(2, 5, 2, 64, device=DEV).to(BF)
    cos, sin = build_rope_cache(5, 64, device=DEV)
    ext.rope_qk(q, k, cos, sin)                       # exactly fits
    for bad in (lambda: ext.rope_qk(q, k, cos[:4], sin[:4]),
                lambda: ext.rope_qk(q, k[:, :4].contiguous(), cos, sin),
                lambda: ext.rope_qk(q.float(), k, cos, sin),
                lambda: ext.rope_qk(q, k, cos.cpu(), sin.cpu()),
                lambda: ext.rope_qk(q.transpose(1, 2), k, cos, sin)):
        with pytest.raises(RuntimeError):
            bad()


@pytest.mark.parametrize("D", [64, 128])
def test_training_path_matches_unfused_route(D):
    """rope_flash_attention (one rope launch, inverse rotation inside flash
    backward) against apply_rope + flash_attention: same forward bits, and
    gradients that agree to the two bf16 roundings the unfused route makes
    (one ulp each: flash backward's store, then the rope kernel's)."""
    from deepspeed_amd.ops.attention import (flash_attention,
                                             rope_flash_attention)
    from deepspeed_amd.ops.functional import apply_rope, build_rope_cache
    B, S, Hq, Hk = 2, 130, 4, 2
    torch.manual_seed(D)
    cos, sin = build_rope_cache(S, D, device=DEV)
    base = [torch.randn(B, S, H, D, device=DEV).to(BF) for H in (Hq, Hk, Hk)]
    dout = torch.randn(B, S, Hq, D, device=DEV).to(BF)

    def run(fused):
        q, k, v = [t.clone().requires_grad_(True) for t in base]
        if fused:
            o = rope_flash_attention(q, k, v, cos, sin, causal=True)
            assert o is not None
        else:
            o = flash_attention(apply_rope(q, cos, sin),
                                apply_rope(k, cos, sin), v, causal=True)
        o.backward(dout)
        return o, q.grad, k.grad, v.grad

    of, dqf, dkf, dvf = run(True)
    ou, dqu, dku, dvu = run(False)
    assert torch.equal(_bits(of), _bits(ou))
    assert torch.equal(_bits(dvf), _bits(dvu))
    for name, a, b in (("dq", dqf, dqu), ("dk", dkf, dku)):
        # Pair (d1, d2) before rotation, M = max(|d1|, |d2|), RNE relative
        # error <= 2^-8. Unfused: the stored d1, d2 are off by <= 2^-8 M,
        # which the rotation turns into <= 2^-8 M (|cos| + |sin|)
        # <= 2^-8 sqrt(2) M; each route's final rounding adds <= 2^-8 times
        # a result of magnitude <= sqrt(2) M. Sum: 3 * 2^-8 * sqrt(2) * M.
        # The rotation keeps d1^2 + d2^2, so M <= sqrt(2) * mag with mag the
        # larger partner after rotation: |a - b| <= 6 * 2^-8 * mag (mag is
        # taken from the rounded b, hence the factor 1 + 2^-7).
        a, b = a.double(), b.double()
        half = D // 2
        mag = torch.maximum(b[..., :half].abs(), b[..., half:].abs())
        tol = 6.0 * 2.0 ** -8 * (1 + 2.0 ** -7) * torch.cat([mag, mag], -1)
        assert ((a - b).abs() <= tol + 1e-30).all(), name


# ---------------------------------------------------- every admitted width
# (B, S, Hq, Hk): several workgroups with Hq + Hk odd, one vector per head
# half at D = 16, and a single k head behind eight q heads
QK_SHAPES = [(3, 257, 5, 2), (1, 1, 1, 1), (2, 130, 8, 1)]
QK_WIDTHS = [16, 32, 48, 64, 96, 128]
SENT = 1000.0


@pytest.mark.parametrize("D", QK_WIDTHS)
@pytest.mark.parametrize("B,S,Hq,Hk", QK_SHAPES)
def test_rope_qk_widths_vs_rope_and_float64(B, S, Hq, Hk, D):
    ext = get_ext(required=True)
    torch.manual_seed(D + 10 * S + Hq)
    q = (torch.randn(B, S, Hq, D, device=DEV) * 2.0).to(BF)
    k = (torch.randn(B, S, Hk, D, device=DEV) * 3.0).to(BF)
    # last element of each tensor and the first of k: the h == Hq hand-over
    q.view(-1)[-1] = SENT
    k.view(-1)[-1] = -SENT
    k.view(-1)[0] = SENT
    cos, sin = make_rope_tables(S, D, 3, device=DEV, seed=Hq)
    assert torch.isnan(cos[S:]).all() and torch.isnan(sin[S:]).all()
    q0, k0 = q.clone(), k.clone()
    qo, ko = ext.rope_qk(q, k, cos, sin)
    assert torch.equal(_bits(q), _bits(q0)) and torch.equal(_bits(k), _bits(k0))
    for name, t, o in (("q", q, qo), ("k", k, ko)):
        assert o.shape == t.shape and o.dtype == BF and o.is_contiguous()
        assert not torch.isnan(o.float()).any(), f"{name}: NaN"
        two = torch.empty_like(t)
        ext.rope(two, t, cos, sin, 0, False)
        assert torch.equal(_bits(o), _bits(two)), f"{name}: != rope"
        ref, terms = _rope_ref(t, cos, sin, 0, 1.0)
        assert_within(o, ref, bf16_tol(ref, 1e-6 * terms), f"rope_qk {name}")


@pytest.mark.parametrize("B,S", [(0, 5), (2, 0)])
def test_rope_qk_zero_size(B, S):
    """Nothing to rotate: empty outputs of the right shape, and the table is
    not looked at (it has no rows at all)."""
    ext = get_ext(required=True)
    q = torch.empty(B, S, 4, 64, device=DEV, dtype=BF)
    k = torch.empty(B, S, 2, 64, device=DEV, dtype=BF)
    cos = torch.empty(0, 32, device=DEV)
    qo, ko = ext.rope_qk(q, k, cos, cos.clone())
    assert qo.shape == q.shape and ko.shape == k.shape
    assert qo.dtype == BF and ko.dtype == BF
    torch.cuda.synchronize()


# ------------------------------------------- rope_flash_attention, autograd
@pytest.mark.parametrize("D", [64, 128])
def test_rope_flash_attention_views_vs_float64(D):
    """q, k, v are column slices of one fused projection buffer and the
    upstream gradient is a strided view. Reference: attention_ref on the bf16
    qr, kr that rope_qk returns for the same inputs (forward attends over
    exactly those), its dq / dk un-rotated in float64."""
    from deepspeed_amd.ops.attention import rope_flash_attention
    ext = get_ext(required=True)
    B, S, Hq, Hk = 2, 130, 4, 2
    c = dict(S=S, D=D, Hq=Hq, Hk=Hk, causal=True, custom=False, mask=None)
    q, k, v, do, _ = make_inputs(c, DEV)
    cos, sin = make_rope_tables(S, D, 3, device=DEV)
    buf = torch.cat([t.reshape(B, S, -1) for t in (q, k, v)], -1) \
        .contiguous().requires_grad_(True)
    nq, nk = Hq * D, Hk * D
    qv = buf[..., :nq].view(B, S, Hq, D)
    kv = buf[..., nq:nq + nk].view(B, S, Hk, D)
    vv = buf[..., nq + nk:].view(B, S, Hk, D)
    assert not (qv.is_contiguous() or kv.is_contiguous() or
                vv.is_contiguous())
    g = torch.empty(B, S, Hq, 2 * D, device=DEV, dtype=BF)[..., ::2]
    g.copy_(do)
    assert not g.is_contiguous()
    out = rope_flash_attention(qv, kv, vv, cos, sin, causal=True)
    assert out is not None
    out.backward(g)
    grad = buf.grad
    dq = grad[..., :nq].view(B, S, Hq, D)
    dk = grad[..., nq:nq + nk].view(B, S, Hk, D)
    dv = grad[..., nq + nk:].view(B, S, Hk, D)

    qr, kr = ext.rope_qk(q, k, cos, sin)
    ref = attention_ref(qr, kr, v, True, 1.0 / math.sqrt(D), None, do)
    un = unrotated_grads(ref, cos, sin)
    assert_within(out, ref["out"], ref["out_tol"], "out")
    assert_within(dq, un["dq"], un["dq_tol"], "dq")
    assert_within(dk, un["dk"], un["dk_tol"], "dk")
    assert_within(dv, ref["dv"], ref["dv_tol"], "dv")


def test_rope_flash_attention_returns_none_off_its_path():
    """None leaves the caller to apply_rope + flash_attention."""
    from deepspeed_amd.ops.attention import rope_flash_attention
    from deepspeed_amd.ops.functional import build_rope_cache
    B, S, Hq, Hk, D = 2, 33, 4, 2, 64
    half = D // 2

    def qkv(d):
        return [torch.randn(B, S, H, d, device=DEV).to(BF)
                for H in (Hq, Hk, Hk)]

    q, k, v = qkv(D)
    cos, sin = build_rope_cache(S, D, device=DEV)
    assert rope_flash_attention(q, k, v, cos, sin) is not None

    def off4(t):            # same values, base 4 bytes past 16-byte alignment
        big = torch.empty(t.numel() + 4, device=DEV)
        assert big.data_ptr() % 16 == 0
        o = big[1:1 + t.numel()].view(t.shape)
        o.copy_(t)
        assert o.is_contiguous() and o.data_ptr() % 16 == 4
        return o

    assert rope_flash_attention(q, k, v, off4(cos), off4(sin)) is None
    assert rope_flash_attention(q, k, v, cos, off4(sin)) is None
    rows = cos.unsqueeze(0).expand(B, S, half).contiguous()     # per-row
    assert rope_flash_attention(q, k, v, rows, rows.clone()) is None
    c32, s32 = build_rope_cache(S, 32, device=DEV)
    assert rope_flash_attention(*qkv(32), c32, s32) is None     # D = 32
    assert rope_flash_attention(q, k, v, cos[:S - 1], sin[:S - 1]) is None
