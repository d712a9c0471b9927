"""rope_qk: q and k rotated by one launch (needs MI355X). Must be bit-identical
to two `rope` calls; also what the fused attention function of the training
path returns and differentiates to."""
import pytest
import torch

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
