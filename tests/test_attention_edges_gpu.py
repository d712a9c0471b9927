"""Flash attention forward / backward HIP kernels at their tile, mask, GQA
and contract edges (needs MI355X).

Every comparison is elementwise against the float64 closed-form reference
of attn_refs.py on the same bf16 inputs, with the bounds derived there;
test_attention_refs_cpu.py shows on the same cases that those bounds hold
for a faithful emulation and fail for one dropped key, an ignored mask, an
off-by-one causal rule, a wrong head / batch mapping or a wrong scale.
"""
import math

import pytest
import torch

from attn_refs import (ATTN_CASES, attention_ref, case_id, case_scale,
                       check_attention, make_inputs)
from edge_refs import assert_within

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16


def _ext():
    return get_ext(required=True)


@pytest.mark.parametrize("c", ATTN_CASES, ids=case_id)
def test_flash_fwd_bwd_vs_float64(c):
    q, k, v, do, mask = make_inputs(c, DEV)
    scale = case_scale(c)
    ref = attention_ref(q, k, v, c["causal"], scale, mask, do)
    out, lse = _ext().flash_attn_fwd(q, k, v, c["causal"], scale, mask)
    dq, dk, dv = _ext().flash_attn_bwd(q, k, v, do, out, lse, c["causal"],
                                       scale, mask)
    check_attention(dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), ref,
                    case_id(c))


# ------------------------------------------------- through flash_attention
def _wrapper_case(mask_shape):
    """q/k/v as transposed views of [B,H,S,D] storage, a non-contiguous
    upstream gradient, and a left-padding mask in the given layout."""
    from deepspeed_amd.ops.attention import flash_attention
    c = dict(S=130, D=64, Hq=4, Hk=2, causal=False, custom=False,
             mask="left", arg=65)
    q, k, v, do, mask = make_inputs(c, DEV)
    B, S = mask.shape
    if mask_shape == "B11S":
        am = mask.view(B, 1, 1, S)
    elif mask_shape == "B1S":
        am = mask.view(B, 1, S)
    else:                       # one row for the whole batch
        mask = mask[:1].expand(B, S).contiguous()
        am = mask[:1].view(1, 1, 1, S) if mask_shape == "111S" else mask
    leaves = [t.permute(0, 2, 1, 3).contiguous().requires_grad_(True)
              for t in (q, k, v)]
    qv, kv, vv = (t.permute(0, 2, 1, 3) for t in leaves)
    assert not qv.is_contiguous() and not kv.is_contiguous()
    g = torch.empty(B, S, 4, 2 * 64, device=DEV, dtype=BF)[..., ::2]
    g.copy_(do)
    assert not g.is_contiguous()
    out = flash_attention(qv, kv, vv, causal=False, attn_mask=am)
    out.backward(g)
    grads = [t.grad.permute(0, 2, 1, 3) for t in leaves]
    return (q, k, v, do, mask), out, grads


@pytest.mark.parametrize("mask_shape", ["B11S", "111S", "B1S"])
def test_flash_attention_wrapper_views_and_mask_shapes(mask_shape):
    (q, k, v, do, mask), out, (dq, dk, dv) = _wrapper_case(mask_shape)
    ref = attention_ref(q, k, v, False, 1.0 / math.sqrt(64), mask, do)
    for name, got in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert_within(got, ref[name], ref[name + "_tol"],
                      f"{mask_shape} {name}")
    if mask_shape == "111S":    # same as the expanded [B,S] mask, bit for bit
        _, out2, grads2 = _wrapper_case("BS_expanded")
        assert torch.equal(out, out2)
        for a, b in zip((dq, dk, dv), grads2):
            assert torch.equal(a, b)


# ---------------------------------------------------------------- contract
def test_scale_zero_means_default_scale():
    c = dict(S=65, D=64, Hq=4, Hk=2, causal=True, custom=False, mask=None)
    q, k, v, do, _ = make_inputs(c, DEV)
    e = _ext()
    explicit = 1.0 / math.sqrt(64)
    out0, lse0 = e.flash_attn_fwd(q, k, v, True, 0.0)
    out1, lse1 = e.flash_attn_fwd(q, k, v, True, explicit)
    outd, lsed = e.flash_attn_fwd(q, k, v)          # binding default
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1)
    assert torch.equal(outd, out1) and torch.equal(lsed, lse1)
    g0 = e.flash_attn_bwd(q, k, v, do, out1, lse1, True, 0.0)
    g1 = e.flash_attn_bwd(q, k, v, do, out1, lse1, True, explicit)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    ref = attention_ref(q, k, v, True, explicit, None, do)
    check_attention(dict(out=out0, lse=lse0, dq=g0[0], dk=g0[1], dv=g0[2]),
                    ref, "scale=0")


def test_flash_entry_points_reject_bad_arguments():
    """Every mismatch raises. Each bad tensor is at least as large as the
    good one it replaces (or a leading view of a larger buffer), so all
    indexing would stay inside the tensors passed even without the check."""
    e = _ext()
    B, S, Hq, Hk, D = 2, 32, 4, 2, 64

    def t(*shape, dtype=BF):
        return torch.zeros(*shape, device=DEV, dtype=dtype)

    q, k, v = t(B, S, Hq, D), t(B, S, Hk, D), t(B, S, Hk, D)
    do, out, lse = t(B, S, Hq, D), t(B, S, Hq, D), t(B, Hq, S,
                                                     dtype=torch.float32)
    k3 = t(B + 1, S, 3, D)[:B]              # Hk = 3: Hq % Hk != 0
    assert k3.is_contiguous()
    kstr = t(B, 2 * S, Hk, D)[:, ::2]       # strided
    bad_kv = [
        ("k dtype", dict(k=k.float())),
        ("v dtype", dict(v=v.float())),
        ("q dtype", dict(q=q.float())),
        ("Sk != Sq", dict(k=t(B, 2 * S, Hk, D), v=t(B, 2 * S, Hk, D))),
        ("v S", dict(v=t(B, 2 * S, Hk, D))),
        ("k D", dict(k=t(B, S, Hk, 2 * D))),
        ("v D", dict(v=t(B, S, Hk, 2 * D))),
        ("k B", dict(k=t(B + 1, S, Hk, D), v=t(B + 1, S, Hk, D))),
        ("v Hk", dict(v=t(B, S, 2 * Hk, D))),
        ("Hq % Hk", dict(k=k3, v=k3.clone())),
        ("k strided", dict(k=kstr)),
        ("k device", dict(k=k.cpu())),
        ("v device", dict(v=v.cpu())),
        ("k 3-d", dict(k=t(B, S, Hk * D))),
        ("mask dtype", dict(kvmask=t(B, S, dtype=torch.float64))),
        ("mask numel", dict(kvmask=t(B, 2 * S, dtype=torch.float32))),
        ("mask device", dict(kvmask=torch.zeros(B, S))),
    ]
    bad_bwd = [
        ("dout dtype", dict(dout=do.float())),
        ("out dtype", dict(out=out.float())),
        ("lse dtype", dict(lse=lse.double())),
        ("dout shape", dict(dout=t(B, 2 * S, Hq, D))),
        ("out shape", dict(out=t(B, S, 2 * Hq, D))),
        ("lse shape", dict(lse=t(B, Hq, 2 * S, dtype=torch.float32))),
        ("lse layout", dict(lse=t(B, S, Hq, dtype=torch.float32))),
        ("dout strided", dict(dout=t(B, S, Hq, 2 * D)[..., ::2])),
        ("dout device", dict(dout=do.cpu())),
        ("lse device", dict(lse=lse.cpu())),
    ]
    good = dict(q=q, k=k, v=v, dout=do, out=out, lse=lse, kvmask=None)
    e.flash_attn_fwd(q, k, v, False, 0.125, None)           # the good call
    e.flash_attn_bwd(q, k, v, do, out, lse, False, 0.125, None)

    def fwd(a):
        return e.flash_attn_fwd(a["q"], a["k"], a["v"], False, 0.125,
                                a["kvmask"])

    def bwd(a):
        return e.flash_attn_bwd(a["q"], a["k"], a["v"], a["dout"], a["out"],
                                a["lse"], False, 0.125, a["kvmask"])

    for name, change in bad_kv:
        for fn in (fwd, bwd):
            with pytest.raises(RuntimeError):
                fn({**good, **change})
                pytest.fail(f"{fn.__name__}: '{name}' did not raise")
    for name, change in bad_bwd:
        with pytest.raises(RuntimeError):
            bwd({**good, **change})
            pytest.fail(f"bwd: '{name}' did not raise")
