"""Inverse RoPE fused into the flash backward epilogues (needs MI355X).

With cos/sin tables `flash_attn_bwd` takes the rotated q and k that forward
attended over and returns dq, dk with respect to the un-rotated tensors.
Three routes are compared per case:
  (a) the fused call;
  (b) the unfused route: flash_attn_bwd without tables, then
      rope(..., backward=True) on dq and dk;
  (c) the closed-form reference of attn_refs.attention_ref, un-rotated with
      _rope_torch(sign=-1).
(a) rounds to bf16 once where (b) rounds twice, so its max abs error against
(c) may not exceed (b)'s by more than one bf16 ulp at max|c| (2^-8 * max|c|:
a different element may land on the maximum). dv does not see the tables and
must be bit-identical.
"""
import itertools

import pytest
import torch

from attn_refs import attention_ref, case_id, case_scale, make_inputs

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"


def _c(S, D, H, causal, mask=None, arg=None, extra=0):
    return dict(S=S, D=D, Hq=H[0], Hk=H[1], causal=causal, custom=False,
                mask=mask, arg=arg, extra=extra)


# S: 1, the padded tail of one 128-row block (33), two blocks (130, 257)
CASES = [_c(S, D, H, causal)
         for D, S, H, causal in itertools.product(
             (64, 128), (1, 33, 130, 257), ((4, 4), (8, 2)), (True, False))]
CASES += [
    _c(130, 128, (8, 2), False, mask="tail", arg=97),   # kv padding mask
    _c(130, 64, (4, 4), True, mask="left", arg=5),
    _c(33, 128, (8, 2), True, extra=7),                 # table longer than S
    _c(257, 64, (4, 4), False, extra=1),
]


def _id(c):
    return case_id(c) + (f"-table+{c['extra']}" if c["extra"] else "")


def _tables(S, D, extra):
    from deepspeed_amd.ops.functional import build_rope_cache
    return build_rope_cache(S + extra, D, device=DEV)


def _maxerr(got, ref):
    return (got.double() - ref).abs().max().item()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_unrotate_not_worse_than_two_kernels(case):
    from deepspeed_amd.ops.functional import _rope_torch
    ext = get_ext(required=True)
    S, D = case["S"], case["D"]
    scale = case_scale(case)
    # q, k play the rotated tensors: that is what the kernels are given
    q, k, v, dout, mask = make_inputs(case, device=DEV)
    cos, sin = _tables(S, D, case["extra"])
    out, lse = ext.flash_attn_fwd(q, k, v, case["causal"], scale, mask)

    # (a) fused
    dq_a, dk_a, dv_a = ext.flash_attn_bwd(q, k, v, dout, out, lse,
                                          case["causal"], scale, mask,
                                          cos, sin)
    # (b) two kernels
    dq_n, dk_n, dv_b = ext.flash_attn_bwd(q, k, v, dout, out, lse,
                                          case["causal"], scale, mask)
    dq_b, dk_b = torch.empty_like(dq_n), torch.empty_like(dk_n)
    ext.rope(dq_b, dq_n, cos, sin, 0, True)
    ext.rope(dk_b, dk_n, cos, sin, 0, True)
    # (c) reference
    r = attention_ref(q, k, v, case["causal"], scale, mask, dout)
    dq_c = _rope_torch(r["dq"], cos, sin, -1.0).double()
    dk_c = _rope_torch(r["dk"], cos, sin, -1.0).double()

    assert torch.equal(dv_a.view(torch.int16), dv_b.view(torch.int16)), "dv"
    for name, a, b, c in (("dq", dq_a, dq_b, dq_c), ("dk", dk_a, dk_b, dk_c)):
        assert not torch.isnan(a.float()).any(), f"{name}: NaN"
        ea, eb = _maxerr(a, c), _maxerr(b, c)
        ulp = 2.0 ** -8 * c.abs().max().item()
        print(f"{_id(case)} {name}: fused err {ea:.4e} two-kernel err "
              f"{eb:.4e} ulp at max {ulp:.4e}")
        assert ea <= eb + ulp, \
            f"{name}: fused {ea:.4e} > two-kernel {eb:.4e} + ulp {ulp:.4e}"


def test_table_contract():
    ext = get_ext(required=True)
    case = _c(33, 64, (4, 4), True)
    q, k, v, dout, _ = make_inputs(case, device=DEV)
    scale = case_scale(case)
    out, lse = ext.flash_attn_fwd(q, k, v, True, scale, None)
    cos, sin = _tables(33, 64, 0)

    def call(c, s):
        return ext.flash_attn_bwd(q, k, v, dout, out, lse, True, scale, None,
                                  c, s)

    call(cos, sin)                                   # exactly fits
    for bad in ((cos[:32], sin[:32]),                # shorter than S
                (cos.cpu(), sin.cpu()),              # host table
                (cos.bfloat16(), sin.bfloat16()),    # not fp32
                (cos.t(), sin.t()),                  # not contiguous
                (cos, None)):                        # only one of the two
        with pytest.raises(RuntimeError):
            call(*bad)
