"""Inverse RoPE fused into the flash backward epilogues (needs MI355X): the
ROPE = true instantiations of flash_bwd_dkv_kernel / flash_bwd_dq_kernel.

With cos/sin tables `flash_attn_bwd` takes the rotated q and k that forward
attended over and returns dq, dk with respect to the un-rotated tensors.
Three routes are compared per case:
  (a) the fused call;
  (b) the unfused route: flash_attn_bwd without tables, then
      rope(..., backward=True) on dq and dk;
  (c) the closed-form float64 reference of attn_refs.attention_ref,
      un-rotated in float64 by attn_refs.unrotate_ref.
Asserted on every case:
  * (a) lies ELEMENTWISE within the bound attn_refs.py derives for (c);
    test_flash_bwd_rope_refs_cpu.py shows on the same cases that this bound
    admits a faithful emulation and rejects a wrong sign, table row or table
    column and a skipped un-rotation;
  * (a) rounds to bf16 once where (b) rounds twice, so its max abs error
    against (c) may not exceed (b)'s by more than one bf16 ulp at max|c|
    (2^-8 * max|c|: a different element may land on the maximum);
  * dv does not see the tables and is bit-identical to the no-table call;
  * a second fused call returns the same bits; no NaN comes out although
    every table row from S on is NaN.
The shared ATTN_CASES / TILE_CASES run on random-angle tables (every entry
distinct and of order 1); CASES keeps real build_rope_cache tables, whose
upper columns are close to the identity at these S.
"""
import itertools

import pytest
import torch

from attn_bwd_tile_cases import TILE_CASES, make_tile_inputs
from attn_refs import (ATTN_CASES, attention_ref, case_id, case_scale,
                       make_inputs, make_rope_tables, unrotated_grads)
from edge_refs import assert_within

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
EXTRA = 3     # NaN rows past S in the random-angle tables


def _c(S, D, H, causal, mask=None, arg=None, extra=0):
    return dict(S=S, D=D, Hq=H[0], Hk=H[1], causal=causal, custom=False,
                mask=mask, arg=arg, extra=extra)


# real RoPE tables. S: 1, the padded tail of one 128-row block (33), two
# blocks (130, 257)
CASES = [_c(S, D, H, causal)
         for D, S, H, causal in itertools.product(
             (64, 128), (1, 33, 130, 257), ((4, 4), (8, 2)), (True, False))]
CASES += [
    _c(130, 128, (8, 2), False, mask="tail", arg=97),   # kv padding mask
    _c(130, 64, (4, 4), True, mask="left", arg=5),
    _c(33, 128, (8, 2), True, extra=7),                 # table longer than S
    _c(257, 64, (4, 4), False, extra=1),
]

# the shared cases of the no-table tests, each with its own input maker
SHARED = [(c, make_inputs) for c in ATTN_CASES] + \
    [(c, make_tile_inputs) for c in TILE_CASES]
SHARED_IDS = [("tile-" if mk is make_tile_inputs else "") + case_id(c)
              for c, mk in SHARED]


def _id(c):
    return case_id(c) + (f"-table+{c['extra']}" if c["extra"] else "")


def _tables(S, D, extra):
    from deepspeed_amd.ops.functional import build_rope_cache
    return build_rope_cache(S + extra, D, device=DEV)


def _maxerr(got, ref):
    return (got.double() - ref).abs().max().item()


def _bits(t):
    return t.view(torch.int16)


def _check_routes(case, inputs, cos, sin, what):
    """Routes (a), (b), (c) on one case and every assertion of the module
    docstring. q, k play the rotated tensors: that is what the kernels are
    given."""
    ext = get_ext(required=True)
    q, k, v, dout, mask = inputs
    scale = case_scale(case)
    causal = case["causal"]
    out, lse = ext.flash_attn_fwd(q, k, v, causal, scale, mask)

    # (a) fused, twice
    dq_a, dk_a, dv_a = ext.flash_attn_bwd(q, k, v, dout, out, lse, causal,
                                          scale, mask, cos, sin)
    dq_2, dk_2, dv_2 = ext.flash_attn_bwd(q, k, v, dout, out, lse, causal,
                                          scale, mask, cos, sin)
    # (b) two kernels
    dq_n, dk_n, dv_b = ext.flash_attn_bwd(q, k, v, dout, out, lse, causal,
                                          scale, mask)
    dq_b, dk_b = torch.empty_like(dq_n), torch.empty_like(dk_n)
    ext.rope(dq_b, dq_n, cos, sin, 0, True)
    ext.rope(dk_b, dk_n, cos, sin, 0, True)
    # (c) reference
    r = attention_ref(q, k, v, causal, scale, mask, dout)
    un = unrotated_grads(r, cos, sin)

    assert torch.equal(_bits(dv_a), _bits(dv_b)), "dv"
    for name, a, a2 in (("dq", dq_a, dq_2), ("dk", dk_a, dk_2),
                        ("dv", dv_a, dv_2)):
        assert torch.equal(_bits(a), _bits(a2)), f"{name}: not deterministic"
    for name, a, b in (("dq", dq_a, dq_b), ("dk", dk_a, dk_b)):
        c, tol = un[name], un[name + "_tol"]
        assert not torch.isnan(c).any()
        assert not torch.isnan(a.float()).any(), f"{name}: NaN"
        ea, eb = _maxerr(a, c), _maxerr(b, c)
        ulp = 2.0 ** -8 * c.abs().max().item()
        share = ((a.double() - c).abs() / tol.clamp_min(1e-300)).max().item()
        print(f"{what} {name}: fused err {ea:.4e} two-kernel err {eb:.4e} "
              f"ulp at max {ulp:.4e}; fused peaks at {share:.3f} of the "
              f"elementwise bound")
        assert_within(a, c, tol, f"{what} {name}")
        assert ea <= eb + ulp, \
            f"{name}: fused {ea:.4e} > two-kernel {eb:.4e} + ulp {ulp:.4e}"


@pytest.mark.parametrize("i", range(len(SHARED)), ids=SHARED_IDS)
def test_fused_unrotate_vs_float64_on_shared_cases(i):
    case, mk = SHARED[i]
    cos, sin = make_rope_tables(case["S"], case["D"], EXTRA, device=DEV)
    assert cos.shape[0] == case["S"] + EXTRA and torch.isnan(cos[-1]).all()
    _check_routes(case, mk(case, DEV), cos, sin, SHARED_IDS[i])


@pytest.mark.parametrize("i", [SHARED_IDS.index(n) for n in (
    "tile-S385-D64-H4x4-causal-left129", "tile-S383-D128-H6x2-causal")])
def test_table_of_exactly_S_rows(i):
    case, mk = SHARED[i]
    cos, sin = make_rope_tables(case["S"], case["D"], 0, device=DEV)
    assert cos.shape[0] == case["S"]
    _check_routes(case, mk(case, DEV), cos, sin, SHARED_IDS[i] + " exact")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_unrotate_not_worse_than_two_kernels(case):
    cos, sin = _tables(case["S"], case["D"], case["extra"])
    _check_routes(case, make_inputs(case, device=DEV), cos, sin, _id(case))


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
