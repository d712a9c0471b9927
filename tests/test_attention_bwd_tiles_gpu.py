"""Flash attention backward at the edges of ITS tiles (needs MI355X): 128-row
workgroups, 32-row waves and steps, the 128-padded transposed scratch.

Comparison and bounds as in test_attention_edges_gpu.py: elementwise against
the float64 reference of attn_refs.py. test_attention_bwd_tiles_cpu.py shows
that those bounds reject one dropped boundary key or q row on these cases.
"""
import pytest
import torch

from attn_bwd_tile_cases import TILE_CASES, make_tile_inputs
from attn_refs import (attention_ref, case_id, case_scale, check_attention,
                       make_inputs)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"


def _ext():
    return get_ext(required=True)


def _fwd_bwd(c, inputs):
    q, k, v, do, mask = inputs
    scale = case_scale(c)
    e = _ext()
    out, lse = e.flash_attn_fwd(q, k, v, c["causal"], scale, mask)
    dq, dk, dv = e.flash_attn_bwd(q, k, v, do, out, lse, c["causal"], scale,
                                  mask)
    return out, lse, dq, dk, dv


@pytest.mark.parametrize("c", TILE_CASES, ids=case_id)
def test_flash_bwd_tile_edges_vs_float64(c):
    inputs = make_tile_inputs(c, DEV)
    q, k, v, do, mask = inputs
    ref = attention_ref(q, k, v, c["causal"], case_scale(c), mask, do)
    out, lse, dq, dk, dv = _fwd_bwd(c, inputs)
    check_attention(dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), ref,
                    case_id(c))


def test_flash_bwd_is_deterministic():
    c = dict(S=385, D=128, Hq=6, Hk=2, causal=True, custom=False, mask=None)
    inputs = make_tile_inputs(c, DEV)
    a = _fwd_bwd(c, inputs)
    b = _fwd_bwd(c, inputs)
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)


def test_small_call_does_not_see_a_large_calls_scratch():
    """The padded tail of the transposed scratch is rewritten by every call:
    a short call gives the same bits alone and right after a long one whose
    scratch the allocator hands back."""
    small = dict(S=129, D=128, Hq=6, Hk=2, causal=True, custom=False,
                 mask=None)
    large = dict(S=513, D=128, Hq=6, Hk=2, causal=True, custom=False,
                 mask=None)
    s_in = make_tile_inputs(small, DEV)
    alone = _fwd_bwd(small, s_in)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    l_in = make_inputs(large, DEV)
    # NaN-free but huge values everywhere a stale read could land
    big = _fwd_bwd(large, tuple(t if i == 4 or t is None else t * 64
                                for i, t in enumerate(l_in)))
    del big
    after = _fwd_bwd(small, s_in)
    for x, y in zip(alone[2:], after[2:]):
        assert torch.equal(x, y)
