"""Flash backward pass 1 with workgroups of BRK = 64 keys (4 waves x 16),
several resident per CU, launched as a 1-D grid whose workgroup id is mapped
to (key block, b * Hk + kv head) by flash_bwd_wgmap.h (needs MI355X).

Comparison and bounds as in test_flash_bwd_oneimage_gpu.py: elementwise
against the float64 reference of attn_refs.py, inputs with the +-64 sentinels
of make_tile_inputs, check_attention's bounds. What the cases straddle:
  * the key block: S = BRK - 1, BRK, BRK + 1, 2 BRK + 1, and 127, 128, 129,
    because the row constants stay padded to 128 while a workgroup is 64
    keys: a last workgroup with one key, one with every wave but one past
    S - 1, and a second workgroup inside one 128-row pad;
  * the map's two parts: heads (4, 4) at the tests' B = 2 give B * Hk = 8, one
    complete round of 8; (6, 2) gives 4, the ragged tail; B 1 with heads
    (2, 1) and S = 3 BRK + 1 gives 4 workgroups in all, not a multiple of 8;
  * a kv mask and the ROPE instantiation per head dim, S across a key block;
  * the loader: at D 128 an image has 8 segments and the workgroup 4 waves,
    so a wave issues two segments into each ring buffer: two steps (S 33) and
    one step with 31 clamped rows (S 31). D 64 (4 segments) runs them too;
  * no scratch besides the row constants: the same bits from two calls, and
    from a call right after a larger one.
"""
import pytest
import torch

from attn_bwd_tile_cases import make_tile_inputs
from attn_refs import (_c, attention_ref, case_id, case_scale,
                       check_attention, make_inputs, make_rope_tables)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BRK = 64      # keys per pass 1 workgroup (bwd::BRK1 of attention_bwd.hip)

BLOCK_CASES = [_c(S, D, H, causal)
               for D in (128, 64)
               for S in (BRK - 1, BRK, BRK + 1, 2 * BRK + 1, 127, 128)
               for H in ((6, 2), (4, 4))
               for causal in (True, False)]
assert 2 * BRK + 1 == 129   # the list above holds 127, 128, 129 once each
MASK_CASES = [_c(2 * BRK + 1, D, (6, 2), True, mask="tail", arg=BRK + 1)
              for D in (128, 64)]
ROPE_CASES = [_c(161, D, (6, 2), True) for D in (128, 64)]
LOADER_CASES = [_c(S, D, (4, 4), causal)
                for D in (128, 64) for S in (33, 31)
                for causal in (True, False)]


def test_brk_is_the_kernels():
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                            "deepspeed_amd", "ops", "csrc",
                            "attention_bwd.hip")).read()
    assert "constexpr int KTW1 = 1;" in src
    assert "constexpr int NW1 = 4;" in src
    assert "constexpr int BRK1 = 16 * KTW1 * NW1;" in src


def _fwd_bwd(c, inputs):
    q, k, v, do, mask = inputs
    scale = case_scale(c)
    e = get_ext(required=True)
    out, lse = e.flash_attn_fwd(q, k, v, c["causal"], scale, mask)
    dq, dk, dv = e.flash_attn_bwd(q, k, v, do, out, lse, c["causal"], scale,
                                  mask)
    return out, lse, dq, dk, dv


def _check(c, inputs=None, what=None):
    inputs = make_tile_inputs(c, DEV) if inputs is None else inputs
    q, k, v, do, mask = inputs
    ref = attention_ref(q, k, v, c["causal"], case_scale(c), mask, do)
    out, lse, dq, dk, dv = _fwd_bwd(c, inputs)
    check_attention(dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), ref,
                    what or case_id(c))


@pytest.mark.parametrize("c", BLOCK_CASES, ids=case_id)
def test_lengths_around_the_key_block(c):
    _check(c)


@pytest.mark.parametrize("c", MASK_CASES, ids=case_id)
def test_kv_mask_ending_inside_the_second_key_block(c):
    _check(c)


@pytest.mark.parametrize("c", ROPE_CASES, ids=case_id)
def test_rope_instantiations(c):
    from test_flash_bwd_rope_gpu import _check_routes
    cos, sin = make_rope_tables(c["S"], c["D"], 3, device=DEV)
    _check_routes(c, make_tile_inputs(c, DEV), cos, sin, case_id(c))


@pytest.mark.parametrize("c", LOADER_CASES, ids=case_id)
def test_a_wave_issues_two_segments_per_image(c):
    _check(c)


@pytest.mark.parametrize("D", (128, 64))
@pytest.mark.parametrize("causal", (True, False))
def test_ragged_map_tail_one_batch_one_kv_head(D, causal):
    c = _c(3 * BRK + 1, D, (2, 1), causal)
    inputs = tuple(None if t is None else t[:1].contiguous()
                   for t in make_tile_inputs(c, DEV))
    assert inputs[1].shape[0] * inputs[1].shape[2] == 1   # B * Hk
    assert -(-c["S"] // BRK) % 8 == 4                     # workgroups
    _check(c, inputs, case_id(c) + "-B1")


@pytest.mark.parametrize("D", (128, 64))
def test_same_bits_twice_and_after_a_large_call(D):
    small = _c(2 * BRK + 1, D, (6, 2), True)
    large = _c(513, D, (6, 2), True)
    s_in = make_tile_inputs(small, DEV)
    alone = _fwd_bwd(small, s_in)
    again = _fwd_bwd(small, s_in)
    for x, y in zip(alone[2:], again[2:]):
        assert torch.equal(x, y)
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
