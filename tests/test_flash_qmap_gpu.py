"""The two q-outer flash kernels, flash_fwd_v6_kernel (256 q rows per
workgroup) and the backward's pass 2, flash_bwd_dq_kernel (128), launched as
1-D grids whose workgroup id is mapped to (q block, b * Hq + q head) by
bwd_wgmap::q_index of flash_bwd_wgmap.h (needs MI355X).

Comparison and bounds as in test_flash_bwd_pass1_wg_gpu.py: elementwise
against the float64 reference of attn_refs.py, inputs with the +-64 sentinels
of make_tile_inputs, check_attention's bounds. A wrong (q block, bh) leaves
rows of out / lse / dq unwritten or writes another head's. What the cases
straddle:
  * the q block: S = 255, 256, 257 and 513 (1, 1, 2 and 3 forward blocks) and
    127, 128, 129 (1, 1 and 2 pass 2 blocks);
  * the map's two parts, at the tests' B = 2: heads (4, 4) give B * Hq = 8,
    one complete round of 8; (6, 2) gives 12, a round plus a ragged tail of 4;
    (8, 2) gives two rounds, with the q heads of one kv head on different
    residues; B 1 with heads (2, 1) is a tail only;
  * D 128 and 64, causal and not (the map serves both);
  * a kv mask ending inside the second q block of each kernel, and the ROPE
    instantiation of pass 2 per head dim;
  * the forward's causal diagonal at wave granularity (a wave skips a 64-key
    tile that lies wholly above its 32 rows): S = 256 + 33, 256 + 64 and
    256 + 65, where some waves of a block skip and some do not, and a
    left-padding mask under which whole q rows have no admissible column
    (out 0, lse -inf);
  * no state between calls: the same bits from two calls, and from a call right
    after a larger one.
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
QT = 256      # q rows per forward workgroup (QT5 of attention.hip)
BR = 128      # q rows per pass 2 workgroup (bwd::BR of attention_bwd.hip)

BLOCK_CASES = [_c(S, D, H, causal)
               for D in (128, 64)
               for S in (QT - 1, QT, QT + 1, 2 * QT + 1, BR - 1, BR, BR + 1)
               for H in ((4, 4), (6, 2), (8, 2))
               for causal in (True, False)]
MASK_CASES = [_c(S, D, (6, 2), True, mask="tail", arg=arg)
              for D in (128, 64)
              for S, arg in ((2 * QT + 1, QT + 44), (2 * BR + 1, BR + 32))]
ROPE_CASES = [_c(2 * BR + 1, D, (8, 2), True) for D in (128, 64)]
# In the first forward block waves 0 .. 5 skip key tiles and waves 6, 7 skip
# none. The second block has one key tile of its own at 33 and 64 more rows,
# which waves 0 and 1 both need (the edge of the skip condition: nothing is
# skipped), and two at 65, where waves 0 and 1 skip the last and wave 2 does
# not.
SKIP_CASES = [_c(QT + n, D, (6, 2), True) for D in (128, 64)
              for n in (33, 64, 65)]


def test_block_sizes_are_the_kernels():
    import os
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "deepspeed_amd", "ops", "csrc")
    assert "constexpr int QT5 = 256;" in \
        open(os.path.join(csrc, "attention.hip")).read()
    assert "constexpr int BR = 128;" in \
        open(os.path.join(csrc, "attention_bwd.hip")).read()


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
def test_lengths_around_the_q_blocks(c):
    _check(c)


@pytest.mark.parametrize("c", MASK_CASES, ids=case_id)
def test_kv_mask_ending_inside_the_second_q_block(c):
    _check(c)


@pytest.mark.parametrize("c", ROPE_CASES, ids=case_id)
def test_rope_instantiations(c):
    from test_flash_bwd_rope_gpu import _check_routes
    cos, sin = make_rope_tables(c["S"], c["D"], 3, device=DEV)
    _check_routes(c, make_tile_inputs(c, DEV), cos, sin, case_id(c))


@pytest.mark.parametrize("c", SKIP_CASES, ids=case_id)
def test_some_waves_skip_a_tile_and_some_do_not(c):
    _check(c)


@pytest.mark.parametrize("D", (128, 64))
def test_rows_without_admissible_columns_under_the_wave_skip(D):
    """Left padding past the first block: rows 0 .. 259 have no admissible
    column in batch row 0 (out 0, lse -inf, as before the skip), and the waves
    of the first block skip tiles while their running max is still -inf."""
    c = _c(QT + 33, D, (6, 2), True, mask="left", arg=QT + 4)
    inputs = make_tile_inputs(c, DEV)
    _check(c, inputs)
    out, lse = _fwd_bwd(c, inputs)[:2]
    assert (out[0, :QT + 4] == 0).all()
    assert (lse[0, :, :QT + 4] == float("-inf")).all()
    assert torch.isfinite(lse[0, :, QT + 4:]).all()
    assert torch.isfinite(lse[1]).all()


@pytest.mark.parametrize("D", (128, 64))
@pytest.mark.parametrize("causal", (True, False))
def test_ragged_map_tail_one_batch_two_q_heads(D, causal):
    c = _c(2 * QT + 1, D, (2, 1), causal)
    inputs = tuple(None if t is None else t[:1].contiguous()
                   for t in make_tile_inputs(c, DEV))
    assert inputs[0].shape[0] * inputs[0].shape[2] == 2   # B * Hq
    _check(c, inputs, case_id(c) + "-B1")


@pytest.mark.parametrize("D", (128, 64))
def test_same_bits_twice_and_after_a_large_call(D):
    small = _c(QT + 1, D, (6, 2), True)
    large = _c(3 * QT + 1, D, (8, 2), True)
    s_in = make_tile_inputs(small, DEV)
    alone = _fwd_bwd(small, s_in)
    again = _fwd_bwd(small, s_in)
    for x, y in zip(alone, again):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    l_in = make_inputs(large, DEV)
    # NaN-free but huge values everywhere a stale read could land
    big = _fwd_bwd(large, tuple(t if i == 4 or t is None else t * 64
                                for i, t in enumerate(l_in)))
    del big
    after = _fwd_bwd(small, s_in)
    for x, y in zip(alone, after):
        assert torch.equal(x, y)
