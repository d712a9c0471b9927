"""The cases of test_attention_bwd_tiles_gpu.py have teeth: on each of them
the float64 reference itself, with one tile-boundary key dropped, or with
one tile-boundary q row dropped from dK / dV, falls outside the bounds that
attn_refs.py derives. Runs without a GPU."""
import pytest
import torch

from attn_bwd_tile_cases import (TILE_CASES, boundary_key, boundary_row,
                                 make_tile_inputs)
from attn_refs import attention_ref, case_id, case_scale
from edge_refs import assert_within


def _check_bwd(got, ref, what):
    for name in ("dq", "dk", "dv"):
        assert_within(got[name], ref[name], ref[name + "_tol"],
                      f"{what} {name}")


@pytest.mark.parametrize("c", TILE_CASES, ids=case_id)
def test_dropped_boundary_key_or_row_is_outside_the_bounds(c):
    q, k, v, do, mask = make_tile_inputs(c)
    scale = case_scale(c)
    ref = attention_ref(q, k, v, c["causal"], scale, mask, do)
    assert not torch.isnan(ref["lse"]).any()
    _check_bwd(ref, ref, "reference against itself")

    # one boundary key dropped from every sum
    j = boundary_key(c, mask)
    B, S = q.shape[0], q.shape[1]
    m2 = torch.zeros(B, S) if mask is None else mask.clone()
    m2[:, j] = float("-inf")
    no_key = attention_ref(q, k, v, c["causal"], scale, m2, do)
    with pytest.raises(AssertionError):
        _check_bwd(no_key, ref, f"key {j} dropped")

    # one boundary q row dropped from dK / dV: dS and P^T dO are linear in
    # dO, so a zero dO row removes exactly that row's terms
    i = boundary_row(c)
    do2 = do.clone()
    do2[:, i] = 0
    no_row = attention_ref(q, k, v, c["causal"], scale, mask, do2)
    for name in ("dk", "dv"):
        with pytest.raises(AssertionError):
            assert_within(no_row[name], ref[name], ref[name + "_tol"],
                          f"q row {i} dropped from {name}")
