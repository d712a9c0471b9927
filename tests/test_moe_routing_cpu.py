"""MoE routing functionals on the CPU: the torch fallbacks against the float64
references, the GPU cases' tie-free inputs, and `fused_routing=True` giving
the unfused layer's result where no kernel runs."""
import copy

import pytest
import torch

from edge_refs import BF16_ULP, assert_within
from moe_routing_refs import (assert_gaps, gate_ref, make_logits, rows_ref,
                              rows_tol, routing_on)
from test_moe_routing_gpu import GATE_CASES, capacities, tokens_of

from deepspeed_amd.ops import functional as Fops


@pytest.mark.parametrize("kind,E,k", GATE_CASES)
def test_gate_inputs_have_no_near_ties(kind, E, k):
    S = tokens_of(kind, E)
    assert_gaps(gate_ref(make_logits(S, E, seed=S + E + k), k, S, True))


@pytest.mark.parametrize("S,E,k", [(5, 4, 1), (257, 6, 2), (130, 64, 4)])
def test_gate_fallback_matches_reference(S, E, k):
    logits = make_logits(S, E, seed=S + E + k)
    for C, drop in capacities(S, E, k):
        r = gate_ref(logits, k, C, drop)
        l_aux, idx, w, loc, keep, counts, slot = Fops.moe_gate_topk(
            logits, k, C, drop)
        for got, name in ((idx, "idx"), (loc, "loc"), (keep, "keep"),
                          (counts, "counts"), (slot, "slot_token")):
            assert torch.equal(got.long(), r[name].long()), name
        assert_within(w, r["weights"], r["w_tol"], "weights")
        assert_within(l_aux, r["l_aux"], r["l_aux_tol"], "l_aux")


def test_gate_no_tokens():
    out = Fops.moe_gate_topk(torch.zeros(0, 4), 2, 4)
    assert out[0].item() == 0 and out[1].shape == (0, 2)
    assert (out[6] == -1).all() and out[6].numel() == 16


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dispatch_combine_fallback(dtype):
    S, E, k, M = 130, 8, 4, 24
    r = gate_ref(make_logits(S, E, seed=3), k, 40, True)
    assert not r["keep"].all()
    C = r["capacity"]
    idx, loc, keep, slot = routing_on(r, "cpu")
    torch.manual_seed(0)
    x = torch.randn(S, M).to(dtype)
    eo = torch.randn(E * C, M).to(dtype)
    ref = rows_ref(r, x, eo, x, eo)
    out = torch.full((E, C, M), float("nan"), dtype=dtype)
    d = Fops.moe_dispatch(x, idx, loc, keep, slot, E, C, out=out)
    assert d.data_ptr() == out.data_ptr()
    assert torch.equal(d.reshape(E * C, M).double(), ref["disp"])
    y = Fops.moe_combine(eo.view(E, C, M), idx, loc, keep,
                         r["weights"].float())
    # the fallback rounds the weights, then each product, to the activation
    # dtype: two more bf16 roundings per term
    tol = rows_tol(ref["comb"], ref["comb_abs"], k, dtype)
    if dtype == torch.bfloat16:
        tol = tol + 2 * BF16_ULP * ref["comb_abs"]
    assert_within(y, ref["comb"], tol, "combine")


def test_layer_flag_on_cpu_is_the_unfused_layer():
    from deepspeed_amd.moe.layer import MoE
    torch.manual_seed(0)
    M = 24
    moe = MoE(M, torch.nn.Linear(M, M), num_experts=4, k=2,
              capacity_factor=0.75)
    fused = copy.deepcopy(moe)
    fused.deepspeed_moe.fused_routing = True
    x = torch.randn(2, 33, M)
    grads = []
    for m in (moe, fused):
        xi = x.clone().requires_grad_(True)
        out, l_aux, counts = m(xi)
        (out.square().sum() + l_aux).backward()
        grads.append((out, l_aux, counts, xi.grad,
                      m.deepspeed_moe.gate.wg.weight.grad))
    for a, b in zip(*grads):
        assert torch.allclose(a.double(), b.double(), rtol=1e-6, atol=1e-7)
