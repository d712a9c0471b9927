"""MoE routing kernels (needs MI355X): the HIP gate, dispatch and combine and
their backward kernels against the float64 references of
`moe_routing_refs.py` (bounds derived there), and `MOELayer` with
`fused_routing=True` against the unfused layer.

Layer errors measured on an MI355X (max |got - ref| / max |ref| against the
float64 CPU layer, unfused / fused): see profiles/README.md, "MoE routing"."""
import copy
import functools

import pytest
import torch

from edge_refs import U24, assert_within
from moe_routing_refs import (assert_gaps, gate_grad_ref, gate_ref,
                              make_logits, rows_ref, rows_tol, routing_on)

from deepspeed_amd.ops import functional as Fops

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32

# S: 1, 5, one token either side of the rank kernel's block, 4 blocks + tail
GATE_CASES = [(kind, E, k)
              for kind in ("one", "five", "block-1", "block", "block+1",
                           "blocks")
              for E in (4, 6, 8, 64, 160) for k in (1, 2, 4)]


def tokens_of(kind, E):
    tb = Fops.moe_gate_block_tokens(E)
    return {"one": 1, "five": 5, "block-1": tb - 1, "block": tb,
            "block+1": tb + 1, "blocks": 4 * tb + 7}[kind]


def capacities(S, E, k):
    """(capacity, drop_tokens): queue 0 overflows / nothing drops / no-drop."""
    return [(max(1, S * k // (2 * E)), True), (S, True), (4, False)]


@pytest.mark.parametrize("kind,E,k", GATE_CASES)
def test_gate_forward_and_backward(kind, E, k):
    S = tokens_of(kind, E)
    assert get_ext(required=True).moe_gate_block_tokens(E) == \
        Fops.moe_gate_block_tokens(E)
    logits = make_logits(S, E, seed=S + E + k)
    torch.manual_seed(S)
    dw = torch.randn(S, k)
    for n, (C, drop) in enumerate(capacities(S, E, k)):
        r = gate_ref(logits, k, C, drop)
        assert_gaps(r)
        if n == 0 and S > 5 and k < E:      # one queue overflows, another
                                            # stays short
            assert not r["keep"].all() and (r["counts"] < C).any()
        lg = logits.to(DEV).requires_grad_(True)
        l_aux, idx, w, loc, keep, counts, slot = Fops.moe_gate_topk(
            lg, k, C, drop)
        what = f"S={S} E={E} k={k} C={C} drop={drop}"
        for got, name in ((idx, "idx"), (loc, "loc"), (keep, "keep"),
                          (counts, "counts"), (slot, "slot_token")):
            assert torch.equal(got.long().cpu(), r[name].long()), \
                f"{name} {what}"
        assert_within(w, r["weights"], r["w_tol"], f"weights {what}")
        assert_within(l_aux, r["l_aux"], r["l_aux_tol"], f"l_aux {what}")
        ((w * dw.to(DEV)).sum() + 0.7 * l_aux).backward()
        ref, tol = gate_grad_ref(r, dw, 0.7)
        assert_within(lg.grad, ref, tol, f"dlogits {what}")


def test_gate_ties_go_to_the_lower_index():
    logits = torch.tensor([[1., 3., 3., 0., 3., 2.],
                           [2., 2., 2., 2., 2., 2.],
                           [0., 1., 5., 5., 1., 0.]])
    for k, want in ((2, [[1, 2], [0, 1], [2, 3]]),
                    (4, [[1, 2, 4, 5], [0, 1, 2, 3], [2, 3, 1, 4]])):
        r = gate_ref(logits, k, 3, True)
        assert r["idx"].tolist() == want
        out = Fops.moe_gate_topk(logits.to(DEV), k, 3, True)
        assert out[1].tolist() == want
        assert torch.equal(out[3].long().cpu(), r["loc"])


@functools.lru_cache(None)
def route(k):
    """Routing with drops from the gate reference, weights as fp32 values."""
    S, E = (257, 6) if k == 2 else (130, 8)
    r = gate_ref(make_logits(S, E, seed=k), k, 40, True)
    assert not r["keep"].all() and (r["slot_token"] < 0).any()
    r["weights"] = r["weights"].float().double()
    return r


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("dtype,M", [(BF, 8), (BF, 136), (BF, 1024),
                                     (F32, 4), (F32, 68)])
def test_dispatch_combine_and_their_backward(dtype, M, k):
    r = route(k)
    S, E, C = r["idx"].shape[0], r["counts"].numel(), r["capacity"]
    idx, loc, keep, slot = routing_on(r, DEV)
    torch.manual_seed(M + k)
    x, dout = (torch.randn(S, M, device=DEV).to(dtype) for _ in range(2))
    eo, dd = (torch.randn(E * C, M, device=DEV).to(dtype) for _ in range(2))
    ref = rows_ref(r, x, eo, dout, dd)
    x.requires_grad_(True)
    eo.requires_grad_(True)
    w = r["weights"].float().to(DEV).requires_grad_(True)
    empty = (r["slot_token"] < 0).to(DEV)

    out = torch.full((E, C, M), float("nan"), device=DEV, dtype=dtype)
    d = Fops.moe_dispatch(x, idx, loc, keep, slot, E, C, out=out)
    assert d.data_ptr() == out.data_ptr()
    assert torch.equal(d.detach().reshape(E * C, M).double().cpu(),
                       ref["disp"])                 # bit-exact, zeros too
    d.backward(dd.view(E, C, M))
    assert_within(x.grad, ref["dx"],
                  rows_tol(ref["dx"], ref["dx_abs"], k, dtype), "dispatch dx")

    y = Fops.moe_combine(eo.view(E, C, M), idx, loc, keep, w,
                         slot_token=slot)
    assert_within(y, ref["comb"],
                  rows_tol(ref["comb"], ref["comb_abs"], k, dtype), "combine")
    y.backward(dout)
    assert_within(eo.grad, ref["d_expert"],
                  rows_tol(ref["d_expert"], ref["d_expert"].abs(), 1, dtype),
                  "combine d_expert_out")
    assert (eo.grad[empty] == 0).all()
    assert_within(w.grad, ref["dw"], M * U24 * ref["dw_abs"], "combine dw")
    assert (w.grad[~keep] == 0).all()


def test_misaligned_rows_take_the_fallback():
    r = route(2)
    S, E, C, M = r["idx"].shape[0], r["counts"].numel(), r["capacity"], 136
    idx, loc, keep, slot = routing_on(r, DEV)
    torch.manual_seed(0)
    x = torch.randn(S * M + 8, device=DEV).to(BF)[1:1 + S * M].view(S, M)
    eo = torch.randn(E * C * M + 8, device=DEV).to(BF)[1:1 + E * C * M]
    assert x.data_ptr() % 16 and not Fops._moe_rows_ok(x)
    with pytest.raises(RuntimeError, match="16-byte"):
        get_ext(required=True).moe_scatter_rows(
            torch.empty(E * C, M, device=DEV, dtype=BF), x, slot, None, 2)
    ref = rows_ref(r, x, eo.view(E * C, M), x, eo.view(E * C, M))
    d = Fops.moe_dispatch(x, idx, loc, keep, slot, E, C)
    assert torch.equal(d.reshape(E * C, M).double().cpu(), ref["disp"])
    y = Fops.moe_combine(eo.view(E, C, M), idx, loc, keep,
                         r["weights"].float().to(DEV))
    # the fallback rounds weights and products to bf16: two ulps per term
    assert_within(y, ref["comb"], rows_tol(ref["comb"], ref["comb_abs"], 2,
                                           BF) + 2.0 ** -6 * ref["comb_abs"],
                  "fallback combine")


def test_layer_fused_routing_against_unfused():
    """fp32 MOELayer, E 4, k 2, M 136, 2 x 129 tokens, dropping: identical
    routing, and the fused path's error against the float64 CPU layer at most
    twice the unfused GPU path's (floor 1e-6): both are fp32 paths that
    differ in summation order only."""
    from deepspeed_amd.moe.layer import MoE
    torch.manual_seed(0)
    M = 136
    moe = MoE(M, torch.nn.Linear(M, M), num_experts=4, k=2,
              capacity_factor=0.75)
    x = torch.randn(2, 129, M)
    dy = torch.randn(2, 129, M)

    def run(m, device, dtype):
        m = copy.deepcopy(m).to(device=device, dtype=dtype)
        xi = x.to(device=device, dtype=dtype).requires_grad_(True)
        out, l_aux, counts = m(xi)
        ((out * dy.to(out)).sum() + l_aux).backward()
        grads = [p.grad for p in m.parameters()]
        return [out, xi.grad] + grads, counts

    ref, ref_counts = run(moe, "cpu", torch.float64)
    plain, plain_counts = run(moe, DEV, F32)
    moe.deepspeed_moe.fused_routing = True
    fused, fused_counts = run(moe, DEV, F32)
    assert torch.equal(fused_counts, plain_counts)
    assert torch.equal(plain_counts.cpu(), ref_counts)
    assert 0 < int(ref_counts.sum()) < 2 * 258      # some choices dropped
    for i, (rf, pl, fu) in enumerate(zip(ref, plain, fused)):
        scale = rf.abs().max()
        e_plain = ((pl.double().cpu() - rf).abs().max() / scale).item()
        e_fused = ((fu.double().cpu() - rf).abs().max() / scale).item()
        print(f"layer tensor {i}: unfused {e_plain:.3e} fused {e_fused:.3e}")
        assert e_fused <= max(2 * e_plain, 1e-6), (i, e_plain, e_fused)
