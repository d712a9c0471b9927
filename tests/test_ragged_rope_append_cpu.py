"""ragged_rope_append off the GPU: the torch fallback against float64, the
`lens` and skip rules, and the engine with `fused_kv_append` step for step
against the default path (bit-identical pools, lengths and tokens)."""
import pytest
import torch

from ragged_rope_append_refs import (POOL, SEQS, SEQS_T1, SKIP_BAD,
                                     SKIP_EDITS, SKIP_LENS, SKIP_POOL,
                                     SKIP_SEQS, check_call, make_inputs,
                                     pattern)

from deepspeed_amd.inference.ragged_batch import RaggedBatch
from deepspeed_amd.inference.serving import ContinuousBatchingEngine
from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
from deepspeed_amd.ops.functional import ragged_rope_append


def _run(seqs, B, Smax, P, Hq, Hk, D, dtype, edits=(), with_lens=True):
    b = RaggedBatch(seqs, B, Smax)
    slot, pos = b.tok_slot.clone(), b.tok_pos.clone()
    for which, t, val in edits:
        (slot if which == "slot" else pos)[t] = val
    T = b.total_tokens
    q, k, v, cos, sin = make_inputs(T, Hq, Hk, D, P, dtype, "cpu")
    kp = pattern((B, Smax, Hk, D), dtype, "cpu", salt=1)
    vp = pattern((B, Smax, Hk, D), dtype, "cpu", salt=2)
    lens = torch.arange(100, 100 + B) if with_lens else None
    before = [t.clone() for t in (q, k, v, kp, vp)]
    lens0 = lens.clone() if with_lens else None
    out = ragged_rope_append(q, k, v, cos, sin, slot, pos, kp, vp, lens)
    for name, t, t0 in zip("qkv", (q, k, v), before):
        assert torch.equal(t, t0), f"{name} was modified"
    check_call(out, q, k, v, cos, sin, slot, pos, kp, vp, before[3],
               before[4], lens, lens0, f"fallback {dtype}")
    return out, kp, vp, lens


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Hq,Hk,D", [(4, 2, 64), (3, 3, 24), (2, 1, 6)])
@pytest.mark.parametrize("T", [1, 7, 300])
def test_fallback_vs_float64(T, Hq, Hk, D, dtype):
    """fp32 in and out: 3*U24*(|a*c|+|b*s|); bf16 adds one output rounding.
    V rows bit-exact, nothing else in the pools touched, q/k/v unchanged."""
    B, Smax, P = POOL[T]
    for seqs in (SEQS_T1 if T == 1 else [SEQS[T]]):
        _run(seqs, B, Smax, P, Hq, Hk, D, dtype)
        _run(seqs, B, Smax, P, Hq, Hk, D, dtype, with_lens=False)


def test_lens_rule():
    """Shuffled slots, multi-token chunks next to decode rows: only the
    slots the batch names change, each to its kv_len."""
    B, Smax, P = POOL[7]
    _, _, _, lens = _run(SEQS[7], B, Smax, P, 4, 2, 16, torch.float32)
    want = torch.arange(100, 100 + B)
    for slot, _, _, kv_len in SEQS[7]:
        want[slot] = kv_len
    assert torch.equal(lens, want)
    B, Smax, P = POOL[300]
    _, _, _, lens = _run(SEQS[300], B, Smax, P, 2, 1, 6, torch.float32)
    named = {s[0]: s[3] for s in SEQS[300]}
    assert lens.tolist() == [named.get(i, 100 + i) for i in range(B)]


def test_skip_rule():
    """slot -1 / B and pos -1 / Smax / P: nothing written for those tokens,
    their q_rot rows are zero, every other token is served as usual."""
    B, Smax, P = SKIP_POOL
    good, kp_g, vp_g, _ = _run(SKIP_SEQS, B, Smax, P, 4, 2, 16,
                               torch.float32)
    out, kp, vp, lens = _run(SKIP_SEQS, B, Smax, P, 4, 2, 16, torch.float32,
                             edits=SKIP_EDITS)
    keep = [t for t in range(out.shape[0]) if t not in SKIP_BAD]
    assert not out[SKIP_BAD].abs().any()
    assert torch.equal(out[keep], good[keep])       # neighbours unaffected
    assert lens.tolist() == [SKIP_LENS.get(i, 100 + i) for i in range(B)]
    # each bad token's own pool row kept the fill; check_call compared the
    # rest of the pool. Rows of the valid run differ there, so this bites.
    b = RaggedBatch(SKIP_SEQS, B, Smax)
    fill_k = pattern((B, Smax, 2, 16), torch.float32, "cpu", salt=1)
    for t in (2, 7, 8):      # pos-edited tokens: their true row is unwritten
        s, p = int(b.tok_slot[t]), int(b.tok_pos[t])
        assert torch.equal(kp[s, p], fill_k[s, p])
        assert not torch.equal(kp_g[s, p], fill_k[s, p])


def _model():
    torch.manual_seed(0)
    return LlamaForCausalLM(LLAMA_CONFIGS["llama-tiny"]).eval()


@pytest.mark.parametrize("fused_step,chunk,budget", [
    (True, 4, 8), (False, 4, None), (False, None, None)])
def test_engine_matches_default_path(fused_step, chunk, budget):
    """fp32 llama-tiny: after EVERY step the k, v and lens of every layer
    are torch.equal between fused_kv_append=True and the default, and so are
    the generated tokens (the fallback is built from the same pieces)."""
    model = _model()
    torch.manual_seed(3)
    prompts = [torch.randint(0, 2000, (n,)) for n in (6, 13, 4, 9)]
    engines = []
    for flag in (False, True):
        cb = ContinuousBatchingEngine(model, max_batch=2, max_seq=64,
                                      prefill_chunk=chunk,
                                      prefill_budget=budget,
                                      fused_step=fused_step,
                                      fused_kv_append=flag)
        rids = [cb.add_request(p, max_new_tokens=5) for p in prompts]
        engines.append((cb, rids, {}))
    assert engines[0][0].caches[0].rope is None
    assert engines[1][0].caches[0].rope[0].dtype == torch.float32
    steps = 0
    (a, _, out_a), (b, _, out_b) = engines
    while a.pending or a.prefilling or a.running:
        for cb, _, out in engines:
            for r in cb.step():
                out[r.rid] = r.tokens
        steps += 1
        for i, (ca, cb_) in enumerate(zip(a.caches, b.caches)):
            assert torch.equal(ca.k, cb_.k), (steps, i, "k")
            assert torch.equal(ca.v, cb_.v), (steps, i, "v")
            assert torch.equal(ca.lens, cb_.lens), (steps, i, "lens")
        assert steps < 200
    assert not (b.pending or b.prefilling or b.running)
    assert sorted(b.free_slots) == [0, 1]
    assert len(out_a) == len(prompts)
    for rid in engines[0][1]:
        assert torch.equal(out_a[rid], out_b[rid]), rid
        assert len(out_b[rid]) == len(prompts[rid]) + 5
