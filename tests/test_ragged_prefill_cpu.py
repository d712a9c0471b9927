"""Ragged prefill attention off the GPU: the torch fallback against the
float64 reference, RaggedBatch validation, the fused serving step token for
token against sequential generate, one model call per fused step, and
logits_rows."""
import pytest
import torch

from edge_refs import assert_within
from ragged_prefill_refs import (MIXED, N_SLOTS, SMAX, make_ragged_prefill,
                                 ragged_prefill_ref)

from deepspeed_amd.inference.engine import InferenceEngine
from deepspeed_amd.inference.ragged_batch import RaggedBatch
from deepspeed_amd.inference.serving import ContinuousBatchingEngine
from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
from deepspeed_amd.ops.functional import ragged_prefill_attention


def _model():
    torch.manual_seed(0)
    return LlamaForCausalLM(LLAMA_CONFIGS["llama-tiny"]).eval()


@pytest.mark.parametrize("G,D,Hk", [(4, 64, 2), (1, 128, 1), (2, 32, 3)])
def test_torch_fallback_vs_float64(G, D, Hk):
    """fp32 fallback on the mixed batch; the pool is plain data. The bound is
    the kernel's slack WITHOUT the final bf16 rounding term (the output is
    fp32), i.e. tighter than the GPU test's."""
    q, kp, vp, seqs = make_ragged_prefill(MIXED, G, D, Hk,
                                          dtype=torch.float32, poison=False)
    ref = ragged_prefill_ref(q, kp, vp, seqs)
    b = RaggedBatch(seqs, N_SLOTS, SMAX)
    out = ragged_prefill_attention(q, kp, vp, b)
    assert out.shape == q.shape and out.dtype == torch.float32
    assert_within(out, ref["out"], ref["slack"], "torch fallback")


def test_ragged_batch_fields_and_shuffled_q_start():
    seqs = [(3, 6, 2, 10), (0, 0, 5, 5), (7, 5, 1, 4)]   # q_start shuffled
    b = RaggedBatch(seqs, 8, 16)
    assert b.desc.dtype == torch.long and b.desc.tolist() == \
        [list(s) for s in seqs]
    assert b.desc.is_contiguous()
    assert (b.max_qlen, b.max_kvlen, b.total_tokens, b.n) == (5, 10, 8, 3)
    assert b.tok_slot.tolist() == [0, 0, 0, 0, 0, 7, 3, 3]
    assert b.tok_pos.tolist() == [0, 1, 2, 3, 4, 3, 8, 9]
    assert b.last_rows() == [7, 4, 5]


@pytest.mark.parametrize("name,seqs,T", [
    ("slot below 0", [(-1, 0, 2, 2)], None),
    ("slot >= B", [(8, 0, 2, 2)], None),
    ("slot twice", [(1, 0, 2, 2), (1, 2, 1, 5)], None),
    ("q_len 0", [(1, 0, 0, 2)], None),
    ("q_len 0 among others", [(1, 0, 2, 2), (2, 2, 0, 5)], None),
    ("kv_len < q_len", [(1, 0, 3, 2)], None),
    ("kv_len > Smax", [(1, 0, 3, 17)], None),
    ("overlap", [(1, 0, 3, 3), (2, 2, 2, 2)], None),
    ("gap", [(1, 0, 3, 3), (2, 4, 2, 2)], None),
    ("does not start at 0", [(1, 1, 3, 3)], None),
    ("short of T", [(1, 0, 3, 3)], 4),
    ("past T", [(1, 0, 3, 3)], 2),
    ("empty", [], None),
])
def test_ragged_batch_rejects(name, seqs, T):
    with pytest.raises(ValueError):
        RaggedBatch(seqs, 8, 16, total_tokens=T)


def _refs(model, prompts, new):
    eng = InferenceEngine(model)
    return [eng.generate(p.view(1, -1), max_new_tokens=new)[0]
            for p in prompts]


def test_fused_step_staggered_admission():
    model = _model()
    torch.manual_seed(2)
    prompts = [torch.randint(0, 2000, (n,)) for n in (6, 9, 4, 11, 5)]
    refs = _refs(model, prompts, 6)
    cb = ContinuousBatchingEngine(model, max_batch=2, prefill_chunk=4,
                                  fused_step=True)
    rids = [cb.add_request(p, max_new_tokens=6) for p in prompts]
    out = cb.run()
    assert len(out) == len(prompts)
    assert sorted(cb.free_slots) == [0, 1]
    for rid, ref in zip(rids, refs):
        assert torch.equal(out[rid], ref.cpu()), \
            f"req {rid}: {out[rid].tolist()} vs {ref.tolist()}"


@pytest.mark.parametrize("chunk,budget", [(4, 8), (16, None)])
def test_fused_step_chunk_and_budget(chunk, budget):
    model = _model()
    torch.manual_seed(5)
    prompts = [torch.randint(0, 2000, (n,)) for n in (37, 9, 3, 18)]
    assert max(len(p) for p in prompts) > 2 * chunk
    refs = _refs(model, prompts, 5)
    cb = ContinuousBatchingEngine(model, max_batch=3, prefill_chunk=chunk,
                                  prefill_budget=budget, fused_step=True)
    rids = [cb.add_request(p, max_new_tokens=5) for p in prompts]
    out = cb.run()
    assert sorted(cb.free_slots) == [0, 1, 2]
    for rid, ref in zip(rids, refs):
        assert torch.equal(out[rid], ref.cpu()), \
            f"req {rid}: {out[rid].tolist()} vs {ref.tolist()}"


def test_fused_step_needs_chunking():
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(_model(), max_batch=2, fused_step=True)
    ContinuousBatchingEngine(_model(), max_batch=2, prefill_budget=8,
                             fused_step=True)


def _calls_per_step(model, fused):
    """Model forwards of every step in which a prompt was still prefilling
    while another request was decoding."""
    calls = [0]
    hook = model.register_forward_hook(
        lambda *a: calls.__setitem__(0, calls[0] + 1))
    cb = ContinuousBatchingEngine(model, max_batch=3, prefill_chunk=4,
                                  prefill_budget=8, fused_step=fused)
    torch.manual_seed(6)
    cb.add_request(torch.randint(0, 2000, (3,)), max_new_tokens=12)
    for n in (21, 17):
        cb.add_request(torch.randint(0, 2000, (n,)), max_new_tokens=2)
    per_step = []
    while cb.pending or cb.running or cb.prefilling:
        mixed = bool(cb.prefilling or cb.pending) and \
            any(not r.done for r in cb.running)
        before = calls[0]
        cb.step()
        if mixed:
            per_step.append(calls[0] - before)
    hook.remove()
    return per_step


def test_fused_step_is_one_model_call():
    model = _model()
    fused = _calls_per_step(model, True)
    assert len(fused) >= 3 and all(c == 1 for c in fused), fused
    unfused = _calls_per_step(model, False)
    assert len(unfused) >= 3 and all(c > 1 for c in unfused), unfused
    assert sum(unfused) > sum(fused)


def test_logits_rows_matches_indexing():
    model = _model()
    torch.manual_seed(7)
    ids = torch.randint(0, 2000, (1, 19))
    rows = torch.tensor([18, 0, 7, 7])
    with torch.no_grad():
        full = model(ids)
        part = model(ids, logits_rows=rows)
        none = model(ids, logits_rows=rows[:0])
    assert part.shape == (1, 4, full.shape[-1])
    assert none.shape == (1, 0, full.shape[-1])
    torch.testing.assert_close(part, full[:, rows], rtol=1e-5, atol=1e-6)
