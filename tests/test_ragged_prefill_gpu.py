"""Ragged prefill HIP kernel and the fused serving step (needs MI355X).
Elementwise against ragged_prefill_refs.ragged_prefill_ref (float64, derived
bound). Both pools are NaN at every position >= kv_len and in every slot the
descriptors do not name, so a read past a length -- or a masked column that
is multiplied instead of selected away -- fails the comparison; V carries
the sentinel 64 on the last column and on the first new token's diagonal."""
import pytest
import torch

from attn_refs import RAGGED_SHAPES
from edge_refs import assert_within
from ragged_prefill_refs import N_SLOTS, SMAX, ragged_prefill_case

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16


def _ext():
    return get_ext(required=True)


def _batch(seqs):
    from deepspeed_amd.inference.ragged_batch import RaggedBatch
    return RaggedBatch(seqs, N_SLOTS, SMAX, DEV)


@pytest.mark.parametrize("G,D,Hk", RAGGED_SHAPES)
def test_ragged_prefill_vs_float64(G, D, Hk):
    """Mixed batch (decode rows, fresh prompts and chunks over a prefix around
    the 32-token and 64-row tiles, shuffled q_start), a lone (1,1) with
    n = T = 1, and an all-decode batch that ragged_decode must match too."""
    from deepspeed_amd.ops.functional import ragged_prefill_attention
    for name in ("mixed", "lone", "decode"):
        q, kp, vp, seqs, ref = ragged_prefill_case(name, G, D, Hk, DEV)
        b = _batch(seqs)
        out = ragged_prefill_attention(q, kp, vp, b)
        assert out.shape == q.shape and out.dtype == BF
        assert_within(out, ref["out"], ref["tol"], f"{name} ragged_prefill")
        if name == "decode":
            starts = torch.tensor([s[1] for s in seqs], device=DEV)
            dec = _ext().ragged_decode(
                q[starts].unsqueeze(1).contiguous(), kp, vp,
                torch.tensor([s[0] for s in seqs], device=DEV),
                torch.tensor([s[3] for s in seqs], device=DEV), 512)
            assert_within(dec[:, 0], ref["out"][starts], ref["tol"][starts],
                          "decode ragged_decode")


def test_ragged_prefill_rejects_bad_arguments():
    """Pools are leading views of larger buffers and every bad tensor is at
    least as large as the good one: indexing would stay in allocated memory
    even without the checks."""
    e = _ext()
    T, Hk, G, D, B, Smax = 6, 2, 2, 64, 4, 16
    Hq = Hk * G
    kbuf = torch.zeros(B + 2, Smax, Hk, D, device=DEV, dtype=BF)
    vbuf = torch.zeros(B + 2, Smax, Hk, D, device=DEV, dtype=BF)
    kp, vp = kbuf[:B], vbuf[:B]
    q = torch.zeros(T, Hq, D, device=DEV, dtype=BF)
    desc = torch.tensor([[2, 0, 5, 9], [0, 5, 1, 16]], device=DEV)
    e.ragged_prefill(q, kp, vp, desc, 5, 16)                # the good call
    q3 = torch.zeros(T, 3, D, device=DEV, dtype=BF)
    k1 = torch.zeros(B + 2, Smax, 1, D, device=DEV, dtype=BF)[:B]
    wide = torch.zeros(B, Smax, Hk, 2 * D, device=DEV, dtype=BF)
    desc3 = torch.zeros(4, 3, dtype=torch.long, device=DEV)
    strided = torch.zeros(2, 8, dtype=torch.long, device=DEV)[:, ::2]
    assert strided.shape == desc.shape and not strided.is_contiguous()
    bad = {
        "q dtype": lambda: e.ragged_prefill(q.float(), kp, vp, desc, 5, 16),
        "kpool dtype": lambda: e.ragged_prefill(q, kp.float(), vp, desc, 5,
                                                16),
        "vpool dtype": lambda: e.ragged_prefill(q, kp, vp.float(), desc, 5,
                                                16),
        "desc int32": lambda: e.ragged_prefill(q, kp, vp, desc.int(), 5, 16),
        "desc device": lambda: e.ragged_prefill(q, kp, vp, desc.cpu(), 5,
                                                16),
        "kpool device": lambda: e.ragged_prefill(q, kp.cpu(), vp, desc, 5,
                                                 16),
        "desc strided": lambda: e.ragged_prefill(q, kp, vp, strided, 5, 16),
        "desc width 3": lambda: e.ragged_prefill(q, kp, vp, desc3, 5, 16),
        "G = 3": lambda: e.ragged_prefill(q3, k1, k1, desc, 5, 16),
        "pool head_dim": lambda: e.ragged_prefill(q, wide, wide, desc, 5, 16),
        "max_kvlen > Smax": lambda: e.ragged_prefill(q, kp, vp, desc, 5,
                                                     Smax + 1),
        "max_qlen = 0": lambda: e.ragged_prefill(q, kp, vp, desc, 0, 16),
        "max_qlen > max_kvlen": lambda: e.ragged_prefill(q, kp, vp, desc, 9,
                                                         8),
        "vpool shape": lambda: e.ragged_prefill(q, kp, vbuf, desc, 5, 16),
        "q rank": lambda: e.ragged_prefill(q.unsqueeze(0), kp, vp, desc, 5,
                                           16),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"'{name}' did not raise")


def test_fused_step_engine_gpu(monkeypatch):
    """bf16 Llama with head_dim 64, so the extension path is the one taken.
    Agreement criterion of test_continuous_batching_gpu (bf16 argmax ties
    break differently between batched shapes); bookkeeping is exact."""
    import deepspeed_amd.models.llama as llama
    import deepspeed_amd.ops.functional as Fops
    from deepspeed_amd.inference.engine import InferenceEngine
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine

    cfg = llama.LlamaConfig(hidden_size=256, intermediate_size=688,
                            num_hidden_layers=2, num_attention_heads=4,
                            num_key_value_heads=2, vocab_size=2048,
                            max_position_embeddings=512,
                            activation_checkpointing=False)
    assert cfg.head_dim == 64
    torch.manual_seed(0)
    model = llama.LlamaForCausalLM(cfg).to(DEV, BF).eval()
    eng = InferenceEngine(model)
    torch.manual_seed(1)
    prompts = [torch.randint(0, 2000, (n,)) for n in (7, 40, 13, 70)]
    new = 8
    refs = [eng.generate(p.view(1, -1).to(DEV), max_new_tokens=new)[0]
            for p in prompts]

    calls = {"fused": 0, "kernel": 0, "other": 0, "model": 0}
    real_fused, real_flash = Fops.ragged_prefill_attention, \
        llama.flash_attention
    real_kernel = _ext().ragged_prefill

    def fused(q, kpool, vpool, batch):
        calls["fused"] += 1
        return real_fused(q, kpool, vpool, batch)

    def kernel(*a):
        calls["kernel"] += 1
        return real_kernel(*a)

    def flash(*a, **kw):
        calls["other"] += 1
        return real_flash(*a, **kw)

    monkeypatch.setattr(Fops, "ragged_prefill_attention", fused)
    monkeypatch.setattr(_ext(), "ragged_prefill", kernel)
    monkeypatch.setattr(llama, "flash_attention", flash)
    hook = model.register_forward_hook(
        lambda *a: calls.__setitem__("model", calls["model"] + 1))
    cb = ContinuousBatchingEngine(model, max_batch=2, prefill_chunk=16,
                                  prefill_budget=32, fused_step=True)
    rids = [cb.add_request(p, max_new_tokens=new) for p in prompts]
    out = cb.run()
    hook.remove()

    assert sorted(cb.free_slots) == [0, 1]
    assert not cb.running and not cb.pending and not cb.prefilling
    assert calls["model"] >= 1 and calls["other"] == 0
    assert calls["fused"] == calls["kernel"] == \
        calls["model"] * cfg.num_hidden_layers
    for rid, ref, p in zip(rids, refs, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
        agree = (out[rid].to(DEV) == ref).float().mean().item()
        assert agree >= 0.75, (rid, agree)
