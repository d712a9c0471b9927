"""Sliding window over the fp8 KV slot pool, off the GPU: the torch fallback
of `ragged_decode_attention_fp8` and the serving classes that used to refuse
the combination."""
import dataclasses

import pytest
import torch

from deepspeed_amd.ops import functional as Fops

LENS = [1, 7, 8, 9, 20]


@pytest.mark.parametrize("window", [3, 8, 20, 64])
def test_fp8_window_fallback_equals_bf16_fallback_on_dequantized(window):
    """fp32 on the CPU: the same torch loop over the same dequantized values,
    bit for bit, for windows below, at and above the lengths."""
    torch.manual_seed(window)
    B, Smax, Hk, G, D = 6, 24, 2, 3, 64
    kc, ks = Fops.kv_quantize(torch.randn(B, Smax, Hk, D))
    vc, vs = Fops.kv_quantize(torch.randn(B, Smax, Hk, D))
    rows = torch.tensor([4, 0, 5, 2, 1])
    lens = torch.tensor(LENS)
    q = torch.randn(len(LENS), 1, Hk * G, D)
    out = Fops.ragged_decode_attention_fp8(q, kc, vc, ks, vs, rows, lens,
                                           window=window)
    want = Fops.ragged_decode_attention(
        q, Fops.kv_dequantize(kc, ks, q.dtype),
        Fops.kv_dequantize(vc, vs, q.dtype), rows, lens, window=window)
    assert out.shape == want.shape == (len(LENS), 1, Hk * G, D)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    full = Fops.ragged_decode_attention_fp8(q, kc, vc, ks, vs, rows, lens)
    short = lens <= window          # the window changes the longer rows only
    assert torch.equal(out[short], full[short])
    assert short.all() or not torch.equal(out[~short], full[~short])
    with pytest.raises(ValueError):
        Fops.ragged_decode_attention_fp8(q, kc, vc, ks, vs, rows, lens,
                                         window=0)


def test_fp8_pool_with_window_constructs_and_serves():
    from deepspeed_amd.inference.serving import (ContinuousBatchingEngine,
                                                 RaggedKVCache)
    from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
    rope = (torch.ones(32, 32), torch.zeros(32, 32))
    c = RaggedKVCache(2, 32, 2, 64, torch.float32, "cpu", rope=rope, fp8=True,
                      window=8)
    assert c.fp8 and c.window == 8 and c.k.dtype == torch.float8_e4m3fn

    cfg = dataclasses.replace(LLAMA_CONFIGS["llama-tiny"],
                              num_hidden_layers=2, num_attention_heads=4,
                              num_key_value_heads=2, sliding_window=8)
    assert cfg.head_dim == 64
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    torch.manual_seed(1)
    prompts = [torch.randint(0, 2000, (n,)) for n in (5, 12, 19)]
    new = 4
    cb = ContinuousBatchingEngine(model, max_batch=2, max_seq=32,
                                  prefill_chunk=8, fused_kv_append=True,
                                  kv_dtype="fp8")
    rids = [cb.add_request(p, max_new_tokens=new) for p in prompts]
    out = cb.run()
    assert sorted(cb.free_slots) == [0, 1]
    assert not cb.running and not cb.pending and not cb.prefilling
    for rid, p in zip(rids, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
