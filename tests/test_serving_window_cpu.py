"""Continuous batching of a sliding-window model on the CPU: the masked
decode and chunked-prefill fallbacks of RaggedKVCache carry the band."""
import dataclasses

import pytest
import torch

from deepspeed_amd.inference.serving import ContinuousBatchingEngine
from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM

WINDOW, NEW = 8, 6


def _greedy_no_cache(model, prompt, new):
    ids = prompt.view(1, -1)
    for _ in range(new):
        nxt = model(ids)[0, -1].float().argmax()
        ids = torch.cat([ids, nxt.view(1, 1)], dim=1)
    return ids[0]


@pytest.mark.parametrize("prefill_chunk", [None, 5])
def test_sliding_window_serving_matches_recompute(prefill_chunk):
    """fp32 llama-tiny with sliding_window=8; prompts on both sides of the
    window. Tokens must equal a greedy recompute of the whole sequence."""
    cfg = dataclasses.replace(LLAMA_CONFIGS["llama-tiny"],
                              sliding_window=WINDOW)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).float().eval()
    torch.manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,)) for n in (3, 8, 13, 21)]
    with torch.no_grad():
        refs = [_greedy_no_cache(model, p, NEW) for p in prompts]
    cb = ContinuousBatchingEngine(model, max_batch=3, max_seq=64,
                                  prefill_chunk=prefill_chunk)
    assert all(c.window == WINDOW for c in cb.caches)
    rids = [cb.add_request(p, max_new_tokens=NEW) for p in prompts]
    out = cb.run()
    assert sorted(cb.free_slots) == [0, 1, 2] and not cb.running
    for rid, ref in zip(rids, refs):
        assert torch.equal(out[rid], ref), rid
