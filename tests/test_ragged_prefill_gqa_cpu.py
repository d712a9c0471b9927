"""The windowed fused serving step off the GPU: the banded float64 reference
against the plain one, the torch fallback inside the banded bound, and the
fp32 engine with fused_step=True and a sliding window."""
import dataclasses

import pytest
import torch

from edge_refs import assert_within
from ragged_prefill_band_refs import (BAND_PAIRS, greedy_no_cache,
                                      ragged_prefill_band_ref)
from ragged_prefill_refs import (N_SLOTS, SMAX, make_ragged_prefill,
                                 ragged_prefill_ref)

from deepspeed_amd.inference.ragged_batch import RaggedBatch
from deepspeed_amd.inference.serving import ContinuousBatchingEngine
from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
from deepspeed_amd.ops.functional import ragged_prefill_attention


def _case():
    return make_ragged_prefill(BAND_PAIRS, 3, 64, 2, dtype=torch.float32,
                               poison=False)


def test_band_ref_without_a_band_is_the_plain_ref():
    q, kp, vp, seqs = _case()
    plain = ragged_prefill_ref(q, kp, vp, seqs)
    band = ragged_prefill_band_ref(q, kp, vp, seqs, max(s[3] for s in seqs))
    assert torch.equal(band["out"], plain["out"])
    assert torch.equal(band["tol"], plain["tol"])


@pytest.mark.parametrize("window", (1, 5, 33))
def test_torch_fallback_inside_the_banded_bound(window):
    """fp32 output: the slack without the final bf16 rounding term."""
    q, kp, vp, seqs = _case()
    ref = ragged_prefill_band_ref(q, kp, vp, seqs, window)
    out = ragged_prefill_attention(q, kp, vp,
                                   RaggedBatch(seqs, N_SLOTS, SMAX),
                                   window=window)
    assert_within(out, ref["out"], ref["slack"], f"window {window}")


def _windowed_model():
    cfg = dataclasses.replace(LLAMA_CONFIGS["llama-tiny"], sliding_window=16)
    torch.manual_seed(0)
    return cfg, LlamaForCausalLM(cfg).float().eval()


def test_fused_step_with_a_window_matches_recompute():
    cfg, model = _windowed_model()
    torch.manual_seed(1)
    prompts = [torch.randint(0, cfg.vocab_size, (n,)) for n in (3, 16, 21, 37)]
    with torch.no_grad():
        refs = [greedy_no_cache(model, p, 6) for p in prompts]
    cb = ContinuousBatchingEngine(model, max_batch=3, max_seq=64,
                                  prefill_chunk=5, fused_step=True)
    rids = [cb.add_request(p, max_new_tokens=6) for p in prompts]
    out = cb.run()
    assert sorted(cb.free_slots) == [0, 1, 2] and not cb.running
    for rid, ref in zip(rids, refs):
        assert torch.equal(out[rid], ref), rid


def test_fp8_pool_with_a_window_refuses_the_fused_step():
    with pytest.raises(NotImplementedError):
        ContinuousBatchingEngine(_windowed_model()[1], max_batch=2,
                                 prefill_chunk=4, fused_step=True,
                                 fused_kv_append=True, kv_dtype="fp8")
