"""fp8 KV slot pool off the GPU: kv_quantize / kv_dequantize, the torch
fallbacks of the three fp8 ops against the checks and bounds of kv_fp8_refs,
the proof that those bounds are VALID (a torch emulation of what the kernels
round stays inside them) and SHARP (the emulation with one edge broken does
not), and the engine with kv_dtype="fp8"."""
import pytest
import torch

from attn_refs import RAGGED_SHAPES
from edge_refs import assert_within
from kv_fp8_refs import (FP8, MUTANTS, check_append_fp8, check_engine,
                         code_bits, decode_case, dequant64, emulate_fp8,
                         mutant_applies, pool_pattern, prefill_case)
from ragged_prefill_refs import BATCHES
from ragged_rope_append_refs import (POOL, SEQS, SEQS_T1, SKIP_EDITS,
                                     SKIP_POOL, SKIP_SEQS, make_inputs)

from deepspeed_amd.inference.ragged_batch import RaggedBatch
from deepspeed_amd.ops import functional as Fops

APPEND_SHAPES = [(Hq, Hk, D) for D in (64, 128) for Hq, Hk in
                 ((1, 1), (4, 1), (4, 4))]
PREFILL_SHAPES = [(4, 64, 2), (1, 128, 1), (2, 128, 2), (8, 64, 1)]


# ---------------------------------------------------------------- format
def test_kv_quantize_format():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(6, 3, 64, generator=g) *
         torch.exp2(torch.arange(6).float() - 3).view(6, 1, 1)).bfloat16()
    x[1, 2] = 0                                  # all-zero row
    x[2, 0, 5] = 2.0 ** -20                      # lands in the subnormal range
    codes, scale = Fops.kv_quantize(x)
    assert codes.dtype == FP8 and codes.shape == x.shape
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1]
    amax = x.float().abs().amax(-1)
    assert scale[1, 2] == 1.0 and not code_bits(codes[1, 2]).any()
    nz = amax > 0
    assert torch.equal(scale[nz], amax[nz] / 448.0)
    assert not codes.float().isnan().any()
    assert codes.float().abs().max() == 448.0    # every row's amax saturates
    deq = Fops.kv_dequantize(codes, scale)
    assert deq.dtype == torch.float32
    assert torch.equal(deq.double(), dequant64(codes, scale).float().double())
    err = (dequant64(codes, scale) - x.double()).abs()
    bound = torch.maximum(2.0 ** -4 * x.double().abs(),
                          (scale.double() * 2.0 ** -10).unsqueeze(-1)) \
        + 4 * 2.0 ** -24 * x.double().abs()
    assert (err <= bound).all()


# ---------------------------------------------------------------- append
def _append(seqs, B, Smax, P, Hq, Hk, D, dtype, identity, edits=(),
            with_lens=True):
    b = RaggedBatch(seqs, B, Smax)
    slot, pos = b.tok_slot, b.tok_pos
    if edits:
        slot, pos = slot.clone(), pos.clone()
        for which, t, val in edits:
            (slot if which == "slot" else pos)[t] = val
    q, k, v, cos, sin = make_inputs(b.total_tokens, Hq, Hk, D, P, dtype,
                                    "cpu")
    k[0, 0] = 0                                  # all-zero rows
    v[-1, Hk - 1] = 0
    if identity:
        cos, sin = torch.ones_like(cos), torch.zeros_like(sin)
    kp, ks = pool_pattern(B, Smax, Hk, D, "cpu", 1)
    vp, vs = pool_pattern(B, Smax, Hk, D, "cpu", 2)
    lens = torch.arange(100, 100 + B) if with_lens else None
    pools0 = tuple(t.clone() for t in (kp, vp, ks, vs))
    lens0 = torch.arange(100, 100 + B)
    out = Fops.ragged_rope_append_fp8(q, k, v, cos, sin, slot, pos, kp, vp,
                                      ks, vs, lens)
    check_append_fp8(out, q, k, v, cos, sin, slot, pos, (kp, vp, ks, vs),
                     pools0, lens, lens0, f"D={D} Hq={Hq} Hk={Hk}", identity)


@pytest.mark.parametrize("identity", [True, False])
@pytest.mark.parametrize("Hq,Hk,D", APPEND_SHAPES)
def test_append_fallback(Hq, Hk, D, identity):
    for T in (1, 7, 300):
        B, Smax, P = POOL[T]
        for seqs in (SEQS_T1 if T == 1 else [SEQS[T]]):
            _append(seqs, B, Smax, P, Hq, Hk, D, torch.float32, identity)
    _append(SEQS[7], *POOL[7], Hq, Hk, D, torch.bfloat16, identity,
            with_lens=False)


@pytest.mark.parametrize("D", [64, 128])
def test_append_fallback_skip_rule(D):
    B, Smax, P = SKIP_POOL
    _append(SKIP_SEQS, B, Smax, P, 4, 2, D, torch.float32, False,
            edits=SKIP_EDITS)


def test_fp8_ops_reject_other_head_dims_and_dtypes():
    B, Smax, Hk, T = 2, 8, 1, 2
    slot, pos = torch.tensor([0, 1]), torch.tensor([0, 0])
    for D in (32, 96, 256):
        q = torch.zeros(T, Hk, D)
        kp = torch.zeros(B, Smax, Hk, D).to(FP8)
        sc = torch.ones(B, Smax, Hk)
        cs = torch.ones(Smax, D // 2)
        with pytest.raises(ValueError):
            Fops.ragged_rope_append_fp8(q, q, q, cs, cs, slot, pos, kp, kp,
                                        sc, sc)
        with pytest.raises(ValueError):
            Fops.ragged_decode_attention_fp8(q.unsqueeze(1), kp, kp, sc, sc,
                                             slot, pos + 1)
    q = torch.zeros(T, Hk, 64)
    with pytest.raises(ValueError):              # a bf16 pool is not fp8
        Fops.ragged_decode_attention_fp8(
            q.unsqueeze(1), torch.zeros(B, Smax, Hk, 64),
            torch.zeros(B, Smax, Hk, 64), torch.ones(B, Smax, Hk),
            torch.ones(B, Smax, Hk), slot, pos + 1)


# ------------------------------------------------- decode / prefill bound
@pytest.mark.parametrize("G,D,Hk", RAGGED_SHAPES)
def test_decode_emulation_valid_and_sharp(G, D, Hk):
    for lens_name in ("A", "B"):
        c = decode_case(lens_name, G, D, Hk)
        assert not torch.isnan(c["out"]).any()
        got = emulate_fp8(c["q"][:, 0], c["clean"], c["seqs"], False)
        assert_within(got.unsqueeze(1), c["out"], c["tol"], "emulation")
        for mut in MUTANTS:
            if not mutant_applies(mut, c["seqs"], Hk):
                continue
            got = emulate_fp8(c["q"][:, 0], c["clean"], c["seqs"], False,
                              mut=mut)
            with pytest.raises(AssertionError):
                assert_within(got.unsqueeze(1), c["out"], c["tol"], mut)


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("G,D,Hk", PREFILL_SHAPES)
def test_prefill_emulation_valid_and_sharp(name, G, D, Hk):
    c = prefill_case(name, G, D, Hk)
    assert not torch.isnan(c["out"]).any()
    got = emulate_fp8(c["q"], c["clean"], c["seqs"], True)
    assert_within(got, c["out"], c["tol"], "emulation")
    for mut in MUTANTS:
        if not mutant_applies(mut, c["seqs"], Hk):
            continue
        got = emulate_fp8(c["q"], c["clean"], c["seqs"], True, mut=mut)
        with pytest.raises(AssertionError):
            assert_within(got, c["out"], c["tol"], mut)


def test_attention_fallbacks_on_the_fp8_pool():
    """The torch fallbacks (fp32 q) over the clean pool, held to the fp8
    bounds; the poisoned pool must give the same bits."""
    c = decode_case("A", 4, 64, 2)
    q = c["q"].float()
    out = Fops.ragged_decode_attention_fp8(q, *c["clean"], c["rows"],
                                           c["lens"])
    assert out.shape == q.shape
    assert_within(out, c["out"], c["tol"], "decode fallback")
    again = Fops.ragged_decode_attention_fp8(q, *c["poisoned"], c["rows"],
                                             c["lens"])
    assert torch.equal(out, again)
    c = prefill_case("mixed", 4, 64, 2)
    q = c["q"].float()
    kc = c["clean"][0]
    b = RaggedBatch(c["seqs"], kc.shape[0], kc.shape[1])
    out = Fops.ragged_prefill_attention_fp8(q, *c["clean"], b)
    assert_within(out, c["out"], c["tol"], "prefill fallback")
    again = Fops.ragged_prefill_attention_fp8(q, *c["poisoned"], b)
    assert torch.equal(out, again)


# ---------------------------------------------------------------- engine
def test_engine_fp8_needs_fused_kv_append():
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine
    from kv_fp8_refs import tiny_llama
    model = tiny_llama("cpu", torch.float32)
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(model, max_batch=2, kv_dtype="fp8")
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(model, max_batch=2, fused_kv_append=True,
                                 kv_dtype="int8")
    cb = ContinuousBatchingEngine(model, max_batch=2, fused_kv_append=True,
                                  kv_dtype=torch.float8_e4m3fn)
    assert cb.caches[0].k.dtype == FP8
    cb = ContinuousBatchingEngine(model, max_batch=2, fused_kv_append=True)
    assert cb.caches[0].k.dtype == torch.float32
    assert cb.caches[0].k_scale is None


def test_engine_fp8_rejects_head_dim_32():
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine
    from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
    model = LlamaForCausalLM(LLAMA_CONFIGS["llama-tiny"]).eval()
    with pytest.raises(ValueError):
        ContinuousBatchingEngine(model, max_batch=2, fused_kv_append=True,
                                 kv_dtype="fp8")


@pytest.mark.parametrize("fused_step", [True, False])
def test_engine_fp8_cpu(fused_step):
    agree = check_engine("cpu", torch.float32, fused_step)
    print(f"greedy agreement fp8 pool vs fp32 pool (fused_step={fused_step},"
          f" reported, not asserted): {agree:.3f}")
