"""ragged_rope_append HIP kernel and the engine's fused_kv_append path (needs
MI355X). Elementwise against float64 with the derived bound of
ragged_rope_append_refs; pools are interior views of larger pattern-filled
buffers, so a stray write anywhere in the allocation fails a bit compare.

Dispatch arms reached:
  (Hq,Hk,D) in {(4,2,64), (1,1,128), (8,1,128), (2,2,16)}
      ragged_rope_append_kernel (bf16x8), half8 = 4 / 8 / 8 / 1, GQA 2/1/8/1
  D in {24, 6}; D = 64 with q one element off 16-byte alignment
      ragged_rope_append_kernel_scalar
  T in {1, 7, 300}; T = 175000 (D=16) / 45000 (D=6)
      one lane group / tail / several blocks; second trip of the grid-stride
      loop in both arms
  with / without lens; slot -1 / B, pos -1 / Smax / P
      lens == nullptr arm; device guard (token skipped, q_rot row zeroed)
"""
import pytest
import torch

from ragged_rope_append_refs import (POOL, SEQS, SEQS_T1, SKIP_BAD,
                                     SKIP_EDITS, SKIP_LENS, SKIP_POOL,
                                     SKIP_SEQS, bits, check_call, make_inputs,
                                     pattern)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
SHAPES = [(4, 2, 64), (1, 1, 128), (8, 1, 128), (2, 2, 16), (3, 3, 24),
          (2, 1, 6)]


def _ext():
    return get_ext(required=True)


def _interior(shape, lead, tail, dtype, salt):
    """`shape` as an interior view (along dim 0) of a larger pattern buffer."""
    buf = pattern((lead + shape[0] + tail,) + tuple(shape[1:]), dtype, DEV,
                  salt=salt)
    return buf, buf[lead:lead + shape[0]]


def _outside_equal(buf, buf0, lead, n, what):
    assert torch.equal(bits(buf[:lead]), bits(buf0[:lead])) and \
        torch.equal(bits(buf[lead + n:]), bits(buf0[lead + n:])), \
        f"{what}: buffer changed outside the view"


def _call(seqs, B, Smax, P, Hq, Hk, D, with_lens=True, misalign_q=False,
          edits=(), lead=1, tail=1, what=""):
    from deepspeed_amd.inference.ragged_batch import RaggedBatch
    b = RaggedBatch(seqs, B, Smax, DEV)
    slot, pos = b.tok_slot, b.tok_pos
    if edits:
        slot, pos = slot.clone(), pos.clone()
        for which, t, val in edits:
            (slot if which == "slot" else pos)[t] = val
    T = b.total_tokens
    q, k, v, cos, sin = make_inputs(T, Hq, Hk, D, P, BF, DEV)
    if misalign_q:      # same values, based one bf16 off 16-byte alignment
        qbuf = torch.zeros(q.numel() + 8, dtype=BF, device=DEV)
        qbuf[1:1 + q.numel()] = q.reshape(-1)
        q = qbuf[1:1 + q.numel()].view(T, Hq, D)
        assert q.is_contiguous() and q.data_ptr() % 16 == 2
    cbuf, cos_v = _interior((P, D // 2), 2, 2, torch.float32, 5)
    sbuf, sin_v = _interior((P, D // 2), 2, 2, torch.float32, 6)
    cos_v.copy_(cos)
    sin_v.copy_(sin)
    kbuf, kp = _interior((B, Smax, Hk, D), lead, tail, BF, 1)
    vbuf, vp = _interior((B, Smax, Hk, D), lead, tail, BF, 2)
    lbuf = torch.arange(98, 98 + B + 4, device=DEV)
    lens = lbuf[2:2 + B]
    assert lens.is_contiguous() and kp.is_contiguous()
    snap = [t.clone() for t in (q, k, v, kbuf, vbuf, lbuf, cbuf, sbuf)]
    out = _ext().ragged_rope_append(q, k, v, cos_v, sin_v, slot, pos, kp, vp,
                                    lens if with_lens else None)
    torch.cuda.synchronize()
    for name, t, t0 in zip(("q", "k", "v"), (q, k, v), snap):
        assert torch.equal(bits(t), bits(t0)), f"{what}: {name} modified"
    assert torch.equal(cbuf, snap[6]) and torch.equal(sbuf, snap[7]), \
        f"{what}: tables modified"
    _outside_equal(kbuf, snap[3], lead, B, f"{what} kpool")
    _outside_equal(vbuf, snap[4], lead, B, f"{what} vpool")
    _outside_equal(lbuf, snap[5], 2, B, f"{what} lens")
    if not with_lens:
        assert torch.equal(lbuf, snap[5]), f"{what}: lens written"
    check_call(out, q, k, v, cos_v, sin_v, slot, pos, kp, vp,
               snap[3][lead:lead + B], snap[4][lead:lead + B],
               lens if with_lens else None, snap[5][2:2 + B], what)
    return out, lens


@pytest.mark.parametrize("T", [1, 7, 300])
@pytest.mark.parametrize("Hq,Hk,D", SHAPES)
def test_kernel_vs_float64(T, Hq, Hk, D):
    """Vector arm (D/2 % 8 == 0) and scalar arm; T = 1, a tail, and more than
    one block of work. With and without `lens`."""
    B, Smax, P = POOL[T]
    for seqs in (SEQS_T1 if T == 1 else [SEQS[T]]):
        what = f"T={T} Hq={Hq} Hk={Hk} D={D}"
        _, lens = _call(seqs, B, Smax, P, Hq, Hk, D, what=what)
        for slot, _, _, kv_len in seqs:
            assert int(lens[slot]) == kv_len
        _call(seqs, B, Smax, P, Hq, Hk, D, with_lens=False,
              what=what + " no lens")


def test_kernel_misaligned_q_takes_scalar_arm():
    """A vector shape whose q starts one element off 16-byte alignment."""
    B, Smax, P = POOL[7]
    _call(SEQS[7], B, Smax, P, 4, 2, 64, misalign_q=True, what="misaligned")


@pytest.mark.parametrize("Hq,Hk,D,B,Smax,T", [
    (1, 1, 16, 256, 1024, 175000),      # vector arm: 3 * T items
    (2, 1, 6, 64, 1024, 45000),         # scalar arm: 12 * T items
])
def test_kernel_grid_stride(Hq, Hk, D, B, Smax, T):
    """More work items than the capped grid has threads (2048 * 256), so the
    grid-stride loop takes a second trip."""
    assert T * (Hq + 2 * Hk) * (D // 16 if D % 16 == 0 else D // 2) \
        > 2048 * 256
    seqs, t, slot = [], 0, B - 1
    while t < T:                         # full slots from B-1 downwards
        n = min(Smax, T - t)
        seqs.append((slot, t, n, n))
        t += n
        slot -= 1
    _call(seqs, B, Smax, Smax, Hq, Hk, D, what=f"grid-stride D={D}")


@pytest.mark.parametrize("Hq,Hk,D", [(4, 2, 64), (2, 1, 6)])
def test_kernel_skip_rule(Hq, Hk, D):
    """slot -1 / B, pos -1 / Smax / P. Pools, lens and tables are interior
    views with room on both sides (pos = P from slot 4 lands two slots on),
    so even an unguarded access would stay inside allocated memory; the whole
    outer buffers are compared."""
    B, Smax, P = SKIP_POOL
    good, _ = _call(SKIP_SEQS, B, Smax, P, Hq, Hk, D, lead=2, tail=4,
                    what="skip: valid run")
    out, lens = _call(SKIP_SEQS, B, Smax, P, Hq, Hk, D, lead=2, tail=4,
                      edits=SKIP_EDITS, what=f"skip D={D}")
    keep = [t for t in range(out.shape[0]) if t not in SKIP_BAD]
    assert not out[SKIP_BAD].float().abs().any()
    assert torch.equal(bits(out[keep]), bits(good[keep]))
    assert lens.tolist() == [SKIP_LENS.get(i, 100 + i) for i in range(B)]


def test_kernel_rejects_bad_arguments():
    """Every bad tensor is at least as large as the good one, so indexing
    would stay in allocated memory even without the checks."""
    e = _ext()
    T, Hq, Hk, D, B, Smax, P = 6, 4, 2, 64, 4, 16, 32
    q, k, v, cos, sin = make_inputs(T, Hq, Hk, D, P, BF, DEV)
    kp = torch.zeros(B, Smax, Hk, D, device=DEV, dtype=BF)
    vp = torch.zeros_like(kp)
    slot = torch.tensor([2, 2, 2, 0, 3, 1], device=DEV)
    pos = torch.tensor([0, 1, 2, 15, 7, 3], device=DEV)
    lens = torch.zeros(B, dtype=torch.long, device=DEV)
    good = dict(q=q, k=k, v=v, cos=cos, sin=sin, tok_slot=slot, tok_pos=pos,
                kpool=kp, vpool=vp, lens=lens)
    e.ragged_rope_append(**good)                            # the good call
    strided = torch.zeros(2 * T, dtype=torch.long, device=DEV)[::2]
    assert strided.shape == slot.shape and not strided.is_contiguous()
    wide = torch.zeros(B, Smax, Hk, 2 * D, device=DEV, dtype=BF)
    bad = {
        "q dtype": dict(q=q.float()),
        "k dtype": dict(k=k.half()),
        "cos dtype": dict(cos=cos.double()),
        "kpool dtype": dict(kpool=kp.float()),
        "q device": dict(q=q.cpu()),
        "tok_pos device": dict(tok_pos=pos.cpu()),
        "vpool device": dict(vpool=vp.cpu()),
        "lens device": dict(lens=lens.cpu()),
        "q rank": dict(q=q.unsqueeze(0)),
        "kpool rank": dict(kpool=kp.unsqueeze(0), vpool=vp.unsqueeze(0)),
        "tok_slot rank": dict(tok_slot=slot.view(1, T)),
        "tok_slot strided": dict(tok_slot=strided),
        "tok_pos strided": dict(tok_pos=strided),
        "tok_slot int32": dict(tok_slot=slot.int()),
        "tok_pos int32": dict(tok_pos=pos.int()),
        "tok_slot length": dict(tok_slot=torch.cat([slot, slot])),
        "Hq % Hk": dict(q=torch.zeros(T, 5, D, device=DEV, dtype=BF)),
        "pool head_dim": dict(kpool=wide, vpool=wide),
        "pool heads": dict(
            kpool=torch.zeros(B, Smax, 2 * Hk, D, device=DEV, dtype=BF),
            vpool=torch.zeros(B, Smax, 2 * Hk, D, device=DEV, dtype=BF)),
        "vpool shape": dict(
            vpool=torch.zeros(B + 1, Smax, Hk, D, device=DEV, dtype=BF)),
        "P < Smax": dict(
            kpool=torch.zeros(B, P + 1, Hk, D, device=DEV, dtype=BF),
            vpool=torch.zeros(B, P + 1, Hk, D, device=DEV, dtype=BF)),
        "lens length": dict(
            lens=torch.zeros(B + 1, dtype=torch.long, device=DEV)),
        "lens int32": dict(
            lens=torch.zeros(2 * B, dtype=torch.int32, device=DEV)),
    }
    for name, change in bad.items():
        with pytest.raises(RuntimeError):
            e.ragged_rope_append(**{**good, **change})
            pytest.fail(f"'{name}' did not raise")
    empty = e.ragged_rope_append(q[:0], k[:0], v[:0], cos, sin, slot[:0],
                                 pos[:0], kp, vp, lens)
    assert empty.shape == (0, Hq, D)


@pytest.mark.parametrize("fused_step", [True, False])
def test_engine_fused_kv_append_gpu(monkeypatch, fused_step):
    """The bf16 Llama of test_fused_step_engine_gpu with fused_kv_append:
    one ragged_rope_append launch per layer on every fused step (resp. every
    decode step of the unfused engine) and no eager RoPE anywhere. The kernel
    may contract to FMA and differ from the eager RoPE by one bf16 ulp, so
    the criterion is the existing agreement >= 0.75; bookkeeping is exact."""
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

    calls = {"kernel": 0, "rope_torch": 0, "model": 0, "decode": 0}
    real_kernel, real_rope = _ext().ragged_rope_append, Fops._rope_torch

    def kernel(*a, **kw):
        calls["kernel"] += 1
        return real_kernel(*a, **kw)

    def rope_torch(*a, **kw):
        calls["rope_torch"] += 1
        return real_rope(*a, **kw)

    monkeypatch.setattr(_ext(), "ragged_rope_append", kernel)
    monkeypatch.setattr(Fops, "_rope_torch", rope_torch)
    hook = model.register_forward_hook(
        lambda *a: calls.__setitem__("model", calls["model"] + 1))
    cb = ContinuousBatchingEngine(model, max_batch=2, prefill_chunk=16,
                                  prefill_budget=32, fused_step=fused_step,
                                  fused_kv_append=True)
    real_decode = cb._decode

    def decode(active):
        calls["decode"] += 1
        return real_decode(active)

    monkeypatch.setattr(cb, "_decode", decode)
    rids = [cb.add_request(p, max_new_tokens=new) for p in prompts]
    out = cb.run()
    hook.remove()

    assert sorted(cb.free_slots) == [0, 1]
    assert not cb.running and not cb.pending and not cb.prefilling
    assert calls["rope_torch"] == 0
    if fused_step:
        assert calls["model"] >= 1 and calls["decode"] == 0
        assert calls["kernel"] == calls["model"] * cfg.num_hidden_layers
    else:
        assert 1 <= calls["decode"] < calls["model"]
        assert calls["kernel"] == calls["decode"] * cfg.num_hidden_layers
    for c in cb.caches:
        assert c.rope[0].dtype == torch.float32
    for rid, ref, p in zip(rids, refs, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
        agree = (out[rid].to(DEV) == ref).float().mean().item()
        assert agree >= 0.75, (rid, agree)
