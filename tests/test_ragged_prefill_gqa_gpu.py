"""`ragged_prefill_gqa`, the MFMA fused-step kernel (needs MI355X), against
the float64 banded reference and poisoned inputs of ragged_prefill_band_refs."""
import pytest
import torch

from edge_refs import assert_within
from ragged_prefill_band_refs import band_case, greedy_no_cache
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


@pytest.mark.parametrize("Hk", (1, 2))
@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("G", (1, 3, 7, 8, 32))
def test_prefill_gqa_vs_float64(G, D, Hk):
    """The maxima only size the grid and the checks: max_kvlen = Smax and
    max_qlen = T (cut to Smax: the host wants max_qlen <= max_kvlen) give the
    same bits."""
    for window in (0, 1, 5, 33, 64, 1000):
        q, kp, vp, seqs, ref = band_case(G, D, Hk, window, DEV)
        b = _batch(seqs)
        out = _ext().ragged_prefill_gqa(q, kp, vp, b.desc, b.max_qlen,
                                        b.max_kvlen, window)
        assert out.shape == q.shape and out.dtype == BF
        assert not out.isnan().any(), window
        assert_within(out, ref["out"], ref["tol"], f"window {window}")
        wide = _ext().ragged_prefill_gqa(q, kp, vp, b.desc,
                                         min(q.shape[0], SMAX), SMAX, window)
        assert torch.equal(wide, out), window


@pytest.mark.parametrize("G", (1, 2, 4, 8))
def test_prefill_gqa_shares_the_bound_of_ragged_prefill(G):
    q, kp, vp, seqs, ref = ragged_prefill_case("mixed", G, 128, 2, DEV)
    b = _batch(seqs)
    for name in ("ragged_prefill", "ragged_prefill_gqa"):
        out = getattr(_ext(), name)(q, kp, vp, b.desc, b.max_qlen,
                                    b.max_kvlen)
        assert_within(out, ref["out"], ref["tol"], name)


def test_prefill_gqa_rejects_bad_arguments():
    """Built as in test_decode_gqa_rejects_bad_arguments: no bad call could
    index outside allocated memory even without the checks."""
    T, Hk, G, D, B, Smax = 6, 2, 3, 64, 4, 16
    z = lambda *shape: torch.zeros(*shape, device=DEV, dtype=BF)  # noqa: E731
    desc = torch.tensor([[2, 0, 5, 9], [0, 5, 1, 16]], device=DEV)
    good = dict(q=z(T, Hk * G, D), kp=z(B + 2, Smax, Hk, D)[:B],
                vp=z(B + 2, Smax, Hk, D)[:B], desc=desc, mq=5, mk=16, w=4)

    def call(**kw):
        a = {**good, **kw}
        return _ext().ragged_prefill_gqa(a["q"], a["kp"], a["vp"], a["desc"],
                                         a["mq"], a["mk"], a["w"])
    call()
    k1, wide = z(B + 2, Smax, 1, D)[:B], z(B, Smax, Hk, 256)
    long8 = torch.zeros(4, 8, dtype=torch.long, device=DEV)
    bad = {
        "G = 33": dict(q=z(T, 33, D), kp=k1, vp=k1),
        "window -1": dict(w=-1),
        "max_kvlen > Smax": dict(mk=Smax + 1),
        "max_qlen > max_kvlen": dict(mq=9, mk=8),
        "head_dim 256": dict(q=z(T, Hk * G, 256), kp=wide, vp=wide),
        "q dtype": dict(q=good["q"].float()),
        "desc int32": dict(desc=desc.int()),
        "kpool device": dict(kp=z(B + 2, Smax, Hk, D).cpu()[:B]),
        "q strided": dict(q=z(T, Hk * G, 2 * D)[..., :D]),
        "kpool strided": dict(kp=wide[..., :D]),
        "desc strided": dict(desc=long8[:2, ::2]),
        "desc width 3": dict(desc=long8[:, :3].contiguous()),
    }
    for name, kw in bad.items():
        with pytest.raises(RuntimeError):
            call(**kw)
            pytest.fail(f"'{name}' did not raise")


def _count(monkeypatch, calls, *names):
    for name in names:
        real = getattr(_ext(), name)
        monkeypatch.setattr(_ext(), name, lambda *a, _n=name, _r=real: (
            calls.append(_n), _r(*a))[1])


def test_prefill_gqa_dispatch(monkeypatch):
    import deepspeed_amd.ops.functional as Fops
    calls = []
    _count(monkeypatch, calls, "ragged_prefill", "ragged_prefill_gqa")
    monkeypatch.setattr(Fops, "_ragged_prefill_torch",
                        lambda *a, **k: pytest.fail("torch fallback ran"))
    for G, kw, window, want in ((4, {}, 0, "ragged_prefill"),
                                (4, {"window": 16}, 16, "ragged_prefill_gqa"),
                                (3, {}, 0, "ragged_prefill_gqa"),
                                (4, {"mfma": True}, 0, "ragged_prefill_gqa")):
        q, kp, vp, seqs, ref = band_case(G, 64, 2, window, DEV)
        out = Fops.ragged_prefill_attention(q, kp, vp, _batch(seqs), **kw)
        assert calls.pop() == want and not calls, (G, kw)
        assert_within(out, ref["out"], ref["tol"], f"G {G} {kw}")


@pytest.mark.parametrize("heads,window", [((6, 2), None), ((4, 2), 16)])
def test_prefill_gqa_engine_gpu(monkeypatch, heads, window):
    """test_decode_gqa_engine_gpu's model and criterion on the fused step;
    prompts past the window and past two chunks."""
    import deepspeed_amd.models.llama as llama
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine

    cfg = llama.LlamaConfig(hidden_size=64 * heads[0], intermediate_size=688,
                            num_hidden_layers=2, num_attention_heads=heads[0],
                            num_key_value_heads=heads[1], vocab_size=2048,
                            max_position_embeddings=512,
                            activation_checkpointing=False,
                            sliding_window=window)
    torch.manual_seed(0)
    model = llama.LlamaForCausalLM(cfg).to(DEV, BF).eval()
    torch.manual_seed(1)
    prompts = [torch.randint(0, 2000, (n,)) for n in (20, 40, 27, 70)]
    new = 8
    with torch.no_grad():
        refs = [greedy_no_cache(model, p.to(DEV), new) for p in prompts]
    calls = []
    _count(monkeypatch, calls, "ragged_prefill", "ragged_prefill_gqa")
    cb = ContinuousBatchingEngine(model, max_batch=2, prefill_chunk=16,
                                  prefill_budget=32, fused_step=True)
    rids = [cb.add_request(p, max_new_tokens=new) for p in prompts]
    out = cb.run()

    assert sorted(cb.free_slots) == [0, 1]
    assert not cb.running and not cb.pending and not cb.prefilling
    assert calls and set(calls) == {"ragged_prefill_gqa"}
    for rid, ref, p in zip(rids, refs, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
        agree = (out[rid].to(DEV) == ref).float().mean().item()
        assert agree >= 0.75, (rid, agree)
