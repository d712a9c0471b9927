#!/usr/bin/env python3
"""Decode latency: eager KV-cache loop vs hipGraph-captured step.

`--kernels [--window W]`: the two slot-pool decode kernels, `ragged_decode` and
`ragged_decode_gqa`, timed alternately with device events over G x context x
batch; median, min..max and the K/V bytes the call must read over the median
(bf16 pool, 2 * 2 * Hk * D bytes per attended position).

`--kernels --fp8 [--window W]`: the same over pools made with `kv_quantize`:
`ragged_decode_fp8` (no window only) and `ragged_decode_gqa_fp8`, 2 * Hk *
(D + 4) bytes per attended position, with `ragged_decode_gqa` on the bf16 pool
of the same shape as the yardstick.

`--prefill-kernels`: the two fused-step kernels, `ragged_prefill` and
`ragged_prefill_gqa`, the same way over a decode-only step (64 rows at context
8192), a chunk step (8 x 256 new tokens over a 4096-token prefix), both mixed,
and the chunk step with window 4096 at prefix 32768 (new kernel only);
8 kv heads, D 128, G 4, 8 and 7 (new kernel only).

`--prefill-kernels --fp8`: the same steps over pools made with `kv_quantize`:
`ragged_prefill_fp8` (G 4 and 8, no window) and `ragged_prefill_gqa_fp8`, with
`ragged_prefill_gqa` on the bf16 pool of the same shape as the yardstick."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402


def _time_ms(fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True),
           torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


def kernels(window, fp8=False, reps=30, rounds=5):
    from deepspeed_amd.ops.loader import get_ext
    ext = get_ext(required=True)
    D, Hk, dev = 128, 8, "cuda:0"
    print("G ctx batch kernel median_ms min_ms max_ms TB/s")
    for G in (4, 8):
        for ctx in (512, 8192, 32768):
            for n in (1, 8, 64):
                g = torch.Generator(device=dev).manual_seed(ctx + n)
                kp = torch.randn(n, ctx, Hk, D, device=dev, generator=g) \
                    .bfloat16()
                vp = torch.randn(n, ctx, Hk, D, device=dev, generator=g) \
                    .bfloat16()
                q = torch.randn(n, 1, G * Hk, D, device=dev, generator=g) \
                    .bfloat16()
                rows = torch.arange(n, device=dev)
                lens = torch.full((n,), ctx, device=dev)
                arms = {"ragged_decode_gqa": lambda: ext.ragged_decode_gqa(
                    q, kp, vp, rows, lens, window, ctx)}
                span = min(window, ctx) if window else ctx
                nbytes = {"ragged_decode_gqa": 2 * 2 * Hk * D * span * n}
                if fp8:
                    from deepspeed_amd.ops.functional import kv_quantize
                    (kc, ks), (vc, vs) = kv_quantize(kp), kv_quantize(vp)
                    arms["ragged_decode_gqa_fp8"] = \
                        lambda: ext.ragged_decode_gqa_fp8(
                            q, kc, vc, ks, vs, rows, lens, window, ctx)
                    if not window:
                        arms["ragged_decode_fp8"] = \
                            lambda: ext.ragged_decode_fp8(q, kc, vc, ks, vs,
                                                          rows, lens)
                    for k in list(arms)[1:]:
                        nbytes[k] = 2 * Hk * (D + 4) * span * n
                    new = arms["ragged_decode_gqa_fp8"]().float()
                    for k, f in arms.items():
                        if k != "ragged_decode_gqa_fp8":
                            d = (new - f().float()).abs().max().item()
                            print(f"# G={G} ctx={ctx} n={n} max |gqa_fp8 - "
                                  f"{k}| = {d:.3e}")
                elif not window:
                    arms["ragged_decode"] = lambda: ext.ragged_decode(
                        q, kp, vp, rows, lens)
                    a, b = (f().float() for f in arms.values())
                    print(f"# G={G} ctx={ctx} n={n} max |new - old| = "
                          f"{(a - b).abs().max().item():.3e}")
                times = {k: [] for k in arms}
                for f in arms.values():
                    _time_ms(f, 5)               # warm-up
                for _ in range(rounds):          # alternate the arms
                    for k, f in arms.items():
                        times[k] += _time_ms(f, reps)
                for k, t in times.items():
                    t.sort()
                    med = t[len(t) // 2]
                    nb = nbytes.get(k, nbytes["ragged_decode_gqa"])
                    print(f"{G} {ctx} {n} {k} {med:.4f} {t[0]:.4f} "
                          f"{t[-1]:.4f} {nb / med / 1e9:.3f}", flush=True)
                del kp, vp, arms


def prefill_kernels(fp8=False, reps=20, rounds=3):
    """The fused-step kernels, `ragged_prefill` (G 4 and 8, no window) and
    `ragged_prefill_gqa`, alternately over the same ragged steps; with `fp8`
    `ragged_prefill_fp8` (G 4 and 8, no window), `ragged_prefill_gqa_fp8`
    and `ragged_prefill_gqa` on the bf16 pool."""
    from deepspeed_amd.inference.ragged_batch import RaggedBatch
    from deepspeed_amd.ops.loader import get_ext
    ext = get_ext(required=True)
    D, Hk, dev = 128, 8, "cuda:0"
    dec = [(1, 8192)] * 64
    chunk = [(256, 4096 + 256)] * 8
    steps = (("decode", dec, 0), ("chunk", chunk, 0),
             ("mixed", dec + chunk, 0),
             ("chunk_w4096", [(256, 32768 + 256)] * 8, 4096))
    print("G step kernel median_ms min_ms max_ms")
    for name, pairs, window in steps:
        n, smax = len(pairs), max(kv for _, kv in pairs)
        g = torch.Generator(device=dev).manual_seed(n + smax)
        kp = torch.randn(n, smax, Hk, D, device=dev, generator=g).bfloat16()
        vp = torch.randn(n, smax, Hk, D, device=dev, generator=g).bfloat16()
        seqs, t = [], 0
        for slot, (ql, kv) in enumerate(pairs):
            seqs.append((slot, t, ql, kv))
            t += ql
        b = RaggedBatch(seqs, n, smax, dev)
        if fp8:
            from deepspeed_amd.ops.functional import kv_quantize
            (kc, ks), (vc, vs) = kv_quantize(kp), kv_quantize(vp)
        for G in ((4, 8) if window else (4, 8, 7)):
            q = torch.randn(t, G * Hk, D, device=dev, generator=g).bfloat16()
            arms = {"ragged_prefill_gqa": lambda: ext.ragged_prefill_gqa(
                q, kp, vp, b.desc, b.max_qlen, b.max_kvlen, window)}
            if fp8:
                arms["ragged_prefill_gqa_fp8"] = \
                    lambda: ext.ragged_prefill_gqa_fp8(
                        q, kc, vc, ks, vs, b.desc, b.max_qlen, b.max_kvlen,
                        window)
                if not window and G != 7:
                    arms["ragged_prefill_fp8"] = \
                        lambda: ext.ragged_prefill_fp8(
                            q, kc, vc, ks, vs, b.desc, b.max_qlen,
                            b.max_kvlen)
                new = arms["ragged_prefill_gqa_fp8"]().float()
                for k, f in arms.items():
                    if k != "ragged_prefill_gqa_fp8":
                        d = (new - f().float()).abs().max().item()
                        print(f"# G={G} {name} max |gqa_fp8 - {k}| = {d:.3e}")
            elif not window and G != 7:
                arms["ragged_prefill"] = lambda: ext.ragged_prefill(
                    q, kp, vp, b.desc, b.max_qlen, b.max_kvlen)
                x, y = (f().float() for f in arms.values())
                print(f"# G={G} {name} max |new - old| = "
                      f"{(x - y).abs().max().item():.3e}")
            times = {k: [] for k in arms}
            for f in arms.values():
                _time_ms(f, 5)                   # warm-up
            for _ in range(rounds):              # alternate the arms
                for k, f in arms.items():
                    times[k] += _time_ms(f, reps)
            for k, ts in times.items():
                ts.sort()
                print(f"{G} {name} {k} {ts[len(ts) // 2]:.4f} {ts[0]:.4f} "
                      f"{ts[-1]:.4f}", flush=True)
        del kp, vp


def main():
    if "--prefill-kernels" in sys.argv:
        return prefill_kernels(fp8="--fp8" in sys.argv)
    if "--kernels" in sys.argv:
        w = sys.argv.index("--window") if "--window" in sys.argv else None
        return kernels(int(sys.argv[w + 1]) if w is not None else 0,
                       fp8="--fp8" in sys.argv)
    model_name = sys.argv[1] if len(sys.argv) > 1 else "llama3-8b"
    n_tok = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    import deepspeed_amd
    from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
    cfg = LLAMA_CONFIGS[model_name]
    torch.manual_seed(0)
    with torch.device("cuda:0"):
        model = LlamaForCausalLM(cfg)
    engine = deepspeed_amd.init_inference(model, config={})
    ids = torch.randint(0, cfg.vocab_size, (1, 64), device="cuda:0")

    # warmup both paths
    engine.generate(ids, max_new_tokens=4)
    engine.generate_hipgraph(ids, max_new_tokens=4)
    torch.cuda.synchronize()

    t0 = time.time()
    engine.generate(ids, max_new_tokens=n_tok)
    torch.cuda.synchronize()
    t_eager = time.time() - t0

    t0 = time.time()
    engine.generate_hipgraph(ids, max_new_tokens=n_tok)
    torch.cuda.synchronize()
    t_graph = time.time() - t0

    print(f"model={model_name} tokens={n_tok}")
    print(f"eager decode:    {t_eager/n_tok*1000:7.2f} ms/token "
          f"({n_tok/t_eager:6.1f} tok/s)")
    print(f"hipGraph decode: {t_graph/n_tok*1000:7.2f} ms/token "
          f"({n_tok/t_graph:6.1f} tok/s)  "
          f"speedup {t_eager/t_graph:.2f}x")


if __name__ == "__main__":
    main()
