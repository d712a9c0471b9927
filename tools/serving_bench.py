#!/usr/bin/env python3
"""Continuous-batching decode throughput vs sequential generate.

SB_FUSED=1 runs the prompt-heavy workload instead: SB_NREQ prompts of
SB_PROMPT..SB_PROMPT+192 tokens, SB_NEW new tokens each, chunked prefill
(SB_CHUNK tokens per chunk, SB_BUDGET prompt tokens per step). The same
requests go through the budgeted engine twice -- one model forward per
chunk plus one per decode batch, then fused_step=True (one ragged forward
per step) -- each after a warm-up pass, and the tok/s and the number of
model forwards of both are printed.

SB_FUSED_KV=1 adds the `fused_kv_append=True` arm (one ragged_rope_append
launch per layer instead of eager per-row RoPE plus index_puts): a third
pass `fused_step=True, fused_kv_append=True` in the SB_FUSED workload, and
in the default workload a warmed pair of passes, default engine then
fused_kv_append, after the usual lines.

SB_KV_FP8=1 adds the fp8 KV pool arm (`kv_dtype="fp8"`, which needs
fused_kv_append): in either workload the bf16-pool engine with
fused_kv_append and the fp8-pool engine run back to back, SB_ROUNDS times
(default 3) after one warm-up pass each, and the generated tok/s of both are
printed per round and as median [min-max]. With SB_FUSED the pair is
`fused_step=True`; otherwise the default whole-prompt engine.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deepspeed_amd.inference.engine import InferenceEngine  # noqa: E402
from deepspeed_amd.inference.serving import \
    ContinuousBatchingEngine  # noqa: E402
from deepspeed_amd.models.llama import (LLAMA_CONFIGS,  # noqa: E402
                                        LlamaForCausalLM)

MODEL = os.environ.get("SB_MODEL", "llama-small")
NREQ = int(os.environ.get("SB_NREQ", 16))
NEW = int(os.environ.get("SB_NEW", 64))
BATCH = int(os.environ.get("SB_BATCH", 8))
# prompt-heavy workload (SB_FUSED=1)
FUSED = int(os.environ.get("SB_FUSED", 0))
FUSED_KV = int(os.environ.get("SB_FUSED_KV", 0))
KV_FP8 = int(os.environ.get("SB_KV_FP8", 0))
ROUNDS = int(os.environ.get("SB_ROUNDS", 3))
PROMPT = int(os.environ.get("SB_PROMPT", 256))
CHUNK = int(os.environ.get("SB_CHUNK", 64))
BUDGET = int(os.environ.get("SB_BUDGET", 256))


def _fp8_rounds(run, gtok):
    """`run(kv_dtype)` is one timed pass returning seconds. Warm both arms,
    then ROUNDS back-to-back pairs; generated tok/s as median [min-max]."""
    arms = (("bf16 pool", None), ("fp8 pool", "fp8"))
    for _, kv in arms:
        run(kv, warm=True)
    rates = {name: [] for name, _ in arms}
    for rnd in range(ROUNDS):
        for name, kv in arms:
            rates[name].append(gtok / run(kv, warm=False))
        print(f"round {rnd}: " + "  ".join(
            f"{name} {rates[name][-1]:8.1f} tok/s" for name, _ in arms))
    med = {}
    for name, _ in arms:
        r = sorted(rates[name])
        med[name] = r[len(r) // 2]
        print(f"+kv {name:9s}: {med[name]:8.1f} generated tok/s median "
              f"[{r[0]:.1f}-{r[-1]:.1f}] over {ROUNDS} rounds")
    print(f"fp8 pool / bf16 pool throughput: "
          f"{med['fp8 pool'] / med['bf16 pool']:.2f}x")


def _run_budgeted(model, prompts, fused, dev, fused_kv=False, kv_dtype=None):
    """One timed pass; returns (seconds, model forwards, engine steps)."""
    calls = [0]
    hook = model.register_forward_hook(
        lambda *a: calls.__setitem__(0, calls[0] + 1))
    cb = ContinuousBatchingEngine(model, max_batch=BATCH,
                                  prefill_chunk=CHUNK, prefill_budget=BUDGET,
                                  fused_step=fused, fused_kv_append=fused_kv,
                                  kv_dtype=kv_dtype)
    for p in prompts:
        cb.add_request(p, max_new_tokens=NEW)
    if dev == "cuda":
        torch.cuda.synchronize()
    t0 = time.time()
    steps = 0
    while cb.pending or cb.prefilling or cb.running:
        cb.step()
        steps += 1
    if dev == "cuda":
        torch.cuda.synchronize()
    dt = time.time() - t0
    hook.remove()
    cb.close()
    return dt, calls[0], steps


def main_fused(model, dev):
    vocab = model.cfg.vocab_size
    prompts = [torch.randint(0, vocab, (PROMPT + (i % 4) * 64,))
               for i in range(NREQ)]
    ptok = sum(len(p) for p in prompts)
    gtok = NREQ * NEW
    print(f"{MODEL}: {NREQ} reqs, prompts {PROMPT}..{PROMPT + 192} "
          f"({ptok} prompt tokens) + {NEW} new tokens each; batch {BATCH}, "
          f"chunk {CHUNK}, budget {BUDGET}")
    res = {}
    arms = [("unfused", False, False), ("fused", True, False)]
    if FUSED_KV:
        arms.append(("fused+kv", True, True))
    for name, fused, kv in arms:
        _run_budgeted(model, prompts[:BATCH], fused, dev, kv)  # warm-up
        dt, calls, steps = _run_budgeted(model, prompts, fused, dev, kv)
        res[name] = dt
        print(f"{name:8s}: {dt:6.2f} s  {gtok / dt:8.1f} generated tok/s  "
              f"{(ptok + gtok) / dt:9.1f} total tok/s  "
              f"{calls:5d} model forwards in {steps} steps")
    print(f"fused / unfused throughput: {res['unfused'] / res['fused']:.2f}x")
    if FUSED_KV:
        print("fused+kv / fused throughput: "
              f"{res['fused'] / res['fused+kv']:.2f}x")
    if KV_FP8:
        _fp8_rounds(lambda kv, warm: _run_budgeted(
            model, prompts[:BATCH] if warm else prompts, True, dev, True,
            kv)[0], gtok)


def _run_decode(model, prompts, dev, fused_kv, kv_dtype=None):
    """One timed pass of the default (whole-prompt prefill) engine."""
    cb = ContinuousBatchingEngine(model, max_batch=BATCH,
                                  fused_kv_append=fused_kv,
                                  kv_dtype=kv_dtype)
    if dev == "cuda":
        torch.cuda.synchronize()
    t0 = time.time()
    for p in prompts:
        cb.add_request(p, max_new_tokens=NEW)
    cb.run()
    if dev == "cuda":
        torch.cuda.synchronize()
    dt = time.time() - t0
    cb.close()
    return dt


def main():
    torch.manual_seed(0)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    dtype = torch.bfloat16 if dev == "cuda" else torch.float32
    model = LlamaForCausalLM(LLAMA_CONFIGS[MODEL]).to(dev, dtype).eval()
    if FUSED:
        return main_fused(model, dev)
    vocab = model.cfg.vocab_size
    prompts = [torch.randint(0, vocab, (32 + (i % 5) * 16,))
               for i in range(NREQ)]

    eng = InferenceEngine(model)
    # warm
    eng.generate(prompts[0].view(1, -1).to(dev), max_new_tokens=4)
    if dev == "cuda":
        torch.cuda.synchronize()
    t0 = time.time()
    for p in prompts:
        eng.generate(p.view(1, -1).to(dev), max_new_tokens=NEW)
    if dev == "cuda":
        torch.cuda.synchronize()
    seq_s = time.time() - t0

    cb = ContinuousBatchingEngine(model, max_batch=BATCH)
    t0 = time.time()
    for p in prompts:
        cb.add_request(p, max_new_tokens=NEW)
    cb.run()
    if dev == "cuda":
        torch.cuda.synchronize()
    cb_s = time.time() - t0

    tok = NREQ * NEW
    print(f"{MODEL}: {NREQ} reqs x {NEW} new tokens")
    print(f"sequential: {seq_s:6.2f} s  {tok / seq_s:8.1f} tok/s")
    print(f"continuous (batch {BATCH}): {cb_s:6.2f} s  "
          f"{tok / cb_s:8.1f} tok/s  ({seq_s / cb_s:.2f}x)")
    if FUSED_KV:
        # both arms warmed (the pass above warmed the default one)
        _run_decode(model, prompts[:BATCH], dev, True)
        res = {}
        for name, kv in (("continuous warm", False),
                         ("continuous +kv", True)):
            res[name] = dt = _run_decode(model, prompts, dev, kv)
            print(f"{name:15s}: {dt:6.2f} s  {tok / dt:8.1f} tok/s")
        print("+kv / warm throughput: "
              f"{res['continuous warm'] / res['continuous +kv']:.2f}x")
    if KV_FP8:
        _fp8_rounds(lambda kv, warm: _run_decode(
            model, prompts[:BATCH] if warm else prompts, dev, True, kv), tok)


if __name__ == "__main__":
    main()
