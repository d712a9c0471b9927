#!/usr/bin/env python3
"""Which operand layout should the bf16 weight-gradient GEMM get?

dW[N,K] = dY^T X reduces over T tokens; X[T,K] and dY[T,N] are row-major, so
neither is contiguous along T. For the five dW shapes of the Llama-3-8B bench
(T = 4 x 4096) this times torch.mm in four operand arrangements

  a  dy.t() @ x          today's path
  b  dyT @ x             dyT [N,T] contiguous
  c  dy.t() @ xT.t()     xT [K,T] contiguous
  d  dyT @ xT.t()        both transposed

and the transposes themselves (ext.transpose_bf16 against
x.t().contiguous()), plus swiglu_fwd at [T, 14336] as the bandwidth gauge.
Each figure is the minimum over ROUNDS alternated rounds of CALLS calls,
every call between its own pair of device events; the spread is the largest
round-to-round difference of the per-round minima.

Every shape runs in a child process of its own under a time limit, and the
first one that fails ends the run. Results: profiles/README.md,
"Weight-gradient GEMMs in the fast layout".

Run on GPU: python tools/wgrad_probe.py            (all shapes)
            python tools/wgrad_probe.py --shape down
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T = 4 * 4096
# name -> (N, K) of dW
SHAPES = {
    "q_o": (4096, 4096),
    "k_v": (1024, 4096),
    "gate_up": (14336, 4096),
    "down": (4096, 14336),
    "lm_head": (128256, 4096),
}
ROUNDS = 3
CALLS = 34  # per round; 3 x 34 = 102 calls per figure
CHILD_LIMIT_S = 240


def time_alternated(fns):
    """fns: name -> callable. Returns name -> (min ms, spread ms)."""
    import torch
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            evs = []
            for _ in range(CALLS):
                s = torch.cuda.Event(enable_timing=True)
                e = torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                evs.append((s, e))
            torch.cuda.synchronize()
            per_round[name].append(min(s.elapsed_time(e) for s, e in evs))
    return {k: (min(v), max(v) - min(v)) for k, v in per_round.items()}


def run_shape(name):
    import torch
    from deepspeed_amd.ops.loader import get_ext
    ext = get_ext(required=True)
    n, k = SHAPES[name]
    torch.manual_seed(0)
    bf = torch.bfloat16
    x = torch.randn(T, k, device="cuda", dtype=bf)
    dy = torch.randn(T, n, device="cuda", dtype=bf)
    xt = ext.transpose_bf16(x)
    dyt = ext.transpose_bf16(dy)
    assert torch.equal(xt, x.t().contiguous())
    assert torch.equal(dyt, dy.t().contiguous())
    res = {"shape": name, "N": n, "K": k, "T": T}
    gemm = time_alternated({
        "a": lambda: torch.mm(dy.t(), x),
        "b": lambda: torch.mm(dyt, x),
        "c": lambda: torch.mm(dy.t(), xt.t()),
        "d": lambda: torch.mm(dyt, xt.t()),
    })
    tr = time_alternated({
        "tr_x": lambda: ext.transpose_bf16(x),
        "tr_dy": lambda: ext.transpose_bf16(dy),
        "torch_tr_dy": lambda: dy.t().contiguous(),
    })
    if name == "down":  # x is [T, 14336]: the size of the bandwidth target
        u = torch.randn_like(x)
        tr.update(time_alternated({"swiglu_fwd": lambda: ext.swiglu_fwd(x, u)}))
    flops = 2.0 * T * n * k
    for key, (ms, spread) in gemm.items():
        res[key] = {"ms": round(ms, 4), "spread_ms": round(spread, 4),
                    "pf_s": round(flops / ms / 1e12, 3)}
    nbytes = {"tr_x": 2 * x.numel() * 2, "tr_dy": 2 * dy.numel() * 2,
              "torch_tr_dy": 2 * dy.numel() * 2,
              "swiglu_fwd": 3 * x.numel() * 2}
    for key, (ms, spread) in tr.items():
        res[key] = {"ms": round(ms, 4), "spread_ms": round(spread, 4),
                    "tb_s": round(nbytes[key] / ms / 1e9, 3)}
    # GEMM plus the transposes that arrangement needs, measured kernel
    res["total_ms"] = {
        "a": res["a"]["ms"],
        "b": round(res["b"]["ms"] + res["tr_dy"]["ms"], 4),
        "c": round(res["c"]["ms"] + res["tr_x"]["ms"], 4),
        "d": round(res["d"]["ms"] + res["tr_dy"]["ms"] + res["tr_x"]["ms"],
                   4),
    }
    print("WGRAD " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default=None)
    args = ap.parse_args()
    if args.shape:
        run_shape(args.shape)
        return 0
    for name in SHAPES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__),
                                "--shape", name], timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {CHILD_LIMIT_S} s; stopping",
                  file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{name}: exit {r.returncode}; stopping", file=sys.stderr)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
