"""Time the MoE routing, unfused torch index ops against the HIP routing path
(`fused_routing=True`), on one MI355X, in one process, alternating the two.

  1. routing alone at the Mixtral-8x7B layer shape (4 x 4096 tokens, M 4096,
     E 8, k 2, capacity factor 1.25, bf16): gate + dispatch + combine with the
     experts replaced by identity, forward and forward + backward;
  2. the two row kernels alone, achieved bytes/s against the HBM peak (bytes
     computed from the shapes: rows read + rows written);
  3. kernel launches of one routing forward + backward, from the profiler;
  4. one full MixtralDecoderLayer forward + backward, flag off against on.

Times are device events around a synchronised window; medians and ranges
over `--reps` alternating repetitions after `--warmup`.

    python profiles/moe_routing_timing.py [--reps 20] [--small]
"""
import argparse
import copy
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from deepspeed_amd.models.mixtral import MIXTRAL_CONFIGS, MixtralDecoderLayer
from deepspeed_amd.moe.layer import MoE
from deepspeed_amd.ops import functional as Fops
from deepspeed_amd.ops.functional import build_rope_cache

HBM_PEAK = 8.0e12       # MI355X HBM3E, bytes/s
DEV = "cuda:0"


def timed(fn):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def compare(name, fns, reps, warmup):
    """fns: {label: callable}; alternate them, print median (min .. max)."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    for k, v in ms.items():
        print(f"{name:34s} {k:8s} median {statistics.median(v):8.3f} ms "
              f"({min(v):.3f} .. {max(v):.3f})")
    return {k: statistics.median(v) for k, v in ms.items()}


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events()
               if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true",
                    help="toy sizes, to rehearse the script")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("needs an MI355X: nothing is timed without one")
    torch.manual_seed(0)
    B, T = (4, 4096) if not args.small else (2, 64)
    cfg = copy.deepcopy(MIXTRAL_CONFIGS["mixtral-tiny" if args.small
                                        else "mixtral-8x7b"])
    M, E, k = cfg.hidden_size, cfg.num_experts, cfg.top_k
    S = B * T

    # ---- 1. routing alone, identity experts
    plain = MoE(M, torch.nn.Identity(), num_experts=E, k=k,
                capacity_factor=cfg.capacity_factor).to(DEV)
    fused = copy.deepcopy(plain)
    fused.deepspeed_moe.fused_routing = True
    x = torch.randn(B, T, M, device=DEV).to(torch.bfloat16)
    dy = torch.randn_like(x)

    def fwd(m):
        with torch.no_grad():
            return m(x)[0]

    def fwd_bwd(m):
        xi = x.detach().requires_grad_(True)
        out, l_aux, _ = m(xi)
        torch.autograd.backward([out, l_aux], [dy, torch.ones_like(l_aux)])

    print(f"shape: S={S} M={M} E={E} k={k} bf16")
    compare("routing forward", {"unfused": lambda: fwd(plain),
                                "fused": lambda: fwd(fused)},
            args.reps, args.warmup)
    compare("routing forward+backward",
            {"unfused": lambda: fwd_bwd(plain),
             "fused": lambda: fwd_bwd(fused)}, args.reps, args.warmup)

    # ---- 2. the row kernels alone
    C = int(cfg.capacity_factor * k * S / E)
    logits = plain.deepspeed_moe.gate.wg(x.reshape(S, M).float()).detach()
    _, idx, w, loc, keep, counts, slot = Fops.moe_gate_topk(logits, k, C)
    kept = int(keep.sum())
    x2 = x.reshape(S, M)
    row = M * x.element_size()
    disp = Fops.moe_dispatch(x2, idx, loc, keep, slot, E, C)
    t = compare("gate (3 launches)",
                {"fused": lambda: Fops.moe_gate_topk(logits, k, C)},
                args.reps, args.warmup)
    t = compare("moe_scatter_rows (dispatch)",
                {"fused": lambda: Fops.moe_dispatch(x2, idx, loc, keep, slot,
                                                    E, C)},
                args.reps, args.warmup)
    nbytes = (kept + E * C) * row
    print(f"  {nbytes / 1e6:.0f} MB moved, {nbytes / t['fused'] / 1e6:.0f} "
          f"GB/s, {100 * nbytes / (t['fused'] * 1e-3) / HBM_PEAK:.0f} % of "
          f"HBM peak")
    t = compare("moe_gather_rows (combine)",
                {"fused": lambda: Fops.moe_combine(disp, idx, loc, keep, w)},
                args.reps, args.warmup)
    nbytes = (kept + S) * row
    print(f"  {nbytes / 1e6:.0f} MB moved, {nbytes / t['fused'] / 1e6:.0f} "
          f"GB/s, {100 * nbytes / (t['fused'] * 1e-3) / HBM_PEAK:.0f} % of "
          f"HBM peak")

    # ---- 3. launches per routing forward + backward
    try:
        print(f"launches, routing forward+backward: unfused "
              f"{launches(lambda: fwd_bwd(plain))}, fused "
              f"{launches(lambda: fwd_bwd(fused))}")
    except Exception as e:          # profiler unavailable: say so
        print(f"launches: not measured ({type(e).__name__}: {e})")
    del plain, fused, disp

    # ---- 4. one decoder layer, real experts
    cfg.activation_checkpointing = False
    layer = MixtralDecoderLayer(cfg).to(DEV).to(torch.bfloat16)
    layer.block_sparse_moe.deepspeed_moe.gate.wg.float()
    cos, sin = build_rope_cache(T, cfg.head_dim, cfg.rope_theta, device=DEV)
    moe = layer.block_sparse_moe.deepspeed_moe

    def layer_step(flag):
        moe.fused_routing = flag
        layer.zero_grad(set_to_none=True)
        xi = x.detach().requires_grad_(True)
        out, l_aux = layer(xi, cos, sin)
        torch.autograd.backward([out, l_aux], [dy, torch.ones_like(l_aux)])

    compare("decoder layer forward+backward",
            {"unfused": lambda: layer_step(False),
             "fused": lambda: layer_step(True)},
            max(5, args.reps // 2), args.warmup)


if __name__ == "__main__":
    main()
