"""ZeRO stage 3: partitioned parameters + gradients + optimizer states.

Parity: reference `runtime/zero/stage3.py:149` (DeepSpeedZeroOptimizer_Stage3),
`runtime/zero/parameter_offload.py:130` (hook installer),
`runtime/zero/partitioned_param_coordinator.py:73` (prefetch coordinator).

MI355X-first redesign (not a translation):
- Per-param contiguous all-gather inside an RCCL coalescing group (see
  stage3_params.py) — zero reassembly copies.
- Gradients reduce-scatter per-param (coalesced) into flat fp32 shard
  accumulators every micro-step; full grads freed immediately.
- Optimizer states live in flat fp32 "sub-group" slabs sized for cache
  residency; the fused HIP AdamW walks them as one multi-tensor launch.
- Prefetch: module-order trace recorded on step 0, replayed with an
  element-budget lookahead (prefetch_bucket_size) so all-gathers overlap
  compute on the same RCCL stream without CPU-side stalls.
"""
from collections import OrderedDict

import torch

from ... import comm as dist
from ...utils.logging import log_dist, logger
from ..loss_scaler import CreateLossScaler
from .stage3_params import (ZeroParamStatus, all_gather_params,
                            convert_to_zero_param, free_param, is_zero_param)

ALIGN = 64


def _pad_to(n, m):
    return (n + m - 1) // m * m


class SubGroup:
    """Flat fp32 master + flat bf16 shard slab + grad accumulator.

    The 16-bit shards (`p.ds_tensor`) are re-pointed to views of one flat
    bf16 buffer so the fused Adam kernel writes updated bf16 shards in the
    same pass as the fp32 update (no separate cast+copy over 16 GB)."""

    __slots__ = ("params", "offsets", "master32", "grad32", "flat16",
                 "flat16_cpu", "grad_stage", "group_idx", "numel", "offload",
                 "param_offload", "dtype16", "store_first", "_written",
                 "_stale")

    def __init__(self, params, offsets, numel, group_idx, device,
                 offload=False, param_offload=False, pin_opt=True,
                 pin_param=True):
        self.params = params
        self.offsets = offsets
        self.numel = numel
        self.group_idx = group_idx
        self.offload = offload
        self.param_offload = param_offload
        dtype16 = params[0].ds_tensor.dtype if params else torch.bfloat16
        self.dtype16 = dtype16
        # pinning giant slabs costs ~1 GB/s at registration: configs
        # (offload_*.pin_memory) choose; 70B-scale host tiers run pageable
        pin = torch.cuda.is_available()
        host = torch.device("cpu")
        state_dev = host if offload else device
        # param offload (ZeRO-Infinity tier): the 16-bit shard slab itself
        # lives in (optionally pinned) host memory; fetches stage it H2D
        # on the gather stream (stage3_params._shard_on_device)
        slab_dev = host if param_offload else device
        self.flat16 = torch.empty(numel, dtype=dtype16, device=slab_dev,
                                  pin_memory=pin and param_offload
                                  and pin_param)
        self.master32 = torch.empty(numel, dtype=torch.float32,
                                    device=state_dev,
                                    pin_memory=pin and offload and pin_opt)
        for p in params:
            off = offsets[p]
            n = p.ds_shard_numel
            self.flat16[off:off + n].copy_(p.ds_tensor)
            p.ds_tensor = self.flat16[off:off + n]
            self.master32[off:off + n].copy_(p.ds_tensor.float())
        self.master32 = self.master32.detach().requires_grad_(True)
        self.grad32 = torch.zeros(numel, dtype=torch.float32,
                                  device=state_dev,
                                  pin_memory=pin and offload and pin_opt)
        if offload:
            if param_offload:
                # the host slab IS the 16-bit output buffer: the fused CPU
                # Adam writes it in place, nothing to publish H2D
                self.flat16_cpu = self.flat16
            else:
                # pinned staging: bf16 shard out (H2D)
                self.flat16_cpu = torch.empty(numel, dtype=dtype16,
                                              device=host,
                                              pin_memory=pin and pin_opt)
            self.grad_stage = torch.empty(numel, dtype=dtype16, device=host,
                                          pin_memory=pin and pin_opt)
        else:
            self.flat16_cpu = None
            self.grad_stage = None
        # Store-first accumulation (device-resident grads only): instead of
        # zero-filling grad32 after every step and adding onto the zeros,
        # the first accumulate of a parameter in a window overwrites its
        # range. `_written`: ranges valid in this window. `_stale`: ranges
        # still holding the previous window's data; `complete_grads` zeroes
        # the ones the window never wrote before anything reads grad32.
        # The offsets tile [0, numel) with whole-parameter ranges, so there
        # is no padding between ranges; within a range, elements past the
        # reduced shard's length are never written and keep the zero from
        # the allocation above.
        self.store_first = not offload
        self._written = set()
        self._stale = set()

    def grad_shard_view(self, p):
        off = self.offsets[p]
        return self.grad32[off:off + p.ds_shard_numel]

    def accumulate_grad(self, p, shard16_gpu):
        """shard16_gpu: this rank's reduced gradient shard (device)."""
        dst = self.grad_shard_view(p)[:shard16_gpu.numel()]
        if self.offload:
            off = self.offsets[p]
            stage = self.grad_stage[off:off + shard16_gpu.numel()]
            stage.copy_(shard16_gpu, non_blocking=True)
            if shard16_gpu.is_cuda:
                torch.cuda.synchronize()
            dst.add_(stage.float())
            return
        overwrite = self.store_first and p not in self._written
        self._written.add(p)
        if shard16_gpu.is_cuda and shard16_gpu.dtype == torch.bfloat16:
            from ...ops.loader import get_ext
            get_ext(required=True).accum_bf16_to_f32(dst, shard16_gpu, 1.0,
                                                     overwrite)
        elif overwrite:
            dst.copy_(shard16_gpu)
        else:
            dst.add_(shard16_gpu.float())

    def complete_grads(self):
        """Make every range of grad32 valid for a reader: zero the ranges
        that hold the previous window's data and were not written since."""
        for p in self._stale:
            if p not in self._written:
                self.grad_shard_view(p).zero_()
        self._stale.clear()

    def clear_grads(self):
        """Start a new accumulation window."""
        if self.store_first:
            self._stale |= self._written
        else:
            self.grad32.zero_()
            self._stale.clear()
        self._written.clear()

    def copy_master_to_shards(self):
        if self.offload:
            self.flat16_cpu.copy_(self.master32.detach().to(self.dtype16)
                                  if self.flat16_cpu.dtype != torch.float32
                                  else self.master32.detach())
            if self.flat16_cpu is not self.flat16:
                self.flat16.copy_(self.flat16_cpu, non_blocking=True)
        else:
            # cross-device copy_ handles dtype+D2H in one pass when the
            # param slab is host-resident (param offload, GPU optimizer)
            self.flat16.copy_(self.master32.detach())

    def publish_flat16(self):
        """After a fused CPU-Adam step wrote flat16_cpu, push H2D (no-op
        when the slab is host-resident: flat16_cpu IS flat16)."""
        if self.flat16_cpu is not self.flat16:
            self.flat16.copy_(self.flat16_cpu, non_blocking=True)


class ZeroStage3Optimizer:
    def __init__(self,
                 init_optimizer,
                 module,
                 engine=None,
                 dp_process_group=None,
                 reduce_bucket_size=int(5e8),
                 prefetch_bucket_size=int(5e7),
                 param_persistence_threshold=int(1e5),
                 model_persistence_threshold=int(1e14),
                 max_live_parameters=int(1e9),
                 max_reuse_distance=int(1e9),
                 sub_group_size=int(1e9),
                 overlap_comm=True,
                 offload_optimizer=None,
                 offload_param=None,
                 zero_quantized_weights=False,
                 zero_quantized_gradients=False,
                 zero_quantized_nontrainable_weights=False,
                 leaf_module_names=None,
                 clip_grad=0.0,
                 static_loss_scale=1.0,
                 dynamic_loss_scale=False,
                 dynamic_loss_args=None,
                 dtype=torch.bfloat16,
                 gradient_accumulation_steps=1,
                 replica_group=None):
        self.optimizer = init_optimizer
        self.module = module
        self.dp_group = dp_process_group
        # MiCS: params shard over dp_group (sub-world); grads additionally
        # average across replica_group (ref runtime/zero/mics.py)
        self.replica_group = replica_group
        self.replica_world = (dist.get_world_size(replica_group)
                              if replica_group is not None else 1)
        self.world = dist.get_world_size(self.dp_group)
        self.rank = dist.get_rank(self.dp_group)
        self.dtype = dtype
        self.clip_grad = clip_grad
        self.reduce_bucket_size = int(reduce_bucket_size)
        self.prefetch_bucket_size = int(prefetch_bucket_size)
        self.persist_threshold = int(param_persistence_threshold)
        self.model_persistence_threshold = int(model_persistence_threshold)
        self.max_live_parameters = int(max_live_parameters)
        self.max_reuse_distance = int(max_reuse_distance)
        self.sub_group_size = int(sub_group_size)
        self.gradient_accumulation_steps = gradient_accumulation_steps
        self.micro_step = 0
        self.overlap_comm = overlap_comm
        # ZeRO++ qwZ (ref coalesced qwZ path): int8 blockwise shard
        # gathers + fp16 scales — halves all-gather bytes over xGMI
        self.quantized_weights = bool(zero_quantized_weights)
        self.quantized_gradients = bool(zero_quantized_gradients)
        self.quantized_nontrainable = bool(
            zero_quantized_nontrainable_weights)
        self.leaf_module_names = list(leaf_module_names or [])

        self.device = (torch.device("cuda", torch.cuda.current_device())
                       if torch.cuda.is_available() else torch.device("cpu"))
        self.offload_device = getattr(offload_optimizer, "device", "none") \
            if offload_optimizer is not None else "none"
        self.offload_optimizer = self.offload_device in ("cpu", "nvme")
        # partial offload (ref offload_optimizer.ratio / zero_partial_
        # offload): keep (1-ratio) of the optimizer-state elements on the
        # GPU with a fused device Adam, offload the rest
        self.offload_ratio = float(getattr(offload_optimizer, "ratio",
                                           1.0)) \
            if offload_optimizer is not None else 1.0
        # ZeRO-Infinity parameter tier (ref partitioned_param_swapper.py:37):
        # cpu => 16-bit shard slabs live in pinned host RAM; nvme => slabs
        # additionally spill to O_DIRECT files with an LRU host budget
        self.param_offload_device = getattr(offload_param, "device", "none") \
            if offload_param is not None else "none"
        self._pin_opt = getattr(offload_optimizer, "pin_memory", True) \
            if offload_optimizer is not None else True
        self._pin_param = getattr(offload_param, "pin_memory", True) \
            if offload_param is not None else True
        self.param_offload = self.param_offload_device in ("cpu", "nvme")
        self.param_swapper = None
        if self.param_offload_device == "nvme":
            from ..swap_tensor.param_swapper import ParamSlabSwapper
            import os as _os
            ppath = getattr(offload_param, "nvme_path", None) \
                or "/tmp/dsamd_nvme_swap"
            ppath = _os.path.join(ppath, f"param_rank{self.rank}")
            self.param_swapper = ParamSlabSwapper(
                ppath,
                max_in_cpu=getattr(offload_param, "max_in_cpu", int(1e9)),
                pin_memory=getattr(offload_param, "pin_memory", True))
        self.nvme_swapper = None
        if self.offload_device == "nvme":
            from ..swap_tensor.optimizer_swapper import OptimizerStateSwapper
            import os as _os
            nvme_path = getattr(offload_optimizer, "nvme_path", None) \
                or "/tmp/dsamd_nvme_swap"
            nvme_path = _os.path.join(nvme_path, f"rank{self.rank}")
            self.nvme_swapper = OptimizerStateSwapper(nvme_path)

        self.loss_scaler = CreateLossScaler(dtype, static_loss_scale,
                                            dynamic_loss_scale,
                                            dynamic_loss_args)
        self.overflow = False

        # MoE expert params partition/reduce over their expert-DP group
        # (the replicas of the same expert), like the stage-1/2 buckets.
        from ...comm import groups as grp
        self._expert_pg = {}
        for p in module.parameters():
            gn = getattr(p, "group_name", None)
            if gn is None:
                continue
            if gn not in self._expert_pg:
                if gn not in grp.get_expert_parallel_group_dict():
                    try:  # groups are lazily built on first forward
                        grp.create_expert_and_data_parallel(
                            int(gn.rsplit("_", 1)[1]))
                    except (ValueError, AssertionError):
                        pass
                try:
                    self._expert_pg[gn] = \
                        grp.get_expert_data_parallel_group(gn)
                except KeyError:
                    self._expert_pg[gn] = None
        if self._expert_pg and self.replica_world > 1:
            raise NotImplementedError("MiCS + expert parallelism")
        self._shard_module_params()
        if self.quantized_nontrainable:
            # frozen params (LoRA bases etc.) keep only an int8 blockwise
            # residency copy — halves their memory (ref
            # zero_quantized_nontrainable_weights)
            from .stage3_params import quantize_frozen_param
            nq = 0
            for p in self._all_params:
                if not p.requires_grad and not p.ds_persist \
                        and p.ds_tensor is not None:
                    quantize_frozen_param(p)
                    nq += 1
            log_dist(f"ZeRO-3: {nq} frozen params int8-quantized",
                     ranks=[0])
        self._build_sub_groups()
        if self.param_swapper is not None:
            for i, sg in enumerate(self.sub_groups):
                self.param_swapper.register(i, sg)
                for p in sg.params:
                    p.ds_swap = (self.param_swapper, i)
            self._sg_index = {id(sg): i for i, sg in
                              enumerate(self.sub_groups)}
        if self.nvme_swapper is not None:
            self._init_nvme_state()
        self._gather_persistent_params()
        self._install_module_hooks()
        self._install_grad_hooks()

        # dedicated HIP streams: all-gathers (prefetch/fetch) and grad
        # reduce-scatters overlap backward/forward compute on the default
        # stream (ref stage3.py reduce_and_partition_stream /
        # __allgather_stream)
        import os as _os
        use_streams = torch.cuda.is_available() and self.overlap_comm \
            and (self.world > 1
                 or _os.environ.get("DSAMD_FORCE_STREAMS") == "1")
        self.ag_stream = torch.cuda.Stream() if use_streams else None
        self.rs_stream = torch.cuda.Stream() if use_streams else None
        self._rs_refs = []  # tensors owned by in-flight reduce work

        # reduction state
        self._ipg_params = []
        self._ipg_numel = 0
        self._reduce_works = []

        # trace / prefetch state
        self._trace = []            # module order recorded on first forward
        self._trace_complete = False
        self._trace_pos = 0
        self._inflight = {}         # module -> AllGatherHandle
        # hybrid-engine generation holds ALL params gathered: fetch/free
        # per submodule is pure churn there (and collectives/frees inside
        # hipGraph capture), so the hooks can be paused
        self._hooks_paused = False
        # partition-traffic counters (ref partitioned_param_profiler)
        self._partition_stats = {"fetches": 0, "prefetch_hits": 0,
                                 "demand_gathers": 0, "gathered_numel": 0,
                                 "releases": 0}

        self._global_grad_norm = 0.0
        self._cached_norm_sq = None
        # opt-in cross-rank sanity asserts (DSAMD_SANITY=1): verify every
        # rank reduces the same params in the same order
        self._sanity = _os.environ.get("DSAMD_SANITY") == "1"
        log_dist(
            f"ZeRO-3: {sum(p.ds_numel for p in self._all_params)/1e9:.2f}B "
            f"params, {len(self.sub_groups)} sub-groups, world {self.world}",
            ranks=[0])

    # ---------------------------------------------------------------- setup
    def _shard_module_params(self):
        """Convert any unsharded params; move buffers to device."""
        params = list(self.module.parameters())
        bcast_group = None if self.replica_world > 1 else self.dp_group
        bcast_world = dist.get_world_size(bcast_group) \
            if dist.is_initialized() else 1
        src = (dist.get_global_rank(bcast_group, 0)
               if bcast_group is not None and bcast_world > 1 else 0)
        # param offload: shard straight to host pinned memory so a big
        # model never stages its full shards through HBM at init
        shard_dev = torch.device("cpu") if self.param_offload else self.device
        for p in params:
            if not is_zero_param(p):
                p.data = p.data.to(self.device, self.dtype)
                gn = getattr(p, "group_name", None)
                pg = self._expert_pg.get(gn) if gn is not None else None
                if pg is not None:
                    # replicate only across expert-DP (distinct experts
                    # stay rank-distinct), then shard over that group
                    if dist.get_world_size(pg) > 1:
                        dist.broadcast(p.data,
                                       dist.get_global_rank(pg, 0),
                                       group=pg)
                    convert_to_zero_param(p, pg, shard_dev, self.dtype,
                                          self.persist_threshold)
                    continue
                if bcast_world > 1:
                    dist.broadcast(p.data, src, group=bcast_group)
                convert_to_zero_param(p, self.dp_group, shard_dev,
                                      self.dtype, self.persist_threshold)
        for b in self.module.buffers():
            b.data = b.data.to(self.device)
        # dedupe (tied weights appear once in .parameters() already)
        self._all_params = [p for p in self.module.parameters()]
        for i, p in enumerate(self._all_params):
            p.ds_param_index = i
        # model_persistence_threshold (ref partition_parameters.py:1264):
        # cap TOTAL persisted elements per partition — stop persisting
        # once the cumulative budget is spent
        budget = self.model_persistence_threshold // max(self.world, 1)
        persisted = 0
        for p in self._all_params:
            if p.ds_persist:
                if persisted + p.ds_numel > budget:
                    p.ds_persist = False
                else:
                    persisted += p.ds_numel

    def _build_sub_groups(self):
        """Pack param shards into flat fp32 sub-groups per optimizer group."""
        param_to_group = {}
        for gi, g in enumerate(self.optimizer.param_groups):
            for p in g["params"]:
                param_to_group[p] = gi
        self.sub_groups = []
        for gi in range(len(self.optimizer.param_groups)):
            gparams = [p for p in self._all_params
                       if param_to_group.get(p, 0) == gi and p.requires_grad]
            cur, offsets, numel = [], OrderedDict(), 0
            for p in gparams:
                if numel >= self.sub_group_size and cur:
                    self.sub_groups.append(
                        SubGroup(cur, offsets, numel, gi, self.device,
                                 offload=self._sg_offload(numel),
                                 param_offload=self.param_offload,
                                 pin_opt=self._pin_opt,
                                 pin_param=self._pin_param))
                    cur, offsets, numel = [], OrderedDict(), 0
                offsets[p] = numel
                cur.append(p)
                numel += p.ds_shard_numel
            if cur:
                self.sub_groups.append(
                    SubGroup(cur, offsets, numel, gi, self.device,
                             offload=self._sg_offload(numel),
                             param_offload=self.param_offload,
                             pin_opt=self._pin_opt,
                             pin_param=self._pin_param))
        self.param_to_subgroup = {}
        for sg in self.sub_groups:
            for p in sg.params:
                self.param_to_subgroup[p] = sg
        for gi, g in enumerate(self.optimizer.param_groups):
            g["params"] = [sg.master32 for sg in self.sub_groups
                           if sg.group_idx == gi]

    def _sg_offload(self, numel):
        """Partial offload: greedily offload sub-groups while the
        offloaded fraction trails `ratio` — converges to ratio of total
        elements without knowing the total upfront."""
        if not self.offload_optimizer:
            return False
        if self.offload_ratio >= 1.0:
            return True
        if self.offload_ratio <= 0.0:
            return False
        if not hasattr(self, "_off_elems"):
            self._off_elems = 0
            self._tot_elems = 0
        behind = self._off_elems <= self.offload_ratio * self._tot_elems
        self._tot_elems += numel
        if behind:
            self._off_elems += numel
            return True
        return False

    def _init_nvme_state(self):
        """Write initial fp32 masters to NVMe; drop resident copies."""
        for i, sg in enumerate(self.sub_groups):
            buf = self.nvme_swapper._buffer(i, "master", sg.numel)
            buf.copy_(sg.master32.detach().cpu())
            # materialize zero state files too
            self.nvme_swapper._buffer(i, "exp_avg", sg.numel)
            self.nvme_swapper._buffer(i, "exp_avg_sq", sg.numel)
            self.nvme_swapper.swap_out(i)
            self.nvme_swapper.release_buffers(i)
            sg.master32 = None  # lives on NVMe now
        for g in self.optimizer.param_groups:
            g["params"] = []

    def _nvme_step(self, combined_scale):
        """Per-sub-group: swap in -> host AdamW -> swap out -> publish."""
        from ...ops.loader import get_ext
        ext = get_ext(required=False)
        for g in self.optimizer.param_groups:
            g["step"] = g.get("step", 0) + 1
        for i, sg in enumerate(self.sub_groups):
            if self.param_swapper is not None:
                self.param_swapper.ensure_resident(i)
            group = self.optimizer.param_groups[sg.group_idx]
            beta1, beta2 = group.get("betas", (0.9, 0.999))
            master, ea, eas = self.nvme_swapper.swap_in(i, sg.numel)
            grad = sg.grad32 if not sg.grad32.is_cuda else sg.grad32.cpu()
            if ext is not None:
                ext.cpu_adam_step(master, grad, ea, eas,
                                  sg.flat16_cpu, group["lr"], beta1, beta2,
                                  group.get("eps", 1e-8), group["step"], 1, 1,
                                  group.get("weight_decay", 0.0),
                                  1.0 / combined_scale)
            else:
                g32 = grad * (1.0 / combined_scale)
                step = group["step"]
                bc1 = 1 - beta1**step
                bc2 = 1 - beta2**step
                master.mul_(1.0 - group["lr"] *
                            group.get("weight_decay", 0.0))
                ea.mul_(beta1).add_(g32, alpha=1 - beta1)
                eas.mul_(beta2).addcmul_(g32, g32, value=1 - beta2)
                denom = (eas / bc2).sqrt().add_(group.get("eps", 1e-8))
                master.addcdiv_(ea, denom, value=-group["lr"] / bc1)
                sg.flat16_cpu.copy_(master.to(sg.flat16_cpu.dtype))
            self.nvme_swapper.swap_out(i)
            self.nvme_swapper.release_buffers(i)
            sg.publish_flat16()
            if self.param_swapper is not None:
                self.param_swapper.mark_dirty(i)
                self.param_swapper.evict_to_budget()

    def _flush_ipg_quant(self, params, world, pg):
        """ZeRO++ qgZ (single-node form, ref coalesced_collectives.py:31
        all_to_all_quant_reduce): grads quantize to int8 blockwise BEFORE
        the wire; one all-to-all moves each rank's shard-chunks (half the
        reduce-scatter bytes), then dequant + sum + average locally."""
        from .stage3_params import dequantize_gathered, quantize_shard
        for p in params:
            sn = p.ds_shard_numel
            if sn * world == p.ds_numel:
                padded = p.grad.reshape(-1)
            else:
                padded = torch.empty(sn * world, dtype=p.grad.dtype,
                                     device=p.grad.device)
                padded[:p.ds_numel].copy_(p.grad.reshape(-1))
                padded[p.ds_numel:].zero_()
            q, sc = quantize_shard(padded)          # int8 [world*sn]
            qr = torch.empty_like(q)
            sr = torch.empty_like(sc)
            dist.all_to_all_single(qr, q, group=pg)
            dist.all_to_all_single(sr, sc, group=pg)
            # received: world chunks of MY shard -> dequant, sum, average
            deq = dequantize_gathered(qr, sr, world, torch.float32)
            shard = deq.view(world, sn).sum(0).div_(world)
            sg = self.param_to_subgroup[p]
            if self.replica_world > 1:
                from .stage_1_and_2 import _avg_op
                op = _avg_op(self.replica_world, shard)
                dist.all_reduce(shard, op=op, group=self.replica_group)
            sg.accumulate_grad(p, shard.to(p.grad.dtype))
            p.grad = None

    def _partial_offload_step(self, combined):
        """Mixed placement: host sub-groups step through the (CPU) base
        optimizer, device-resident sub-groups through a dedicated fused
        device Adam (ref zero_partial_offload semantics)."""
        if not hasattr(self, "_gpu_adam"):
            from ...ops.adam import FusedAdam
            g0 = self.optimizer.param_groups[0]
            dev_masters = [sg.master32 for sg in self.sub_groups
                           if not sg.offload]
            self._gpu_adam = FusedAdam(
                dev_masters, lr=g0["lr"],
                betas=g0.get("betas", (0.9, 0.999)),
                eps=g0.get("eps", 1e-8),
                weight_decay=g0.get("weight_decay", 0.0)) \
                if dev_masters else None
        if self._gpu_adam is not None:
            # follow any LR schedule applied to the base optimizer
            self._gpu_adam.param_groups[0]["lr"] = \
                self.optimizer.param_groups[0]["lr"]
        for which, opt in (("host", self.optimizer),
                           ("dev", self._gpu_adam)):
            if opt is None:
                continue
            fused = hasattr(opt, "set_grad_scale")
            sel = [sg for sg in self.sub_groups
                   if sg.offload == (which == "host")]
            if not sel:
                continue
            if fused:
                opt.set_grad_scale(1.0 / combined)
                opt.set_fused_out16(
                    {sg.master32: (sg.flat16_cpu if sg.offload
                                   else sg.flat16) for sg in sel})
            elif combined != 1.0:
                for sg in sel:
                    sg.grad32.mul_(1.0 / combined)
            for sg in sel:
                sg.master32.grad = sg.grad32
            opt.step()
            for sg in sel:
                sg.master32.grad = None
                if not fused:
                    sg.copy_master_to_shards()
                elif sg.offload:
                    sg.publish_flat16()
            if fused:
                opt.set_grad_scale(1.0)
                opt.set_fused_out16({})

    def _param_offload_step(self, combined, fused):
        """NVMe param tier: per-sub-group step under the host-RAM budget.
        Each slab is made resident, updated (fused CPU/GPU Adam writes the
        16-bit host slab in the same pass), marked dirty, then eligible
        for eviction back to its O_DIRECT file."""
        bases = [g.get("step", 0) for g in self.optimizer.param_groups]
        if fused:
            self.optimizer.set_grad_scale(1.0 / combined)
        for i, sg in enumerate(self.sub_groups):
            self.param_swapper.ensure_resident(i)
            # optimizer.step() bumps each group's step counter once per
            # call; pin it so N sub-group calls count as ONE step
            for g, b in zip(self.optimizer.param_groups, bases):
                g["step"] = b
            if fused:
                self.optimizer.set_fused_out16(
                    {sg.master32: (sg.flat16_cpu if sg.offload
                                   else sg.flat16)})
            elif combined != 1.0:
                sg.grad32.mul_(1.0 / combined)
            sg.master32.grad = sg.grad32
            self.optimizer.step()
            sg.master32.grad = None
            if not fused:
                sg.copy_master_to_shards()
            elif sg.offload:
                sg.publish_flat16()
            self.param_swapper.mark_dirty(i)
            self.param_swapper.evict_to_budget()
        if fused:
            self.optimizer.set_grad_scale(1.0)
            self.optimizer.set_fused_out16({})

    @torch.no_grad()
    def _muon_step(self, combined):
        """Distributed Muon inside ZeRO-3 (ref stage3.py:1619
        _apply_distributed_muon_update). Momentum stays SHARDED (the
        momentum update is elementwise, so it commutes with sharding);
        only Newton-Schulz needs the full 2-D matrix: one all-gather per
        2-D param rebuilds the nesterov-effective update, every rank runs
        NS on it (replicated, deterministic), and applies its own shard
        of U to its master slice. Non-2D params take the sharded AdamW
        path."""
        from ...ops.muon import zeropower_via_newtonschulz5
        inv = 1.0 / combined
        if not hasattr(self, "_muon_state"):
            self._muon_state = {}
        for sg in self.sub_groups:
            group = self.optimizer.param_groups[sg.group_idx]
            group["step"] = group.get("step", 0) + 1
            mom = group["momentum"]
            for p in sg.params:
                sn = p.ds_shard_numel
                off = sg.offsets[p]
                gs = sg.grad32[off:off + sn]
                master = sg.master32[off:off + sn]
                st = self._muon_state.setdefault(p.ds_id, {})
                use_muon = len(p.ds_shape) == 2 and min(p.ds_shape) > 1
                if use_muon:
                    g = gs * inv
                    buf = st.setdefault("momentum_buffer",
                                        torch.zeros_like(gs))
                    buf.mul_(mom).add_(g)
                    eff = g.add(buf, alpha=mom) if group["nesterov"]                         else buf.clone()
                    pg = self._param_pg(p)
                    world = dist.get_world_size(pg)
                    eff_dev = eff.to(self.device)
                    if world > 1:
                        full = torch.empty(world * sn, dtype=eff_dev.dtype,
                                           device=eff_dev.device)
                        dist.all_gather_into_tensor(full, eff_dev, group=pg)
                    else:
                        full = eff_dev
                    mat = full[:p.ds_numel].view(p.ds_shape)
                    u = zeropower_via_newtonschulz5(
                        mat, group["ns_steps"]).reshape(-1)
                    rank = dist.get_rank(pg)
                    start = rank * sn
                    end = min(start + sn, p.ds_numel)
                    scale = max(1.0, p.ds_shape[0] / p.ds_shape[1]) ** 0.5
                    if group["weight_decay"]:
                        master.mul_(1 - group["lr"] *
                                    group["weight_decay"])
                    if end > start:
                        master[:end - start].add_(
                            u[start:end].to(master.device),
                            alpha=-group["lr"] * scale)
                else:
                    g = gs * inv
                    if "exp_avg" not in st:
                        st["exp_avg"] = torch.zeros_like(g)
                        st["exp_avg_sq"] = torch.zeros_like(g)
                    b1, b2 = group["adamw_betas"]
                    t = group["step"]
                    m, v = st["exp_avg"], st["exp_avg_sq"]
                    m.mul_(b1).add_(g, alpha=1 - b1)
                    v.mul_(b2).addcmul_(g, g, value=1 - b2)
                    denom = (v / (1 - b2 ** t)).sqrt_()                         .add_(group["adamw_eps"])
                    master.addcdiv_(m, denom,
                                    value=-group["adamw_lr"] /
                                    (1 - b1 ** t))
            if self.param_swapper is not None:
                i = self._sg_index[id(sg)]
                self.param_swapper.ensure_resident(i)
                sg.copy_master_to_shards()
                self.param_swapper.mark_dirty(i)
                self.param_swapper.evict_to_budget()
            else:
                sg.copy_master_to_shards()

    def _param_pg(self, p):
        return getattr(p, "ds_group", None) or self.dp_group

    def _gather_grouped(self, params, async_op=True, stream=None):
        """Launch one gather per distinct partitioning group (dense
        params share dp_group; expert params use their expert-DP group).
        Returns a handle with .wait()."""
        if self.param_swapper is not None:
            # NVMe param tier: bring evicted shard slabs back to pinned
            # host RAM before the H2D + all-gather; the whole working set
            # of this fetch is protected from eviction
            need_ids = []
            for pm in params:
                sg = self.param_to_subgroup.get(pm)
                if sg is not None and self._sg_index[id(sg)] not in need_ids:
                    need_ids.append(self._sg_index[id(sg)])
            for i in need_ids:
                self.param_swapper.ensure_resident(i, exclude=need_ids)
        by_pg = {}
        for p in params:
            by_pg.setdefault(id(self._param_pg(p)), []).append(p)
        handles = [all_gather_params(ps, self._param_pg(ps[0]),
                                     async_op=async_op, stream=stream,
                                     quantized=self.quantized_weights)
                   for ps in by_pg.values()]
        if len(handles) == 1:
            return handles[0]

        class _Multi:
            def __init__(self, hs):
                self._hs = hs
                self.params = [p for h in hs for p in h.params]

            def wait(self):
                for h in self._hs:
                    h.wait()
        return _Multi(handles)

    def _gather_persistent_params(self):
        persist = [p for p in self._all_params if p.ds_persist]
        if persist:
            self._gather_grouped(persist, async_op=False).wait()

    # ------------------------------------------------------------- hooks
    def _leaf_module_classes(self):
        """Class names configured as ZeRO leaf modules (ref
        runtime/zero/leaf_module_config.py): their whole parameter
        subtree gathers/releases as ONE unit — e.g. an MoE expert bank
        whose data-dependent submodule order would defeat trace
        prefetch."""
        return set(getattr(self, "leaf_module_names", []) or [])

    def _install_module_hooks(self):
        """fetch/release hooks on every module owning direct params (or
        registered external ones, see register_external_parameter).
        Modules whose class name is in leaf_module_names hook at their
        own level with their ENTIRE subtree's params; descendants are
        skipped."""
        self._module_hooks = []
        leaf_names = self._leaf_module_classes()
        leaf_descendants = set()
        for mod in self.module.modules():
            if type(mod).__name__ in leaf_names:
                for sub in mod.modules():
                    if sub is not mod:
                        leaf_descendants.add(id(sub))
        for mod in self.module.modules():
            if id(mod) in leaf_descendants:
                continue
            if type(mod).__name__ in leaf_names:
                direct = [p for p in mod.parameters(recurse=True)
                          if is_zero_param(p)]
            else:
                direct = [p for p in mod.parameters(recurse=False)
                          if is_zero_param(p)]
            external = [p for p in getattr(mod, "_ds_external_params", [])
                        if is_zero_param(p)]
            if not direct and not external:
                continue
            mod._ds_direct_params = direct + external
            self._module_hooks.append(mod.register_forward_pre_hook(
                self._pre_forward_hook))
            self._module_hooks.append(mod.register_forward_hook(
                self._post_forward_hook))
            self._module_hooks.append(mod.register_full_backward_pre_hook(
                self._pre_backward_hook))
            self._module_hooks.append(mod.register_full_backward_hook(
                self._post_backward_hook))
        # root hook: reset trace replay position each step
        self._module_hooks.append(self.module.register_forward_pre_hook(
            self._root_pre_forward))

    def _root_pre_forward(self, mod, inputs):
        self._trace_pos = 0
        if self._trace and not self._trace_complete:
            self._trace_complete = True
            self._compute_reuse_keep()

    def _compute_reuse_keep(self):
        """max_reuse_distance (ref zero/config.py:238, coordinator
        release-by-reuse-distance): a module whose backward re-fetch is
        closer than the threshold (in parameter elements walked through
        the tail of forward + head of backward) keeps its params gathered
        across the turn instead of releasing + re-gathering."""
        sizes = [sum(p.ds_numel for p in m._ds_direct_params)
                 for m in self._trace]
        suffix = 0
        for i in range(len(self._trace) - 1, -1, -1):
            # distance fwd-exit(i) -> bwd-entry(i): rest of forward plus
            # the same modules walked back = 2 * suffix(i+1)
            self._trace[i]._ds_keep_for_backward =                 2 * suffix < self.max_reuse_distance
            suffix += sizes[i]

    # -- forward path
    def _pre_forward_hook(self, mod, inputs):
        if self._hooks_paused:
            return
        self.fetch_sub_module(mod, forward=True)

    def _post_forward_hook(self, mod, inputs, output):
        if self._hooks_paused:
            return
        self.release_sub_module(mod)

    # -- backward path
    def _pre_backward_hook(self, mod, grad_output):
        self.fetch_sub_module(mod, forward=False)

    def _post_backward_hook(self, mod, grad_input, grad_output):
        # NOTE: for modules whose inputs don't require grad (the first layer)
        # this hook fires BEFORE the module's internal backward nodes run, so
        # it must not free data. Actual freeing happens per-param in
        # _on_grad_ready (post-accumulate-grad == module backward complete).
        for p in mod._ds_direct_params:
            p.ds_active_sub_modules.discard(id(mod))

    def fetch_sub_module(self, mod, forward=True):
        params = mod._ds_direct_params
        st = self._partition_stats
        st["fetches"] += 1
        for p in params:
            p.ds_active_sub_modules.add(id(mod))
        # record trace on first iteration
        if forward and not self._trace_complete:
            self._trace.append(mod)
        h = self._inflight.pop(mod, None)
        if h is not None:
            st["prefetch_hits"] += 1
            h.wait()
        need = [p for p in params
                if p.ds_status == ZeroParamStatus.NOT_AVAILABLE]
        if need:
            st["demand_gathers"] += 1
            st["gathered_numel"] += sum(p.ds_numel for p in need)
            self._gather_grouped(need,
                              stream=self.ag_stream).wait()
        # tied params may be INFLIGHT under another module's handle
        pending = [p for p in params
                   if p.ds_status == ZeroParamStatus.INFLIGHT]
        if pending:
            for key, handle in list(self._inflight.items()):
                if any(p in handle.params for p in pending):
                    handle.wait()
                    self._inflight.pop(key, None)
        for p in params:
            assert p.ds_status == ZeroParamStatus.AVAILABLE, \
                f"param {p.ds_id} not available after fetch"
        if self._trace_complete:
            self._prefetch(forward=forward, current_mod=mod)

    def _prefetch(self, forward=True, current_mod=None):
        """Launch lookahead all-gathers along the recorded trace.

        Forward walks the trace ahead of _trace_pos; backward walks it in
        reverse starting just before the current module (backward re-fetch
        order is the reverse of the forward trace).
        """
        budget = self.prefetch_bucket_size
        # max_live_parameters (ref zero/config.py:238): cap the gathered
        # working set — prefetch pauses when live + in-flight exceeds it
        live = sum(p.ds_numel for p in self._all_params
                   if p.ds_status != ZeroParamStatus.NOT_AVAILABLE
                   and not p.ds_persist)
        budget = min(budget, max(0, self.max_live_parameters - live))
        n = len(self._trace)
        launched = 0
        if forward:
            pos = self._trace_pos
            step = 1
        else:
            if not hasattr(self, "_trace_index"):
                self._trace_index = {id(m): i
                                     for i, m in enumerate(self._trace)}
            pos = self._trace_index.get(id(current_mod), 0) - 1
            step = -1
        while 0 <= pos < n and budget > 0:
            mod = self._trace[pos]
            pos += step
            if mod in self._inflight:
                continue
            need = [p for p in mod._ds_direct_params
                    if p.ds_status == ZeroParamStatus.NOT_AVAILABLE]
            if not need:
                continue
            budget -= sum(p.ds_numel for p in need)
            self._inflight[mod] = self._gather_grouped(need,
                                                    stream=self.ag_stream)
            launched += 1
            if launched >= 8:
                break
        if forward:
            self._trace_pos = min(max(pos, 0), n)

    def release_sub_module(self, mod):
        keep = getattr(mod, "_ds_keep_for_backward", False)
        for p in mod._ds_direct_params:
            p.ds_active_sub_modules.discard(id(mod))
            if not keep and not p.ds_active_sub_modules \
                    and not p.ds_persist:
                self._partition_stats["releases"] += 1
                free_param(p)

    def partition_stats(self):
        """Fetch/prefetch/release counters since construction (role of
        ref zero/partitioned_param_profiler.py). prefetch_hits /
        demand_gathers shows how much the trace-replay prefetch covers;
        gathered_numel is total elements pulled on demand."""
        return dict(self._partition_stats)

    def _install_grad_hooks(self):
        self._grad_hooks = []
        for p in self._all_params:
            if p.requires_grad:
                self._grad_hooks.append(
                    p.register_post_accumulate_grad_hook(self._on_grad_ready))

    # --------------------------------------------------------- grad reduce
    def _on_grad_ready(self, p):
        self._ipg_params.append(p)
        self._ipg_numel += p.ds_numel
        # grad finalized => this param's backward consumers have run; safe to
        # drop the gathered weight now (backward-release point).
        if not p.ds_active_sub_modules and not p.ds_persist:
            free_param(p)
        if self._ipg_numel >= self.reduce_bucket_size:
            self._flush_ipg()

    def _flush_ipg(self):
        if not self._ipg_params:
            return
        params = self._ipg_params
        self._ipg_params = []
        self._ipg_numel = 0
        if self._sanity:
            from ..utils import assert_ints_same_as_other_ranks
            assert_ints_same_as_other_ranks(
                [p.ds_id for p in params], group=self.dp_group,
                tag="ipg_flush")
        by_pg = {}
        for p in params:
            by_pg.setdefault(id(self._param_pg(p)), []).append(p)
        if self.rs_stream is not None:
            # grads were produced on the default stream
            self.rs_stream.wait_stream(torch.cuda.current_stream())
            for p in params:
                if p.grad is not None:
                    p.grad.record_stream(self.rs_stream)
            with torch.cuda.stream(self.rs_stream):
                for ps in by_pg.values():
                    pg = self._param_pg(ps[0])
                    self._flush_ipg_body(ps, dist.get_world_size(pg), pg)
            return
        for ps in by_pg.values():
            pg = self._param_pg(ps[0])
            self._flush_ipg_body(ps, dist.get_world_size(pg), pg)

    def _flush_ipg_body(self, params, world, pg=None):
        if pg is None:
            pg = self.dp_group
        use_coalescing = (torch.cuda.is_available() and world > 1
                          and len(params) > 1)
        shards = []
        if world == 1:
            for p in params:
                sg = self.param_to_subgroup[p]
                g = p.grad.reshape(-1)
                if self.replica_world > 1:
                    from .stage_1_and_2 import _avg_op
                    op = _avg_op(self.replica_world, g)
                    dist.all_reduce(g, op=op, group=self.replica_group)
                sg.accumulate_grad(p, g)
                p.grad = None
            return
        if self.quantized_gradients:
            self._flush_ipg_quant(params, world, pg)
            return
        from .stage_1_and_2 import _avg_op
        inputs = []
        for p in params:
            shard_numel = p.ds_shard_numel
            if shard_numel * world == p.ds_numel:
                # aligned param: reduce-scatter the autograd grad in place
                padded = p.grad.reshape(-1)
            else:
                padded = torch.empty(shard_numel * world, dtype=p.grad.dtype,
                                     device=p.grad.device)
                padded[:p.ds_numel].copy_(p.grad.reshape(-1))
                padded[p.ds_numel:].zero_()
            inputs.append(padded)
            shards.append(torch.empty(shard_numel, dtype=p.grad.dtype,
                                      device=p.grad.device))
            p.grad = None
        if use_coalescing:
            try:
                from torch.distributed.distributed_c10d import \
                    _coalescing_manager
                from .stage_1_and_2 import _premul_avg_op
                op = _premul_avg_op(world) if inputs[0].is_cuda else None
                if op is None:
                    # no on-wire averaging: pre-divide EVERY input in the
                    # coalescing group, not just the first
                    if world > 1:
                        for inp in inputs:
                            inp.div_(world)
                    op = dist.ReduceOp.SUM
                with _coalescing_manager(pg, self.device,
                                         async_ops=True) as cm:
                    for out, inp in zip(shards, inputs):
                        dist.reduce_scatter_tensor(out, inp, op=op,
                                                   group=pg)
                cm.wait()
            except Exception as e:
                from .stage3_params import _COALESCE_OK  # noqa: F401
                import deepspeed_amd.runtime.zero.stage3_params as s3p
                s3p._COALESCE_OK = False
                logger.warning(f"coalesced reduce-scatter failed ({e}); "
                               "falling back to per-param calls")
                use_coalescing = False
        if not use_coalescing:
            for out, inp in zip(shards, inputs):
                op = _avg_op(world, inp)
                dist.reduce_scatter_tensor(out, inp, op=op,
                                           group=pg)
        if self.replica_world > 1:
            from .stage_1_and_2 import _avg_op
            for shard in shards:
                op = _avg_op(self.replica_world, shard)
                dist.all_reduce(shard, op=op, group=self.replica_group)
        for p, shard in zip(params, shards):
            sg = self.param_to_subgroup[p]
            sg.accumulate_grad(p, shard)

    # -------------------------------------------------------------- train
    def backward(self, loss, retain_graph=False):
        self.micro_step += 1
        self.loss_scaler.backward(loss.float(), retain_graph=retain_graph)
        self._flush_ipg()

    def is_gradient_accumulation_boundary(self):
        return self.micro_step % self.gradient_accumulation_steps == 0

    def _grad_norm_sq(self):
        """One pass over the fp32 grad slabs: squared L2 norm (double),
        all-reduced over DP. Serves BOTH the overflow check (inf/nan in any
        grad makes the squared sum non-finite) and grad clipping — the
        separate grad32.sum() scan the fp16 path used to do is folded in."""
        self._complete_grads()
        grads = [sg.grad32 for sg in self.sub_groups]
        if grads and grads[0].is_cuda:
            from ...ops.loader import get_ext
            total_sq = get_ext(required=True).l2norm_sq(grads).double()
        else:
            total_sq = torch.zeros(1, dtype=torch.float64)
            for g in grads:
                s = g.double()
                total_sq += torch.dot(s, s)
        total_sq = total_sq.reshape(1)
        if dist.is_initialized():
            total_sq = total_sq.to(self.device)
            dist.all_reduce(total_sq, group=self.dp_group)
        return total_sq

    def has_overflow(self):
        total_sq = self._cached_norm_sq if self._cached_norm_sq is not None \
            else self._grad_norm_sq()
        self._cached_norm_sq = total_sq
        return not bool(torch.isfinite(total_sq).item())

    def _combined_scale(self):
        """loss_scale x clip coefficient; folded into the Adam kernel as
        grad_scale = 1/combined (zero extra passes over the 32 GB shards).
        Reuses the norm pass the fp16 overflow check already did."""
        scale = self.loss_scaler.loss_scale
        combined = scale
        if self.clip_grad > 0.0:
            total_sq = self._cached_norm_sq \
                if self._cached_norm_sq is not None else self._grad_norm_sq()
            norm = total_sq.sqrt().item() / scale
            self._global_grad_norm = norm
            clip = norm / self.clip_grad
            if clip > 1.0:
                combined = scale * clip
        return combined

    def _sync_comm_streams(self):
        if self.rs_stream is not None:
            torch.cuda.current_stream().wait_stream(self.rs_stream)
        if self.ag_stream is not None:
            torch.cuda.current_stream().wait_stream(self.ag_stream)
        self._rs_refs = []

    def _drain_inflight(self):
        """Consume leftover prefetch handles (e.g. frozen-param modules)
        so no pre-step gathered copy survives the optimizer update."""
        for mod, h in list(self._inflight.items()):
            h.wait()
            for p in h.params:
                if not p.ds_persist:
                    free_param(p)
        self._inflight.clear()

    def step(self, closure=None):
        assert closure is None
        self._flush_ipg()
        self._sync_comm_streams()
        self._drain_inflight()
        self._complete_grads()
        self._cached_norm_sq = None  # one norm pass per step, shared below

        if self.dtype == torch.float16:
            self.overflow = self.has_overflow()
            self.loss_scaler.update_scale(self.overflow)
            if self.overflow:
                log_dist("OVERFLOW: skipping step, new scale "
                         f"{self.loss_scaler.loss_scale}", ranks=[0])
                self._clear_grads()
                return

        combined = self._combined_scale()

        if self.nvme_swapper is not None:
            self._nvme_step(combined)
            self._clear_grads()
            self._refresh_persistent_params()
            return

        from ...ops.muon import Muon as _Muon
        if isinstance(self.optimizer, _Muon):
            self._muon_step(combined)
            self._clear_grads()
            self._refresh_persistent_params()
            return

        fused = hasattr(self.optimizer, "set_grad_scale")
        if getattr(self, "offload_ratio", 1.0) < 1.0 \
                and self.offload_optimizer:
            if self.param_swapper is not None:
                raise NotImplementedError(
                    "offload_optimizer.ratio < 1 with offload_param nvme "
                    "is unsupported: use ratio 1.0 (full offload) with "
                    "the NVMe parameter tier")
            self._partial_offload_step(combined)
            self._clear_grads()
            self._refresh_persistent_params()
            return
        if self.param_swapper is not None:
            self._param_offload_step(combined, fused)
            self._clear_grads()
            self._refresh_persistent_params()
            return
        if fused:
            self.optimizer.set_grad_scale(1.0 / combined)
            self.optimizer.set_fused_out16(
                {sg.master32: (sg.flat16_cpu if sg.offload else sg.flat16)
                 for sg in self.sub_groups})
        elif combined != 1.0:
            for sg in self.sub_groups:
                sg.grad32.mul_(1.0 / combined)

        for sg in self.sub_groups:
            sg.master32.grad = sg.grad32
        self.optimizer.step()
        for sg in self.sub_groups:
            sg.master32.grad = None
            if not fused:
                sg.copy_master_to_shards()
            elif sg.offload:
                sg.publish_flat16()
        if fused:
            self.optimizer.set_grad_scale(1.0)
            self.optimizer.set_fused_out16({})
        self._clear_grads()
        self._refresh_persistent_params()

    def _refresh_persistent_params(self):
        persist = [p for p in self._all_params if p.ds_persist]
        for p in persist:
            p.ds_status = ZeroParamStatus.NOT_AVAILABLE
        if persist:
            self._gather_grouped(persist, async_op=False).wait()

    def _clear_grads(self):
        # device-resident sub-groups start a store-first window (no fill);
        # host-resident ones are zero-filled as before
        for sg in self.sub_groups:
            sg.clear_grads()

    def _set_store_first(self, enabled):
        """Private switch (tests): False restores fill-then-add."""
        self._complete_grads()
        for sg in self.sub_groups:
            sg.store_first = bool(enabled) and not sg.offload

    def _complete_grads(self):
        """Call before anything reads grad32: ranges no accumulate wrote
        in this window read as zero, never as the previous window's data."""
        for sg in self.sub_groups:
            sg.complete_grads()

    def zero_grad(self, set_to_none=True):
        pass

    # -------------------------------------------------------------- state
    @property
    def loss_scale(self):
        return self.loss_scaler.loss_scale

    def get_global_grad_norm(self):
        return self._global_grad_norm

    @property
    def param_groups(self):
        return self.optimizer.param_groups

    def shard_layout(self):
        names = {id(p): n for n, p in self.module.named_parameters()}
        subgroups = []
        for i, sg in enumerate(self.sub_groups):
            subgroups.append({
                "group_idx": sg.group_idx,
                "numel": sg.numel,
                # 6th element: the param's SHARD world — expert params
                # partition over the (smaller) expert-DP group, so
                # offline reassembly must concatenate only that group's
                # ranks (stride ep = world // shard_world)
                "params": [(names.get(id(p), f"param_{p.ds_id}"),
                            sg.offsets[p], p.ds_shard_numel, p.ds_numel,
                            list(p.ds_shape),
                            dist.get_world_size(p.ds_group))
                           for p in sg.params],
            })
        return {"stage": 3, "world": self.world, "kind": "subgroup",
                "subgroups": subgroups}

    def state_dict(self):
        if self.nvme_swapper is not None:
            # masters + Adam state live on NVMe: read them back so the
            # checkpoint is self-contained (resume works without the
            # original swap files)
            masters, eas, eass = [], [], []
            for i, sg in enumerate(self.sub_groups):
                m, ea, eas_ = self.nvme_swapper.swap_in(i, sg.numel)
                masters.append(m.clone())
                eas.append(ea.clone())
                eass.append(eas_.clone())
                self.nvme_swapper.release_buffers(i)
            return {
                "loss_scaler": self.loss_scaler,
                "base_optimizer_state": self.optimizer.state_dict(),
                "fp32_flat_groups": masters,
                "nvme_exp_avg": eas,
                "nvme_exp_avg_sq": eass,
                "param_shapes": self._param_shapes(),
                "zero_stage": 3,
                "partition_count": self.world,
                "shard_layout": self.shard_layout(),
            }
        sd = {
            "loss_scaler": self.loss_scaler,
            "base_optimizer_state": self.optimizer.state_dict(),
            "fp32_flat_groups": [sg.master32 for sg in self.sub_groups],
            "param_shapes": self._param_shapes(),
            "zero_stage": 3,
            "partition_count": self.world,
            "shard_layout": self.shard_layout(),
        }
        if getattr(self, "_muon_state", None):
            # distributed-Muon momentum/Adam shards (keyed by ds_id)
            sd["muon_state"] = {
                k: {n: v for n, v in st.items()}
                for k, st in self._muon_state.items()}
        return sd

    def _param_shapes(self):
        """name -> full shape, in module order (for zero_to_fp32)."""
        shapes = OrderedDict()
        pmap = {id(p): n for n, p in self.module.named_parameters()}
        for sg in self.sub_groups:
            for p in sg.params:
                shapes[pmap.get(id(p), f"param_{p.ds_id}")] = {
                    "shape": p.ds_shape, "numel": p.ds_numel,
                    "shard_numel": p.ds_shard_numel,
                    "subgroup_offset": sg.offsets[p]}
        return shapes

    def load_state_dict(self, sd, load_optimizer_states=True):
        if "loss_scaler" in sd:
            self.loss_scaler = sd["loss_scaler"]
        if load_optimizer_states and "base_optimizer_state" in sd:
            self.optimizer.load_state_dict(sd["base_optimizer_state"])
        if load_optimizer_states and "muon_state" in sd:
            self._muon_state = {k: dict(st)
                                for k, st in sd["muon_state"].items()}
        saved = sd.get("fp32_flat_groups", [])
        assert len(saved) == len(self.sub_groups)
        if self.nvme_swapper is not None:
            eas = sd.get("nvme_exp_avg")
            eass = sd.get("nvme_exp_avg_sq")
            for i, (sg, m) in enumerate(zip(self.sub_groups, saved)):
                if self.param_swapper is not None:
                    self.param_swapper.ensure_resident(i)
                mb, eab, easb = self.nvme_swapper.swap_in(i, sg.numel)
                mb.copy_(m.cpu())
                if eas is not None:
                    eab.copy_(eas[i].cpu())
                    easb.copy_(eass[i].cpu())
                sg.flat16_cpu.copy_(mb.to(sg.flat16_cpu.dtype))
                self.nvme_swapper.swap_out(i)
                self.nvme_swapper.release_buffers(i)
                sg.publish_flat16()
                if self.param_swapper is not None:
                    self.param_swapper.mark_dirty(i)
                    self.param_swapper.evict_to_budget()
            self._refresh_persistent_params()
            return
        for i, (sg, s) in enumerate(zip(self.sub_groups, saved)):
            if self.param_swapper is not None:
                self.param_swapper.ensure_resident(i)
            sg.master32.data.copy_(s.data.to(sg.master32.device))
            sg.copy_master_to_shards()
            if self.param_swapper is not None:
                self.param_swapper.mark_dirty(i)
                self.param_swapper.evict_to_budget()
        self._refresh_persistent_params()

    @torch.no_grad()
    def offload_states(self, include=None, device="cpu",
                       pin_memory=False, non_blocking=False):
        """Temporarily move engine-held states to host (ref
        stage3.py:3583 offload_states / offload_states.py): frees HBM for
        a generation phase (RLHF) or a different model. States:
        lp_params (16-bit shard slabs), hp_params (fp32 masters),
        lp_grads (grad accumulators), optim_states (Adam moments)."""
        inc = set(include or ("lp_params", "hp_params", "lp_grads",
                              "optim_states"))
        dev = torch.device(device)

        def _move(t):
            if t is None or t.device == dev:
                return t
            new = torch.empty_like(t, device=dev,
                                   pin_memory=pin_memory and
                                   dev.type == "cpu")
            new.copy_(t, non_blocking=non_blocking)
            return new

        for sg in self.sub_groups:
            if "lp_params" in inc and sg.flat16 is not None:
                sg.flat16 = _move(sg.flat16)
                for p in sg.params:
                    off = sg.offsets[p]
                    p.ds_tensor = sg.flat16[off:off + p.ds_shard_numel]
            if "hp_params" in inc:
                sg.master32.data = _move(sg.master32.data)
            if "lp_grads" in inc:
                sg.grad32 = _move(sg.grad32)
        if "optim_states" in inc:
            for st in self.optimizer.state.values():
                for k, v in list(st.items()):
                    if torch.is_tensor(v):
                        st[k] = _move(v)
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    def reload_states(self, non_blocking=False):
        """Bring offloaded states back to the training device."""
        self.offload_states(device=self.device,
                            non_blocking=non_blocking)

    def empty_partition_cache(self):
        """Release every gathered (non-persistent) param and return the
        HBM to the allocator (ref engine.empty_partition_cache)."""
        self._drain_inflight()
        for p in self._all_params:
            if not p.ds_persist:
                free_param(p)
        if torch.cuda.is_available():
            torch.cuda.empty_cache()

    def destroy(self):
        for h in self._grad_hooks + self._module_hooks:
            h.remove()
        self._grad_hooks, self._module_hooks = [], []
