"""deepspeed_amd.comm — torch.distributed facade.

Parity: reference `deepspeed/comm/comm.py:227-790` (module-level collectives
mirroring torch.distributed), `:792` (init_distributed), `:106` (timed_op
profiling decorator feeding CommsLogger `deepspeed/utils/comms_logging.py:67`).

MI355X-native design: no backend registry — torch.distributed's "nccl"
backend IS RCCL on ROCm, gloo is the CPU path for plumbing tests. All
collectives are thin passthroughs (zero Python overhead on the hot path
unless the comms logger is enabled).
"""
import os
import time
from datetime import timedelta

import torch
import torch.distributed as torch_dist
from torch.distributed import ReduceOp  # re-export  # noqa: F401

from ..utils.logging import logger
from .comms_logging import CommsLogger, get_default_logger

_initialized = False
comms_logger: CommsLogger = get_default_logger()


def is_initialized():
    return torch_dist.is_available() and torch_dist.is_initialized()


def init_distributed(dist_backend=None,
                     auto_mpi_discovery=True,
                     distributed_port=29500,
                     verbose=True,
                     timeout=timedelta(minutes=30),
                     init_method=None,
                     dist_init_required=None,
                     config=None,
                     rank=-1,
                     world_size=-1):
    """Initialize torch.distributed (RCCL on ROCm GPUs, gloo on CPU)."""
    global _initialized
    if is_initialized():
        _initialized = True
        return
    if dist_backend is None:
        dist_backend = "nccl" if torch.cuda.is_available() else "gloo"
    required = {"RANK", "WORLD_SIZE", "MASTER_ADDR"}
    if not required.issubset(os.environ) and rank == -1:
        # single-process fallback
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("LOCAL_RANK", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(distributed_port))
    kwargs = dict(backend=dist_backend, timeout=timeout)
    if init_method is not None:
        kwargs["init_method"] = init_method
    if rank != -1:
        kwargs["rank"] = rank
        kwargs["world_size"] = world_size
    torch_dist.init_process_group(**kwargs)
    _initialized = True
    if verbose and get_rank() == 0:
        logger.info(f"initialized distributed: backend={dist_backend} "
                    f"world_size={get_world_size()}")
    if torch.cuda.is_available() and "LOCAL_RANK" in os.environ:
        torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))


def configure(config=None):
    """Wire the comms logger from engine config."""
    if config is not None and getattr(config, "comms_logger", None) is not None:
        cl = config.comms_logger
        comms_logger.configure(enabled=cl.enabled, verbose=cl.verbose,
                               prof_all=cl.prof_all, debug=cl.debug,
                               prof_ops=cl.prof_ops)


# ---------------------------------------------------------------------------
# profiling wrapper
# ---------------------------------------------------------------------------

def _msg_size(tensor_or_list):
    if tensor_or_list is None:
        return 0
    if torch.is_tensor(tensor_or_list):
        return tensor_or_list.numel() * tensor_or_list.element_size()
    if isinstance(tensor_or_list, (list, tuple)):
        return sum(_msg_size(t) for t in tensor_or_list)
    return 0


def timed_op(fn):
    name = fn.__name__

    def wrapper(*args, **kwargs):
        if not comms_logger.enabled:
            return fn(*args, **kwargs)
        size = _msg_size(args[0] if args else kwargs.get("tensor"))
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        t0 = time.time()
        ret = fn(*args, **kwargs)
        if kwargs.get("async_op", False):
            # logged as issue-time only; completion untracked
            comms_logger.append(name, size, time.time() - t0, async_op=True)
        else:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            comms_logger.append(name, size, time.time() - t0)
        return ret

    wrapper.__name__ = name
    return wrapper


# ---------------------------------------------------------------------------
# collectives — mirror torch.distributed call signatures
# ---------------------------------------------------------------------------

def get_rank(group=None):
    return torch_dist.get_rank(group=group) if is_initialized() else 0


def get_world_size(group=None):
    return torch_dist.get_world_size(group=group) if is_initialized() else 1


def get_local_rank():
    return int(os.environ.get("LOCAL_RANK", 0))


def get_global_rank(group, group_rank):
    return torch_dist.distributed_c10d.get_global_rank(group, group_rank)


def new_group(ranks=None, backend=None):
    return torch_dist.new_group(ranks=ranks, backend=backend)


def barrier(group=None, device_ids=None):
    return torch_dist.barrier(group=group)


@timed_op
def all_reduce(tensor, op=ReduceOp.SUM, group=None, async_op=False):
    return torch_dist.all_reduce(tensor, op=op, group=group, async_op=async_op)


@timed_op
def all_reduce_coalesced(tensors, op=ReduceOp.SUM, group=None, async_op=False):
    return torch_dist.all_reduce_coalesced(tensors, op=op, group=group,
                                           async_op=async_op)


@timed_op
def reduce(tensor, dst, op=ReduceOp.SUM, group=None, async_op=False):
    return torch_dist.reduce(tensor, dst, op=op, group=group, async_op=async_op)


@timed_op
def reduce_scatter_tensor(output, input, op=ReduceOp.SUM, group=None,
                          async_op=False):
    return torch_dist.reduce_scatter_tensor(output, input, op=op, group=group,
                                            async_op=async_op)


@timed_op
def all_gather_into_tensor(output, input, group=None, async_op=False):
    return torch_dist.all_gather_into_tensor(output, input, group=group,
                                             async_op=async_op)


@timed_op
def all_gather(tensor_list, tensor, group=None, async_op=False):
    return torch_dist.all_gather(tensor_list, tensor, group=group,
                                 async_op=async_op)


@timed_op
def all_to_all_single(output, input, output_split_sizes=None,
                      input_split_sizes=None, group=None, async_op=False):
    return torch_dist.all_to_all_single(output, input,
                                        output_split_sizes=output_split_sizes,
                                        input_split_sizes=input_split_sizes,
                                        group=group, async_op=async_op)


@timed_op
def all_to_all(output_tensor_list, input_tensor_list, group=None,
               async_op=False):
    return torch_dist.all_to_all(output_tensor_list, input_tensor_list,
                                 group=group, async_op=async_op)


@timed_op
def broadcast(tensor, src, group=None, async_op=False):
    return torch_dist.broadcast(tensor, src, group=group, async_op=async_op)


@timed_op
def broadcast_object_list(object_list, src, group=None):
    return torch_dist.broadcast_object_list(object_list, src=src, group=group)


@timed_op
def send(tensor, dst, group=None, tag=0):
    return torch_dist.send(tensor, dst, group=group, tag=tag)


@timed_op
def recv(tensor, src=None, group=None, tag=0):
    return torch_dist.recv(tensor, src=src, group=group, tag=tag)


@timed_op
def isend(tensor, dst, group=None, tag=0):
    return torch_dist.isend(tensor, dst, group=group, tag=tag)


@timed_op
def irecv(tensor, src=None, group=None, tag=0):
    return torch_dist.irecv(tensor, src=src, group=group, tag=tag)


@timed_op
def gather(tensor, gather_list=None, dst=0, group=None, async_op=False):
    return torch_dist.gather(tensor, gather_list=gather_list, dst=dst,
                             group=group, async_op=async_op)


@timed_op
def scatter(tensor, scatter_list=None, src=0, group=None, async_op=False):
    return torch_dist.scatter(tensor, scatter_list=scatter_list, src=src,
                              group=group, async_op=async_op)


@timed_op
def reduce_scatter(output, input_list, op=ReduceOp.SUM, group=None,
                   async_op=False):
    return torch_dist.reduce_scatter(output, input_list, op=op,
                                     group=group, async_op=async_op)


def all_gather_object(object_list, obj, group=None):
    return torch_dist.all_gather_object(object_list, obj, group=group)


def monitored_barrier(group=None, timeout=None, wait_all_ranks=False):
    if torch_dist.get_backend(group) == "nccl":
        # RCCL has no monitored barrier; plain barrier is the equivalent
        return torch_dist.barrier(group=group)
    return torch_dist.monitored_barrier(group=group, timeout=timeout,
                                        wait_all_ranks=wait_all_ranks)


def get_all_gather_function():
    return all_gather_into_tensor


def get_reduce_scatter_function():
    return reduce_scatter_tensor


# legacy aliases kept for reference-API compat
allgather_fn = all_gather_into_tensor
reduce_scatter_fn = reduce_scatter_tensor


@timed_op
def inference_all_reduce(tensor, op=ReduceOp.SUM, group=None):
    """TP all-reduce used by injected inference modules (ref comm.py:662)."""
    return torch_dist.all_reduce(tensor, op=op, group=group)


def log_summary(show_straggler=False):
    comms_logger.log_all(show_straggler=show_straggler)


def destroy_process_group():
    if is_initialized():
        torch_dist.destroy_process_group()
    # the cached group handles are stale now, and each one keeps its
    # backend (and the backend's worker threads) alive until it is dropped
    from . import groups
    groups.reset_groups()
