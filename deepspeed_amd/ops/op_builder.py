"""op_builder compatibility shim.

Parity: reference `deepspeed/ops/op_builder/*` (JIT builders like
FusedAdamBuilder().load()). Here every kernel is AOT-compiled into the
single in-tree `_hip_ops` extension (ops/build.py, hipcc gfx950), so a
"builder" just verifies the op family is present and returns the loaded
extension module. Code written against the reference's builder API keeps
working; there is nothing to JIT.
"""
from .loader import get_ext


class _PrebuiltBuilder:
    NAME = "base"
    _required_syms = ()

    def load(self, verbose=False):
        ext = get_ext(required=True)
        for sym in self._required_syms:
            if not hasattr(ext, sym):
                raise RuntimeError(
                    f"{self.NAME}: symbol {sym} missing from _hip_ops — "
                    "rebuild with python -m deepspeed_amd.ops.build")
        return ext

    def is_compatible(self, verbose=False):
        return True

    def jit_load(self, verbose=False):
        return self.load(verbose)


class FusedAdamBuilder(_PrebuiltBuilder):
    NAME = "fused_adam"
    _required_syms = ("multi_tensor_adam",)


class FusedLambBuilder(_PrebuiltBuilder):
    NAME = "fused_lamb"
    _required_syms = ("multi_tensor_lamb",)


class FusedLionBuilder(_PrebuiltBuilder):
    NAME = "fused_lion"
    _required_syms = ("multi_tensor_lion",)


class CPUAdamBuilder(_PrebuiltBuilder):
    NAME = "cpu_adam"
    _required_syms = ("cpu_adam_step",)


class CPUAdagradBuilder(_PrebuiltBuilder):
    NAME = "cpu_adagrad"
    _required_syms = ("cpu_adagrad_step",)


class CPULionBuilder(_PrebuiltBuilder):
    NAME = "cpu_lion"
    _required_syms = ("cpu_lion_step",)


class AsyncIOBuilder(_PrebuiltBuilder):
    NAME = "async_io"
    _required_syms = ("aio_handle",)


class QuantizerBuilder(_PrebuiltBuilder):
    NAME = "quantizer"
    _required_syms = ("quantize_int8", "quantize_fp8")


class FPQuantizerBuilder(_PrebuiltBuilder):
    NAME = "fp_quantizer"
    _required_syms = ("quantize_fp_em",)


class TransformerBuilder(_PrebuiltBuilder):
    NAME = "transformer"
    _required_syms = ("flash_attn_fwd", "rmsnorm_fwd", "rope",
                     "cross_entropy_fwd")


class InferenceBuilder(_PrebuiltBuilder):
    NAME = "transformer_inference"
    _required_syms = ("flash_attn_fwd", "gemv_bf16")


class SpatialInferenceBuilder(_PrebuiltBuilder):
    NAME = "spatial_inference"
    _required_syms = ("spatial_bias_add",)


class RaggedOpsBuilder(_PrebuiltBuilder):
    NAME = "ragged_ops"
    _required_syms = ("ragged_decode", "ragged_prefill",
                      "ragged_rope_append")
