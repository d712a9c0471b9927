// The BAND instantiations of the two flash backward passes (sliding window
// and packed documents; the variant is described in attention_bwd.hip's
// header) and their launcher, flash_bwd_band_launch. The pre-pass they run
// after is launched by flash_attn_bwd and exists once, in attention_bwd.hip.
//
// A translation unit of its own because it is built with other flags than
// attention_bwd.hip: without packed fp32 instructions (ops/build.py,
// NO_PACKED_FP32, where the reason and the measurement are).
#define DSAMD_FLASH_BAND_TU 1
#include "attention_bwd.hip"
