// The BAND instantiations of the flash forward kernel (sliding window and
// packed documents; the variant is described in attention.hip's header) and
// their launcher, flash_fwd_band_launch.
//
// A translation unit of its own because it is built with other flags than
// attention.hip: without packed fp32 instructions (ops/build.py,
// NO_PACKED_FP32, where the reason and the measurement are).
#define DSAMD_FLASH_BAND_TU 1
#include "attention.hip"
