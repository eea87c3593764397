// bf16 storage helpers of the bf16 inference kernels.  A bf16 value travels as its bit pattern (u16); bf16 -> f32 is exact,
// f32 -> bf16 is a plain cast: v_cvt_pk_bf16_f32, round to nearest even, NaN stays NaN.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned short u16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));     // an MFMA operand fragment
typedef float f32x16 __attribute__((ext_vector_type(16)));     // a 32x32 MFMA accumulator
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));     // 16 bytes as a native vector: promoted to registers, unlike uint4 copies

__device__ __forceinline__ float bf2f(u16 v) { return __builtin_bit_cast(float, (unsigned)v << 16); }
__device__ __forceinline__ u16 f2bf(float v) { return __builtin_bit_cast(u16, (__bf16)v); }
