// Used by so3conv_y.hip: the constants and vector types of the inter conv's 32x32x16 kernel, its transposed LDS read and the inline-asm W load of step 2.
#pragma once
#include "common.h"
#include "split_bf16.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define NA 60
#define KS 24

__device__ __forceinline__ bf16x4 x_tr16(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((bf16x4 __attribute__((address_space(3)))*)p);
}
// a 16-byte global load with a wave-uniform base (SGPR pair) + 32-bit lane offset + k KiB immediate; the caller counts its own waits (s_waitcnt vmcnt)
__device__ __forceinline__ void x_wload_s(f32x4& dst, unsigned voff, const void* sbase, int k) {
    if (k == 0) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(dst) : "v"(voff), "s"(sbase));
    else if (k == 1) asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=v"(dst) : "v"(voff), "s"(sbase));
    else asm volatile("global_load_dwordx4 %0, %1, %2 offset:2048" : "=v"(dst) : "v"(voff), "s"(sbase));
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
