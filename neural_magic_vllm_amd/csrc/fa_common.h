// What the prompt-attention kernels share (prefill_attention.hip, prefix_attention_fp8.hip): the tile sizes,
// the MFMA of the model dtype and the logit mask.
#pragma once
#include "common.h"

namespace nmv {

constexpr int FA_QT = 64;   // queries per workgroup
constexpr int FA_KT = 64;   // keys per iteration

template <typename T> struct FaMfma;
template <> struct FaMfma<BF16> {
  static __device__ __forceinline__ f32x4_t run(uint4 a, uint4 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
};
template <> struct FaMfma<F16> {
  static __device__ __forceinline__ f32x4_t run(uint4 a, uint4 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
};

// logit of (query position qp, key position key) after the softmax scale: ALiBi bias, causal / length mask
// (-inf) and the sliding window, which the reference masks with -10000 rather than -inf because a whole tile of
// a row may lie outside the window (prefix_prefill.py:130-144, :201-204; alibi :552-557)
__device__ __forceinline__ float fa_mask(float x, int key, int qp, int L, float slope, int window) {
  x += slope * (float)(key - qp);
  if (window > 0 && qp - key >= window) x = -10000.f;
  if (key > qp || key >= L) x = -INFINITY;
  return x;
}

}  // namespace nmv
