// What the prompt-attention kernels share (prefill_attention.hip, prefill_attention_blocksparse.hip,
// prefix_attention_staged.hip, prefix_attention_fp8.hip, prefix_attention_fp8_wide.hip): the tile sizes and the tile
// plan per head size, the MFMAs of the model dtype, the logit mask and the parameters of the prefix kernels, 16-bit
// and fp8 cache.
#pragma once
#include "common.h"

namespace nmv {

constexpr int FA_QT = 64;   // queries per workgroup
constexpr int FA_KT = 64;   // keys per iteration (head sizes up to 128; the wider ones choose their own, see the kernels)

typedef short v4s_t __attribute__((ext_vector_type(4)));
typedef v4s_t __attribute__((address_space(3))) lds_v4s_t;
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));

// The tile plan per head size.  A K + V image pair of KT keys is 2 * KT * (D + 8) * 2 bytes.  A gfx950 CU has
// 160 KiB of LDS and the compiler accepts more than 64 KiB of it per workgroup (head size 128 has always used
// 69632 B), so the plan is a choice, not a limit: keep two workgroups on a CU.
//   D <= 128  64 keys per iteration, double buffered (D = 112: 61440 B, D = 128: 69632 B)
//   D  = 192  32 keys, double buffered (51200 B; 64 keys would be 102400 B: one workgroup per CU)
//   D  = 256  32 keys, ONE buffer (33792 B): the next tile still waits in registers while this one is consumed, and
//             is parked between two barriers, as prefix_attention_fp8_kernel does.  Two buffers (67584 B) were
//             measured against it: DESIGN.md 3.8
template <int D> struct FaPlan {
  static constexpr int KT = D <= 128 ? FA_KT : 32;                          // keys per iteration
  static constexpr bool DB = D != 256;                                      // double buffered
  // waves per SIMD asked of the register allocator: the highest that leaves no scratch and that the LDS image
  // lets run; 64 and 128 keep the allocator's default
  static constexpr int WAVES = D == 64 || D == 128 ? 1 : (D == 96 || D == 192 ? 3 : 2);
};

template <typename T> struct FaMfma;
template <> struct FaMfma<BF16> {
  static __device__ __forceinline__ f32x4_t run(uint4 a, uint4 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
  // the 16-wide tail of a contraction whose length is 16 mod 32 (head size 112): v_mfma_f32_16x16x16.  Lane
  // (r, g) supplies k = 4g .. 4g+3 of row / column r; the accumulator layout is that of the 32-wide step
  static __device__ __forceinline__ f32x4_t run16(uint2 a, uint2 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4_t, a), __builtin_bit_cast(s16x4_t, b), c, 0, 0, 0);
  }
};
template <> struct FaMfma<F16> {
  static __device__ __forceinline__ f32x4_t run(uint4 a, uint4 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x4_t run16(uint2 a, uint2 b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4_t, a), __builtin_bit_cast(f16x4_t, b), c, 0, 0, 0);
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

// prefix-enabled prefill on a 16-bit cache: prefix_attention_kernel (prefill_attention.hip, head sizes 64 / 128)
// and prefix_attention_staged_kernel (prefix_attention_staged.hip, head sizes 96 / 112 / 192 / 256)
struct PfxParams {
  const uint16_t* q;    // [new tokens, H, D]
  uint16_t* out;
  const uint16_t* kc;   // key cache
  const uint16_t* vc;   // value cache
  const int* block_tables;   // [num_seqs, max_blocks]
  const int* q_start;        // [num_seqs + 1] offsets of the new tokens
  const int* seq_lens;       // [num_seqs] context + new
  const int* ctx_lens;       // [num_seqs]
  int64_t q_stride, o_stride, kv_block_stride, kv_head_stride;  // elements
  int max_blocks, block_size, num_heads, num_kv_heads;
  float scale;
  const float* alibi_slopes;  // [H] or null
  int window;                 // sliding window, 0 = none
};

// launches prefix_attention_staged_kernel; false when (head_size, p.block_size) has no instantiation
bool launch_prefix_staged(const PfxParams& p, bool bf16, int head_size, dim3 grid, hipStream_t s);

// prefix-enabled prefill on an fp8 (e4m3) cache: prefix_attention_fp8_kernel (prefix_attention_fp8.hip, head sizes
// 64 / 128) and prefix_attention_fp8_wide_kernel (prefix_attention_fp8_wide.hip, head sizes 96 / 112 / 192 / 256)
struct Pfx8Params {
  const uint16_t* q;    // [new tokens, H, D]
  uint16_t* out;
  const uint8_t* kc;    // key cache   [NB, KVH, D/16, BS, 16] e4m3
  const uint8_t* vc;    // value cache [NB, KVH, D, BS] e4m3
  const int* block_tables;   // [num_seqs, max_blocks]
  const int* q_start;        // [num_seqs + 1] offsets of the new tokens
  const int* seq_lens;       // [num_seqs] context + new
  const int* ctx_lens;       // [num_seqs]
  int64_t q_stride, o_stride;                  // elements
  int64_t kv_block_stride, kv_head_stride;     // cache elements = bytes
  int max_blocks, num_heads, num_kv_heads;
  float scale, kv_scale;
  const float* alibi_slopes;  // [H] or null
  int window;                 // sliding window, 0 = none
};

// the low n bytes of a dword (n <= 0: none, n >= 4: all)
__device__ __forceinline__ uint32_t low_bytes(int n) {
  return n >= 4 ? 0xffffffffu : (n <= 0 ? 0u : (1u << (8 * n)) - 1u);
}

// launches prefix_attention_fp8_wide_kernel; false when (head_size, block_size) has no instantiation
bool launch_prefix_fp8_wide(const Pfx8Params& p, bool bf16, int head_size, int block_size, dim3 grid, hipStream_t s);

}  // namespace nmv
