// Prefix-enabled prompt attention (chunked prefill / prefix caching) on an fp8 (e4m3) KV cache, for gfx950.
//
// Same contract as prefix_attention_kernel (prefill_attention.hip): the new tokens of a sequence attend causally
// to ALL its keys, context and new, read from the paged cache, which the backend has written before the call.
// With an fp8 cache a chunk therefore sees the quantised values of its own tokens -- the values every later
// decode step sees.  Same maths (S^T = K . Q^T and O^T += V^T . P^T on v_mfma_f32_16x16x32, fp32 online softmax
// per lane, P rounded to the model dtype, fa_mask) and the same decomposition (one 256-thread workgroup per
// (64-query tile, head, sequence), 16 query rows per wave, 64 keys per iteration, tiles wholly before the window
// skipped).
//
// What differs is how K and V reach the MFMAs.  The 16-bit kernel uses no LDS: each of the four waves loads the
// same cache lines straight into MFMA operands.  fp8 bytes must be widened to the model dtype first, and doing that
// per wave would repeat the conversion four times, so here the workgroup does it once and shares the result:
//   gather   thread -> 16 bytes of the K plane [NB, KVH, D/16, BS, 16] = 16 head dims of one key (consecutive
//            threads take consecutive keys: contiguous within a block), and min(BS, 16) bytes of the V plane
//            [NB, KVH, D, BS] = that many consecutive tokens of one head dim (consecutive threads take consecutive
//            head dims: contiguous within a block).  Keys are clamped to the sequence before the block table is
//            read; bytes of keys at or past its end are cleared (fp8 0x00 = +0), because the cache behind a
//            sequence is uninitialised and 0 x NaN would poison a row through V.
//   convert  v_cvt_pk_f32_fp8 + pack to the model dtype (fp8x4_to_pairs_t): exact, e4m3 has 3 mantissa bits.
//            kv_scale is never applied per element: K's factor is folded into the softmax scale, V's into 1 / l.
//   stage    K row-major per key, row stride D + 8 elements: the A operand of S^T is one ds_read_b128 per
//            (key, 32-dim chunk), conflict-free.  V as V^T, head dim major, 64 keys per row, row stride 72
//            elements = 36 dwords: the A operand of O^T is two ds_read_b64 of keys {4g..4g+3} and {16+4g..16+4g+3},
//            and a half-wave (16 rows x 2 groups x 2 dwords) covers the 64 banks exactly once.  The cache already
//            holds V transposed, so no transposed LDS read is needed.
//   overlap  the raw bytes of tile kt+1 are fetched into registers (16 VGPRs at D = 128) before the MFMAs of
//            tile kt and converted and parked after them.
//
// LDS budget: one converted K + V image is 64 * 136 * 2 + 128 * 72 * 2 = 35840 bytes at D = 128; two would be
// 71680, over the 64 KiB static limit.  Chosen: ONE converted buffer plus the register prefetch, two barriers per
// tile (readers done -> park -> visible).  The 160 KiB of a gfx950 CU then hold four workgroups where a double
// buffer behind a dynamic-LDS opt-in would hold two, and other workgroups' MFMAs cover a workgroup's barriers.
// Registers decide the rest: the launch bounds ask for 3 waves per SIMD at D = 128 (136-148 VGPRs, no scratch;
// a bound of 4 spills 10-24 VGPRs) and 4 at D = 64 (99-104 VGPRs), against 2 / 3 of the 16-bit kernel.
// -Rpass-analysis=kernel-resource-usage lines are quoted in DESIGN.md 3.8.
#include "fa_common.h"

namespace nmv {

template <typename T, int D, int BS>
__global__ __launch_bounds__(256, D == 128 ? 3 : 4) void prefix_attention_fp8_kernel(const Pfx8Params p) {
  static_assert(D == 64 || D == 128, "head size");
  static_assert(BS == 8 || BS == 16 || BS == 32, "block size");
  constexpr int DC = D / 32, DT = D / 16;
  constexpr int KS = D + 8;                 // K image: elements per key row
  constexpr int VS = FA_KT + 8;             // V^T image: elements per head-dim row
  constexpr int KP = FA_KT * (D / 16) / 256;   // 16-byte K pieces per thread
  constexpr int PB = BS < 16 ? BS : 16;     // bytes (= tokens) of a V piece
  constexpr int PPR = BS / PB;              // V pieces per (head dim, block)
  constexpr int ROWP = D * PPR;             // V pieces per block
  constexpr int VP = (FA_KT / BS) * ROWP / 256;   // V pieces per thread
  static_assert(KP >= 1 && VP >= 1 && (FA_KT / BS) * ROWP % 256 == 0, "whole pieces per thread");
  __shared__ __attribute__((aligned(16))) uint16_t k_s[FA_KT * KS];
  __shared__ __attribute__((aligned(16))) uint16_t v_s[D * VS];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int seq = blockIdx.z, head = blockIdx.y;
  const int kv_head = head / (p.num_heads / p.num_kv_heads);
  const int tok0 = p.q_start[seq];
  const int q_len = p.q_start[seq + 1] - tok0;
  const int L = p.seq_lens[seq];
  const int ctx = p.ctx_lens[seq];
  const int qt0 = blockIdx.x * FA_QT;
  if (qt0 >= q_len) return;  // uniform: before any barrier
  const int q_row = qt0 + wave * 16 + r;          // new-token index of this lane's query
  const int q_pos = ctx + q_row;                  // its position in the sequence
  const int* bt = p.block_tables + (int64_t)seq * p.max_blocks;
  const uint8_t* kbase = p.kc + (int64_t)kv_head * p.kv_head_stride;
  const uint8_t* vbase = p.vc + (int64_t)kv_head * p.kv_head_stride;

  uint4 qf[DC];
  {
    const uint16_t* qp = p.q + (int64_t)(tok0 + min(q_row, q_len - 1)) * p.q_stride + (int64_t)head * D + g * 8;
#pragma unroll
    for (int c = 0; c < DC; ++c) qf[c] = ld16(qp + c * 32);
  }
  f32x4_t o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const int last_pos = ctx + min(qt0 + FA_QT, q_len) - 1;   // causal: keys 0 .. last_pos (< L)
  const int n_kt = last_pos / FA_KT + 1;
  const int kt_lo = p.window > 0 ? max(ctx + qt0 - p.window + 1, 0) / FA_KT : 0;
  const float sc = p.scale * p.kv_scale;          // K's dequantisation factor rides on the softmax scale
  const float slope = p.alibi_slopes ? p.alibi_slopes[head] : 0.f;
  const bool every_tile = p.window > 0 || slope != 0.f;   // uniform

  // ---- tile loader.  K: thread t owns key t & 63, 16-dim chunks (t >> 6) + 4 i.  V: piece id = t + 256 i is
  // (block of the tile, head dim, PB-token part of the block), head dim fastest across threads ----
  const int k_key = threadIdx.x & 63, k_c16 = threadIdx.x >> 6;
  uint4 kraw[KP];
  uint32_t vraw[VP][PB / 4];
  auto fetch = [&](int kt) {
    const int k0 = kt * FA_KT;
    {
      const int key = k0 + k_key;
      const int kc = min(key, L - 1);       // clamp BEFORE the block table: entries past the last block are not read
      const uint8_t* src = kbase + (int64_t)bt[kc / BS] * p.kv_block_stride + (kc % BS) * 16;
      const uint32_t keep = key < L ? 0xffffffffu : 0u;
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        const uint4 w = ld16(src + (k_c16 + 4 * i) * (BS * 16));
        kraw[i] = make_uint4(w.x & keep, w.y & keep, w.z & keep, w.w & keep);
      }
    }
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      const int id = threadIdx.x + i * 256;
      const int j = id % ROWP, d = j / PPR, part = j % PPR;
      const int key = k0 + (id / ROWP) * BS + part * PB;    // first token of the piece
      const int kc = min(key, L - 1);
      const uint8_t* src = vbase + (int64_t)bt[kc / BS] * p.kv_block_stride + d * BS + part * PB;
      const int valid = L - key;            // tokens of the piece inside the sequence (may be <= 0 or >= PB)
      if constexpr (PB == 16) {
        const uint4 w = ld16(src);
        vraw[i][0] = w.x & low_bytes(valid);
        vraw[i][1] = w.y & low_bytes(valid - 4);
        vraw[i][2] = w.z & low_bytes(valid - 8);
        vraw[i][3] = w.w & low_bytes(valid - 12);
      } else {
        const uint2 w = ld8(src);
        vraw[i][0] = w.x & low_bytes(valid);
        vraw[i][1] = w.y & low_bytes(valid - 4);
      }
    }
  };
  // convert once per workgroup and store in operand order
  auto park = [&]() {
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      uint32_t e[8];
      fp8x4_to_pairs_t<T>(kraw[i].x, e[0], e[1]);
      fp8x4_to_pairs_t<T>(kraw[i].y, e[2], e[3]);
      fp8x4_to_pairs_t<T>(kraw[i].z, e[4], e[5]);
      fp8x4_to_pairs_t<T>(kraw[i].w, e[6], e[7]);
      uint4* dst = reinterpret_cast<uint4*>(&k_s[k_key * KS + (k_c16 + 4 * i) * 16]);
      dst[0] = make_uint4(e[0], e[1], e[2], e[3]);
      dst[1] = make_uint4(e[4], e[5], e[6], e[7]);
    }
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      const int id = threadIdx.x + i * 256;
      const int j = id % ROWP, d = j / PPR, part = j % PPR;
      uint32_t e[PB / 2];
#pragma unroll
      for (int w = 0; w < PB / 4; ++w) fp8x4_to_pairs_t<T>(vraw[i][w], e[2 * w], e[2 * w + 1]);
      uint4* dst = reinterpret_cast<uint4*>(&v_s[d * VS + (id / ROWP) * BS + part * PB]);
#pragma unroll
      for (int w = 0; w < PB / 8; ++w) dst[w] = make_uint4(e[4 * w], e[4 * w + 1], e[4 * w + 2], e[4 * w + 3]);
    }
  };
  fetch(kt_lo);
  park();
  __syncthreads();

  for (int kt = kt_lo; kt < n_kt; ++kt) {
    const int k0 = kt * FA_KT;
    const bool more = kt + 1 < n_kt;                // uniform
    if (more) fetch(kt + 1);                        // raw bytes land in registers while this tile is consumed
    // ---- S^T = K . Q^T: K rows from LDS, shared by the 4 waves ----
    f32x4_t s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const uint16_t* kp = &k_s[(t * 16 + r) * KS + g * 8];
#pragma unroll
      for (int c = 0; c < DC; ++c) s[t] = FaMfma<T>::run(*reinterpret_cast<const uint4*>(kp + c * 32), qf[c], s[t]);
    }
    // ---- scale, mask, online softmax (row = this lane's query) ----
    const bool diag = every_tile || k0 + FA_KT - 1 > ctx + qt0;   // uniform; true on the tile that holds L
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + t * 16 + 4 * g + i;
        float x = s[t][i] * sc;
        if (diag) x = fa_mask(x, key, q_pos, L, slope, p.window);
        s[t][i] = x;
        mx = fmaxf(mx, x);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);           // finite: the first tile holds a key at or before every query
    const float alpha = __expf(m_run - m_new);
    float psum = 0.f;
    uint32_t pp[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      float e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        e[i] = T::to_float(T::from_float(__expf(s[t][i] - m_new)));   // P in the model dtype, and the sum of the same
        psum += e[i];
      }
      pp[2 * t] = T::pack2(e[0], e[1]);
      pp[2 * t + 1] = T::pack2(e[2], e[3]);
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int t = 0; t < DT; ++t) o[t] *= alpha;
    // ---- O^T += V^T . P^T: V^T row d = 16 t + r, keys 32 st + {4g..4g+3, 16+4g..16+4g+3} ----
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const uint4 pb = make_uint4(pp[4 * st], pp[4 * st + 1], pp[4 * st + 2], pp[4 * st + 3]);
#pragma unroll
      for (int t = 0; t < DT; ++t) {
        const uint16_t* vp = &v_s[(16 * t + r) * VS + 32 * st + 4 * g];
        const uint2 lo = *reinterpret_cast<const uint2*>(vp);
        const uint2 hi = *reinterpret_cast<const uint2*>(vp + 16);
        o[t] = FaMfma<T>::run(make_uint4(lo.x, lo.y, hi.x, hi.y), pb, o[t]);
      }
    }
    if (more) {
      __syncthreads();      // every wave has read tile kt
      park();
      __syncthreads();      // tile kt+1 is visible
    }
  }
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  if (q_row >= q_len) return;
  const float inv = p.kv_scale / l_run;             // V's dequantisation factor rides on the normalisation
  uint16_t* op = p.out + (int64_t)(tok0 + q_row) * p.o_stride + (int64_t)head * D + 4 * g;
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    uint2 pk;
    pk.x = T::pack2(o[t][0] * inv, o[t][1] * inv);
    pk.y = T::pack2(o[t][2] * inv, o[t][3] * inv);
    *reinterpret_cast<uint2*>(op + 16 * t) = pk;
  }
}

template <typename T, int D>
static void launch_pfx8(int block_size, dim3 grid, hipStream_t s, const Pfx8Params& p) {
  const dim3 block(256);
  if (block_size == 8) hipLaunchKernelGGL((prefix_attention_fp8_kernel<T, D, 8>), grid, block, 0, s, p);
  else if (block_size == 16) hipLaunchKernelGGL((prefix_attention_fp8_kernel<T, D, 16>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((prefix_attention_fp8_kernel<T, D, 32>), grid, block, 0, s, p);
}

}  // namespace nmv

using namespace nmv;

extern "C" int nmv_prefix_prefill_attention_fp8(void* out, const void* q, const void* key_cache,
                                                const void* value_cache, const int32_t* block_tables,
                                                const int32_t* query_start_loc, const int32_t* seq_lens,
                                                const int32_t* context_lens, int num_seqs,
                                                int max_query_len, int max_blocks_per_seq, int block_size,
                                                int num_heads, int num_kv_heads, int head_size, float scale,
                                                int64_t q_stride, int64_t o_stride, int64_t kv_block_stride,
                                                int64_t kv_head_stride, const float* alibi_slopes,
                                                int sliding_window, nmv_dtype_t dtype, nmv_kv_dtype_t kv_dtype,
                                                float kv_scale, void* stream) {
  NMV_CHECK(kv_dtype == NMV_KV_FP8_E4M3, "prefix_prefill_attention_fp8: kv cache dtype must be fp8 e4m3");
  NMV_CHECK(dtype == NMV_F16 || dtype == NMV_BF16, "prefix_prefill_attention_fp8: fp16 / bf16 queries only");
  NMV_CHECK(head_size == 64 || head_size == 96 || head_size == 112 || head_size == 128 || head_size == 192 ||
            head_size == 256, "prefix_prefill_attention_fp8: head size %d not built (64, 96, 112, 128, 192, 256)", head_size);
  NMV_CHECK(block_size == 8 || block_size == 16 || block_size == 32, "prefix_prefill_attention_fp8: block size %d", block_size);
  NMV_CHECK(num_kv_heads > 0 && num_heads % num_kv_heads == 0, "prefix_prefill_attention_fp8: heads %% kv_heads != 0");
  NMV_CHECK(q_stride % 8 == 0 && o_stride % 4 == 0, "prefix_prefill_attention_fp8: token strides break alignment");
  NMV_CHECK(kv_block_stride % 16 == 0 && kv_head_stride % 16 == 0 && (uintptr_t)key_cache % 16 == 0 &&
            (uintptr_t)value_cache % 16 == 0, "prefix_prefill_attention_fp8: cache planes must keep 16-byte alignment");
  if (num_seqs <= 0 || max_query_len <= 0) return NMV_OK;
  Pfx8Params p{(const uint16_t*)q, (uint16_t*)out, (const uint8_t*)key_cache, (const uint8_t*)value_cache,
               block_tables, query_start_loc, seq_lens, context_lens, q_stride, o_stride, kv_block_stride,
               kv_head_stride, max_blocks_per_seq, num_heads, num_kv_heads, scale, kv_scale, alibi_slopes,
               sliding_window > 0 ? sliding_window : 0};
  const dim3 grid((max_query_len + FA_QT - 1) / FA_QT, num_heads, num_seqs);
  hipStream_t s = (hipStream_t)stream;
  if (head_size != 64 && head_size != 128) {   // prefix_attention_fp8_wide.hip
    NMV_CHECK(launch_prefix_fp8_wide(p, dtype == NMV_BF16, head_size, block_size, grid, s),
              "prefix_prefill_attention_fp8: no kernel for head size %d, block size %d", head_size, block_size);
  } else if (dtype == NMV_BF16) {
    if (head_size == 64) launch_pfx8<BF16, 64>(block_size, grid, s, p);
    else launch_pfx8<BF16, 128>(block_size, grid, s, p);
  } else {
    if (head_size == 64) launch_pfx8<F16, 64>(block_size, grid, s, p);
    else launch_pfx8<F16, 128>(block_size, grid, s, p);
  }
  NMV_LAUNCH_CHECK();
  return NMV_OK;
}
