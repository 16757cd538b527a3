// Prefix-enabled prompt attention (chunked prefill / prefix caching) on an fp8 (e4m3) KV cache at the head sizes
// beyond 64 / 128 -- 96, 112, 192 and 256 -- for gfx950.
//
// Contract of prefix_attention_fp8_kernel (prefix_attention_fp8.hip): every key and value, context and new, is read
// from the paged uint8 cache (K plane [NB, KVH, D/16, BS, 16], V plane [NB, KVH, D, BS]); kv_scale is never applied
// per element (K's factor rides on the softmax scale, V's on 1 / l); a key is clamped to the sequence BEFORE the block
// table is read, and bytes of keys at or past its end are cleared before conversion (fp8 0x00 = +0: the cache behind
// a sequence is uninitialised and 0 x NaN would poison a row through V).  Maths of the other prompt kernels:
// S^T = K . Q^T and O^T += V^T . P^T on v_mfma_f32_16x16x32, fp32 online softmax per lane, P rounded to the model
// dtype, fa_mask; one 256-thread workgroup per (64-query tile, head, sequence), 16 query rows per wave, tiles wholly
// before the window skipped.
//
// Tile plan (Pfx8WidePlan).  The workgroup gathers the raw bytes of a tile once, converts them once
// (v_cvt_pk_f32_fp8 + pack: exact) and shares ONE converted K + V^T image of KT keys, (KT (D + 8) + D (KT + 8)) 2
// bytes; the raw bytes of tile kt+1 wait in registers across the MFMAs of tile kt and are converted and parked
// between two barriers.  The alternatives weighed:
//   raw staging   parking the raw bytes halves the image (D = 256, 64 keys: 35 KiB instead of 69), but then each of
//                 the four waves widens every K and V operand for itself: 4x the v_cvt + pack work (about 3 VALU ops
//                 per element pair), issued between the MFMAs that wait for it.  A CU holds 8 waves of this kernel
//                 either way at D >= 192 (registers: O^T alone is D / 4 VGPRs, Q another D / 8), so the LDS saved
//                 buys no occupancy.  Not taken.
//   two buffers   saves one barrier per tile and doubles the image: 106 KiB at D = 192, one workgroup per CU.  At
//                 96 / 112 it would fit, but the single buffer already leaves 5-6 workgroups' worth of LDS and the
//                 other workgroups' MFMAs cover the barriers, as at 64 / 128.  Not taken.
//   keys / iter   64 at every head size.  The 16-bit staged kernel drops to 32 keys at D = 256 because its register
//                 prefetch would be 64 VGPRs; raw fp8 bytes make it 32.  32 keys at D = 256 (37376 B, 164-175 VGPRs,
//                 3 waves / SIMD at block 8 / 16) were built and measured: slower on a chunk behind a context,
//                 4 % faster on a prompt without one.  64 stays.
//      D    KT   LDS bytes   workgroups / CU (160 KiB)   waves / SIMD asked   prefetch VGPRs (K + V)
//      96   64     27136              6                    4 (3 at block 8)        8 + 8 (12 at block 8)
//     112   64     31488              5                         3                  8 + 8 (16 at block 8)
//     192   64     53248              3                         2                 12 + 12
//     256   64     70656              2                         2                 16 + 16
//   The launch bound is the highest waves / SIMD that leaves no scratch (one step higher spills 12-128 B / lane;
//   DESIGN.md 3.8 quotes the -Rpass-analysis=kernel-resource-usage lines); at 192 / 256 registers, not LDS, set
//   the occupancy.
//
// Ragged gather.  A 64-key K tile is D / 64 16-byte pieces per thread (1.5 at 96, 1.75 at 112) and the V tile D / 64
// 16-byte or, at block size 8, D / 32 8-byte pieces: the last round of each is guarded, in fetch and in park alike.
// The access pattern is that of the 64 / 128 kernel.  K: thread t keeps key t % 64 and takes the 16-dim chunks
// t / 64 + 4 i, so consecutive threads read consecutive keys (contiguous 16-byte pieces within a block) and a thread
// reads the block table once per tile.  V: piece id = t + 256 i is (block of the tile, head dim, part of the block),
// part fastest, i.e. memory order: a block's D x BS plane is one contiguous run.  K's short last round falls to the
// low waves, so V's is handed to the HIGH threads (still consecutive threads on consecutive pieces): at D = 96 every
// wave then converts three pieces per tile instead of four in waves 0-1 and two in waves 2-3, and the barrier waits
// for the slowest wave.  All block-table entries of a tile are requested before any of its bytes (one dependent
// round trip per tile, not one per piece); at D = 256 they are requested a whole tile earlier (Pfx8WidePlan::AHEAD).
//
// LDS strides.  K row-major per key, row stride D + 8 elements = 13 / 15 / 25 / 33 x 16 bytes, odd at all four sizes:
// the A operand of S^T is one ds_read_b128 per (key, 32-dim chunk) and the 16 keys of a quarter-wave start 16 bytes x
// an odd number apart, so they cover the banks without conflict.  V as V^T, head dim major, row stride KT + 8 = 72
// elements = 36 dwords: the A operand of O^T is two ds_read_b64 of keys {4g..4g+3} and {16+4g..16+4g+3}, and a
// half-wave (16 rows x 2 groups x 2 dwords) covers the 64 banks exactly once.  The cache already holds V transposed.
//
// Head size 112 leaves a 16-wide rest of the three 32-wide k-steps of S^T: one v_mfma_f32_16x16x16 (FaMfma::run16,
// same accumulator layout), accumulated from zero and added by the VALU (the direct chain miscompared).
#include "fa_common.h"

namespace nmv {

template <int D, int BS> struct Pfx8WidePlan {
  static constexpr int KT = 64;             // keys per iteration
  // block-table entries read one tile before the bytes they lead to (measured per head size: DESIGN.md 5)
  static constexpr bool AHEAD = D == 256;
  // waves per SIMD asked of the register allocator: the highest that leaves no scratch.  Block size 8 fetches V in
  // 8-byte pieces, twice as many address computations in flight: at D = 96 that is the step from 123 VGPRs to a spill
  static constexpr int WAVES = D == 96 ? (BS == 8 ? 3 : 4) : (D == 112 ? 3 : 2);
};

template <typename T, int D, int BS>
__global__ __launch_bounds__(256, (Pfx8WidePlan<D, BS>::WAVES)) void prefix_attention_fp8_wide_kernel(const Pfx8Params p) {
  static_assert(D % 16 == 0 && D <= 256, "head size");
  static_assert(BS == 8 || BS == 16 || BS == 32, "block size");
  constexpr int KT = Pfx8WidePlan<D, BS>::KT;
  constexpr int NT = KT / 16;               // 16-key tiles of S
  constexpr int NS = KT / 32;               // 32-key steps of P.V
  constexpr int DC = D / 32, DT = D / 16;
  constexpr bool TAIL = D % 32 != 0;
  constexpr int KS = D + 8;                 // K image: elements per key row
  constexpr int VS = KT + 8;                // V^T image: elements per head-dim row
  static_assert((KS / 8) % 2 == 1 && KT % BS == 0 && 256 % KT == 0, "K row stride / whole blocks per tile");
  constexpr int KSTEP = 256 / KT;           // K: 16-dim chunks between a thread's pieces
  constexpr int KP = (DT + KSTEP - 1) / KSTEP;     // 16-byte K pieces per thread
  constexpr bool K_RAGGED = DT % KSTEP != 0;       // 96: 1.5, 112: 1.75 pieces per thread
  constexpr int PB = BS < 16 ? BS : 16;     // bytes (= tokens) of a V piece
  constexpr int PPR = BS / PB;              // V pieces per (head dim, block)
  constexpr int ROWP = D * PPR;             // V pieces per block
  constexpr int VPIECES = (KT / BS) * ROWP; // V pieces per tile
  constexpr int VP = (VPIECES + 255) / 256; // V pieces per thread
  constexpr bool V_RAGGED = VPIECES % 256 != 0;
  __shared__ __attribute__((aligned(16))) uint16_t k_s[KT * KS];
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
  uint2 qtail;                                    // TAIL: dims D - 16 + 4 g .. + 3
  {
    const uint16_t* qp = p.q + (int64_t)(tok0 + min(q_row, q_len - 1)) * p.q_stride + (int64_t)head * D;
#pragma unroll
    for (int c = 0; c < DC; ++c) qf[c] = ld16(qp + c * 32 + g * 8);
    if constexpr (TAIL) qtail = ld8(qp + DC * 32 + g * 4);
  }
  f32x4_t o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const int last_pos = ctx + min(qt0 + FA_QT, q_len) - 1;   // causal: keys 0 .. last_pos (< L)
  const int n_kt = last_pos / KT + 1;
  const int kt_lo = p.window > 0 ? max(ctx + qt0 - p.window + 1, 0) / KT : 0;
  const float sc = p.scale * p.kv_scale;          // K's dequantisation factor rides on the softmax scale
  const float slope = p.alibi_slopes ? p.alibi_slopes[head] : 0.f;
  const bool every_tile = p.window > 0 || slope != 0.f;   // uniform

  // ---- tile loader.  K: thread t owns key t % KT, 16-dim chunks t / KT + KSTEP i.  V: piece id = t + 256 i is
  // (block of the tile, head dim, PB-token part of the block), part fastest.  Both guard their last round ----
  const int k_key = threadIdx.x % KT, k_c16 = threadIdx.x / KT;
  // V's last round goes to the HIGH threads, K's to the low ones, so that no wave converts both rests
  auto v_piece = [&](int i) {
    return i * 256 + (int)threadIdx.x - (V_RAGGED && i == VP - 1 ? 256 - VPIECES % 256 : 0);
  };
  // the block-table entries of a tile are read together, ahead of all its bytes, so that a fetch is two round trips
  // to memory and not one pair per piece; with AHEAD they are read one tile earlier still.  A key is clamped BEFORE
  // the table is read: entries past the last block are not touched, whatever tile is asked for
  constexpr bool AHEAD = Pfx8WidePlan<D, BS>::AHEAD;
  int kblk, vblk[VP];
  auto lookup = [&](int kt) {
    const int k0 = kt * KT;
    kblk = bt[min(k0 + k_key, L - 1) / BS];
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      const int id = v_piece(i);
      if (V_RAGGED && i == VP - 1 && (id < 256 * i || id >= VPIECES)) break;
      vblk[i] = bt[min(k0 + (id / ROWP) * BS + (id % ROWP % PPR) * PB, L - 1) / BS];
    }
  };
  uint4 kraw[KP];
  uint32_t vraw[VP][PB / 4];
  auto fetch = [&](int kt) {      // AHEAD: after lookup(kt)
    if (!AHEAD) lookup(kt);
    const int k0 = kt * KT;
    {
      const int key = k0 + k_key;
      const uint8_t* src = kbase + (int64_t)kblk * p.kv_block_stride + (min(key, L - 1) % BS) * 16;
      const uint32_t keep = key < L ? 0xffffffffu : 0u;
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        const int c16 = k_c16 + KSTEP * i;
        if (K_RAGGED && i == KP - 1 && c16 >= DT) break;
        const uint4 w = ld16(src + c16 * (BS * 16));
        kraw[i] = make_uint4(w.x & keep, w.y & keep, w.z & keep, w.w & keep);
      }
    }
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      const int id = v_piece(i);
      if (V_RAGGED && i == VP - 1 && (id < 256 * i || id >= VPIECES)) break;
      const int j = id % ROWP, d = j / PPR, part = j % PPR;
      const int key = k0 + (id / ROWP) * BS + part * PB;    // first token of the piece
      const uint8_t* src = vbase + (int64_t)vblk[i] * p.kv_block_stride + d * BS + part * PB;
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
      const int c16 = k_c16 + KSTEP * i;
      if (K_RAGGED && i == KP - 1 && c16 >= DT) break;
      uint32_t e[8];
      fp8x4_to_pairs_t<T>(kraw[i].x, e[0], e[1]);
      fp8x4_to_pairs_t<T>(kraw[i].y, e[2], e[3]);
      fp8x4_to_pairs_t<T>(kraw[i].z, e[4], e[5]);
      fp8x4_to_pairs_t<T>(kraw[i].w, e[6], e[7]);
      uint4* dst = reinterpret_cast<uint4*>(&k_s[k_key * KS + c16 * 16]);
      dst[0] = make_uint4(e[0], e[1], e[2], e[3]);
      dst[1] = make_uint4(e[4], e[5], e[6], e[7]);
    }
#pragma unroll
    for (int i = 0; i < VP; ++i) {
      const int id = v_piece(i);
      if (V_RAGGED && i == VP - 1 && (id < 256 * i || id >= VPIECES)) break;
      const int j = id % ROWP, d = j / PPR, part = j % PPR;
      uint32_t e[PB / 2];
#pragma unroll
      for (int w = 0; w < PB / 4; ++w) fp8x4_to_pairs_t<T>(vraw[i][w], e[2 * w], e[2 * w + 1]);
      uint4* dst = reinterpret_cast<uint4*>(&v_s[d * VS + (id / ROWP) * BS + part * PB]);
#pragma unroll
      for (int w = 0; w < PB / 8; ++w) dst[w] = make_uint4(e[4 * w], e[4 * w + 1], e[4 * w + 2], e[4 * w + 3]);
    }
  };
  if (AHEAD) lookup(kt_lo);
  fetch(kt_lo);
  if (AHEAD) lookup(kt_lo + 1);
  park();
  __syncthreads();

  for (int kt = kt_lo; kt < n_kt; ++kt) {
    const int k0 = kt * KT;
    const bool more = kt + 1 < n_kt;                // uniform
    if (more) fetch(kt + 1);                        // raw bytes land in registers while this tile is consumed
    if (AHEAD) lookup(kt + 2);                      // clamped to the sequence: safe past the last tile
    // ---- S^T = K . Q^T: K rows from LDS, shared by the 4 waves ----
    f32x4_t s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const uint16_t* kp = &k_s[(t * 16 + r) * KS];
#pragma unroll
      for (int c = 0; c < DC; ++c)
        s[t] = FaMfma<T>::run(*reinterpret_cast<const uint4*>(kp + c * 32 + g * 8), qf[c], s[t]);
      // the tail accumulates from zero and is added by the VALU (see the header)
      if constexpr (TAIL)
        s[t] += FaMfma<T>::run16(*reinterpret_cast<const uint2*>(kp + DC * 32 + g * 4), qtail, f32x4_t{0.f, 0.f, 0.f, 0.f});
    }
    // ---- scale, mask, online softmax (row = this lane's query) ----
    const bool diag = every_tile || k0 + KT - 1 > ctx + qt0;   // uniform; true on the tile that holds L
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
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
    uint32_t pp[2 * NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
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
    for (int st = 0; st < NS; ++st) {
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
static bool launch_pfx8_wide_bs(const Pfx8Params& p, int block_size, dim3 grid, hipStream_t s) {
  const dim3 block(256);
  switch (block_size) {
    case 8: hipLaunchKernelGGL((prefix_attention_fp8_wide_kernel<T, D, 8>), grid, block, 0, s, p); return true;
    case 16: hipLaunchKernelGGL((prefix_attention_fp8_wide_kernel<T, D, 16>), grid, block, 0, s, p); return true;
    case 32: hipLaunchKernelGGL((prefix_attention_fp8_wide_kernel<T, D, 32>), grid, block, 0, s, p); return true;
    default: return false;
  }
}

bool launch_prefix_fp8_wide(const Pfx8Params& p, bool bf16, int head_size, int block_size, dim3 grid, hipStream_t s) {
  switch (head_size) {
    case 96: return bf16 ? launch_pfx8_wide_bs<BF16, 96>(p, block_size, grid, s) : launch_pfx8_wide_bs<F16, 96>(p, block_size, grid, s);
    case 112: return bf16 ? launch_pfx8_wide_bs<BF16, 112>(p, block_size, grid, s) : launch_pfx8_wide_bs<F16, 112>(p, block_size, grid, s);
    case 192: return bf16 ? launch_pfx8_wide_bs<BF16, 192>(p, block_size, grid, s) : launch_pfx8_wide_bs<F16, 192>(p, block_size, grid, s);
    case 256: return bf16 ? launch_pfx8_wide_bs<BF16, 256>(p, block_size, grid, s) : launch_pfx8_wide_bs<F16, 256>(p, block_size, grid, s);
    default: return false;
  }
}

}  // namespace nmv
