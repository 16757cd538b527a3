// Prefix-enabled prompt attention (chunked prefill / prefix caching) on a 16-bit KV cache for the head sizes
// beyond 64 / 128 -- 96, 112, 192 and 256 -- for gfx950.
//
// Same contract and maths as prefix_attention_kernel (prefill_attention.hip): the new tokens of a sequence attend
// causally to ALL its keys, context and new, read from the paged cache; S^T = K . Q^T and O^T += V^T . P^T on
// v_mfma_f32_16x16x32, fp32 online softmax per lane, P rounded to the model dtype, fa_mask; one 256-thread
// workgroup per (64-query tile, head, sequence), 16 query rows per wave, tiles wholly before the window skipped.
//
// What differs is the data path.  prefix_attention_kernel uses no LDS: each of the four waves loads the same cache
// lines straight into MFMA operands, and that four-fold load grows with the head size.  Here the workgroup
// gathers a tile ONCE and shares it, the way prefix_attention_fp8_kernel does:
//   gather   16-byte pieces through the block table.  K plane [NB, KVH, D/8, BS, 8]: a piece is 8 head dims of
//            one key; consecutive threads take consecutive keys (contiguous within a block), so a thread keeps one
//            key and reads the block table once per tile.  V plane [NB, KVH, D, BS]: a piece is 8 consecutive
//            tokens of one head dim; pieces are numbered in memory order (token part, head dim, block), so a
//            block's D x BS plane is read as one contiguous run.  8 divides every block size, so no piece crosses
//            a block.  The key is clamped to the sequence BEFORE the block table is read; pieces (K) and elements
//            (V) of keys at or past its end are cleared, because the cache behind a sequence is uninitialised and
//            0 x NaN would poison a row through V.
//   stage    K row-major per key, row stride D + 8 elements (an odd multiple of 16 bytes): the A operand of S^T is
//            one conflict-free ds_read_b128 per (key, 32-dim chunk).  V as V^T, head dim major, KT keys per row,
//            row stride KT + 8 elements (36 or 20 dwords): the A operand of O^T is two ds_read_b64 of keys
//            {4g..4g+3} and {16+4g..16+4g+3}, and a half-wave covers the 64 banks exactly once.  The cache already
//            holds V transposed, so no transposed LDS read is needed.
//   overlap  the pieces of tile kt+1 are fetched into registers before the MFMAs of tile kt and parked after
//            them, between two barriers (one K + V^T image; the LDS saved keeps more workgroups on a CU, and their
//            MFMAs cover this one's barriers).
//   tail     head size 112 leaves a 16-wide rest of the 32-wide k-steps of S^T: one v_mfma_f32_16x16x16
//            (FaMfma::run16), whose accumulator layout is that of the 32-wide step.
//
// Keys per iteration: 64 while one K image and one V^T image stay within a budget of 64 KiB -- D = 192 is the
// tightest, 64 * 200 * 2 + 192 * 72 * 2 = 53248 B -- else 32: D = 256 takes 32 * 264 * 2 + 256 * 40 * 2 = 37376 B.
// The budget is a choice, not a compiler limit (gfx950 accepts more static LDS per workgroup): 64 keys at D = 256
// would be 70656 B and would double the register prefetch to 64 VGPRs; what that does is recorded in DESIGN.md 3.8,
// with the launch bounds and the -Rpass-analysis=kernel-resource-usage lines.
#include "fa_common.h"

namespace nmv {

template <int D> struct PfxPlan {
  static constexpr int lds_bytes(int kt) { return (kt * (D + 8) + D * (kt + 8)) * 2; }
  static constexpr int KT = lds_bytes(64) <= 65536 ? 64 : 32;   // keys per iteration
  // waves per SIMD asked of the register allocator: the highest that leaves no scratch
  static constexpr int WAVES = D <= 128 ? 3 : 2;
};

// both elements, the low one or neither of a dword of two 16-bit elements, by how many (n) are valid
__device__ __forceinline__ uint32_t low_halves(int n) { return n >= 2 ? 0xffffffffu : (n == 1 ? 0xffffu : 0u); }

template <typename T, int D, int BS>
__global__ __launch_bounds__(256, PfxPlan<D>::WAVES) void prefix_attention_staged_kernel(const PfxParams p) {
  static_assert(D % 16 == 0 && D <= 256, "head size");
  static_assert(BS == 8 || BS == 16 || BS == 32, "block size");
  constexpr int KT = PfxPlan<D>::KT;
  constexpr int NT = KT / 16;               // 16-key tiles of S
  constexpr int NS = KT / 32;               // 32-key steps of P.V
  constexpr int DC = D / 32, DT = D / 16;
  constexpr bool TAIL = D % 32 != 0;
  constexpr int KS = D + 8;                 // K image: elements per key row
  constexpr int VS = KT + 8;                // V^T image: elements per head-dim row
  static_assert((KS / 8) % 2 == 1 && KT % BS == 0, "K row stride / whole blocks per tile");
  constexpr int PIECES = KT * D / 8;        // 16-byte pieces of the K tile, and of the V tile
  constexpr int PPT = (PIECES + 255) / 256; // pieces per thread
  constexpr bool RAGGED = PIECES % 256 != 0;   // D = 112: 3.5 pieces per thread, the last round is guarded
  constexpr int KSTEP = 256 / KT;           // K: 8-dim chunks between a thread's pieces
  constexpr int PPR = BS / 8;               // V pieces per (head dim, block)
  constexpr int ROWP = D * PPR;             // V pieces per block
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
  const uint16_t* kbase = p.kc + (int64_t)kv_head * p.kv_head_stride;
  const uint16_t* vbase = p.vc + (int64_t)kv_head * p.kv_head_stride;

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
  const float sc = p.scale;
  const float slope = p.alibi_slopes ? p.alibi_slopes[head] : 0.f;
  const bool every_tile = p.window > 0 || slope != 0.f;   // uniform

  // ---- tile loader.  K: thread t owns key t % KT, 8-dim chunks t / KT + KSTEP i.  V: piece id = t + 256 i is
  // (block of the tile, head dim, 8-token part of the block), part fastest ----
  const int k_key = threadIdx.x % KT, k_c8 = threadIdx.x / KT;
  uint4 kreg[PPT], vreg[PPT];
  auto fetch = [&](int kt) {
    const int k0 = kt * KT;
    {
      const int key = k0 + k_key;
      const int kc = min(key, L - 1);       // clamp BEFORE the block table: entries past the last block are not read
      const uint16_t* src = kbase + (int64_t)bt[kc / BS] * p.kv_block_stride + (kc % BS) * 8;
      const uint32_t keep = key < L ? 0xffffffffu : 0u;
#pragma unroll
      for (int i = 0; i < PPT; ++i) {
        const int c8 = k_c8 + KSTEP * i;
        if (RAGGED && i == PPT - 1 && c8 >= D / 8) break;
        const uint4 w = ld16(src + c8 * (BS * 8));
        kreg[i] = make_uint4(w.x & keep, w.y & keep, w.z & keep, w.w & keep);
      }
    }
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int id = threadIdx.x + i * 256;
      if (RAGGED && i == PPT - 1 && id >= PIECES) break;
      const int j = id % ROWP, d = j / PPR, part = j % PPR;
      const int key = k0 + (id / ROWP) * BS + part * 8;    // first token of the piece
      const int kc = min(key, L - 1);
      const uint4 w = ld16(vbase + (int64_t)bt[kc / BS] * p.kv_block_stride + d * BS + part * 8);
      const int valid = L - key;            // tokens of the piece inside the sequence (may be <= 0 or >= 8)
      vreg[i] = make_uint4(w.x & low_halves(valid), w.y & low_halves(valid - 2), w.z & low_halves(valid - 4),
                           w.w & low_halves(valid - 6));
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int c8 = k_c8 + KSTEP * i;
      if (RAGGED && i == PPT - 1 && c8 >= D / 8) break;
      *reinterpret_cast<uint4*>(&k_s[k_key * KS + c8 * 8]) = kreg[i];
    }
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int id = threadIdx.x + i * 256;
      if (RAGGED && i == PPT - 1 && id >= PIECES) break;
      const int j = id % ROWP, d = j / PPR, part = j % PPR;
      *reinterpret_cast<uint4*>(&v_s[d * VS + (id / ROWP) * BS + part * 8]) = vreg[i];
    }
  };
  fetch(kt_lo);
  park();
  __syncthreads();

  for (int kt = kt_lo; kt < n_kt; ++kt) {
    const int k0 = kt * KT;
    const bool more = kt + 1 < n_kt;                // uniform
    if (more) fetch(kt + 1);                        // lands in registers while this tile is consumed
    // ---- S^T = K . Q^T: K rows from LDS, shared by the 4 waves ----
    f32x4_t s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      const uint16_t* kp = &k_s[(t * 16 + r) * KS];
#pragma unroll
      for (int c = 0; c < DC; ++c)
        s[t] = FaMfma<T>::run(*reinterpret_cast<const uint4*>(kp + c * 32 + g * 8), qf[c], s[t]);
      // the tail accumulates from zero and is added by the VALU (see prefill_attention_kernel)
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
  const float inv = 1.f / l_run;
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
static bool launch_staged_bs(const PfxParams& p, dim3 grid, hipStream_t s) {
  const dim3 block(256);
  switch (p.block_size) {
    case 8: hipLaunchKernelGGL((prefix_attention_staged_kernel<T, D, 8>), grid, block, 0, s, p); return true;
    case 16: hipLaunchKernelGGL((prefix_attention_staged_kernel<T, D, 16>), grid, block, 0, s, p); return true;
    case 32: hipLaunchKernelGGL((prefix_attention_staged_kernel<T, D, 32>), grid, block, 0, s, p); return true;
    default: return false;
  }
}

bool launch_prefix_staged(const PfxParams& p, bool bf16, int head_size, dim3 grid, hipStream_t s) {
  switch (head_size) {
    case 96: return bf16 ? launch_staged_bs<BF16, 96>(p, grid, s) : launch_staged_bs<F16, 96>(p, grid, s);
    case 112: return bf16 ? launch_staged_bs<BF16, 112>(p, grid, s) : launch_staged_bs<F16, 112>(p, grid, s);
    case 192: return bf16 ? launch_staged_bs<BF16, 192>(p, grid, s) : launch_staged_bs<F16, 192>(p, grid, s);
    case 256: return bf16 ? launch_staged_bs<BF16, 256>(p, grid, s) : launch_staged_bs<F16, 256>(p, grid, s);
    default: return false;
  }
}

}  // namespace nmv
