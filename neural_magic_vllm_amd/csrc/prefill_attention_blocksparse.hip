// Block-sparse prompt attention for gfx950 (local + strided blocks, the Phi-3-small pattern): varlen, causal, GQA,
// fp16 / bf16, q / k / v as strided [tokens, heads, head_size] views of the qkv GEMM output.
//
// Rule.  With sb = the sparse block size, qb = i / sb and kb = j / sb, query i of head h attends key j iff j <= i and
//   qb - kb < local_blocks   or   (kb + off_h) % vert_stride == 0,
//   off_h = (tp_rank * H + h) * step + 1            for step >= 0,
//   off_h = (tp_rank * KVH + kv_head(h)) * -step + 1 for step <  0 (homo_head_group: one pattern per GQA group).
// This is the rule of the decode kernel (attention_kernels.hip, paged_attention_kernel's SPARSE branch), so the last
// prompt token of a sequence and its first decode token see the same blocks.  For step >= 0 it is also the prompt mask
// of the reference (vllm/attention/ops/blocksparse_attention/utils.py, get_sparse_attn_mask).  For step < 0 the
// reference's prompt side ignores the group flag and slides per query head; its decode kernel does not.  This kernel
// follows the decode kernel.
// The reference serves such prompts on ROCm with torch SDPA under a dense [H, L, L] bias
// (blocksparse_attention/interface.py); its Triton kernel is CUDA-only.
//
// Maths and register layout are those of prefill_attention_kernel (prefill_attention.hip): S^T = K . Q^T and
// O^T += V^T . P^T on MFMA 16x16x32, fp32 online softmax per lane = per query row, P rounded to the model dtype
// before P.V, masked keys left out of the softmax (-inf).  What is new is WHICH key tiles a workgroup walks:
//
//   * Skip, do not mask.  A workgroup (64 queries of one head of one prompt) owns the query blocks qb_lo .. qb_hi.
//     Their local bands unite to the key blocks band_lo = qb_lo - local + 1 .. qb_hi, a contiguous run of key tiles
//     that ends on the diagonal.  Below it only the strided blocks kb0, kb0 + vs, ... are attended, kb0 =
//     (vs - off % vs) % vs.  visit(t) returns the first key tile >= t that holds a key of one of these blocks, by
//     arithmetic on uniform scalars: no CSR tensor, no host-built layout, no tile is loaded to be masked away.
//   * The K / V tile of the NEXT VISITED tile is fetched into registers while the current one is consumed, and parked
//     in the other LDS buffer; the buffer index flips per visited tile (list order), not with the tile number.
//   * A wave's 16 queries and a 16-key sub-tile each lie inside one sparse block (sb is a multiple of 16), so "does
//     this wave attend this sub-tile" is a wave-uniform bit: am has one bit per sub-tile (block rule, and the sub-tile
//     does not lie wholly past the wave's last query).  A clear bit skips the sub-tile's Q.K^T MFMAs and exps, two
//     clear bits skip the P.V step, am == 0 skips the tile for this wave.  With sb a multiple of 64 every sub-tile of
//     a visited tile passes the block rule, so only the causal part of am is computed.  Inside attended sub-tiles the
//     per-element mask is causal / length only (fa_mask), and only on tiles that reach the wave's diagonal or the
//     end of the prompt.
//   * blockIdx.x counts query tiles from the LAST one down: the work of a query tile grows with its position (the band
//     is constant, the strided part grows), so the heaviest workgroups start first.
//   * Tile sizes, LDS image and waves per SIMD are FaPlan's (fa_common.h); head size 112 keeps the "tail accumulates
//     from zero, VALU adds it" form.
// One K / V tile per workgroup and head: sharing a tile among the heads of a GQA group (possible when step <= 0) is
// not built.
#include "fa_common.h"

namespace nmv {

struct FaBsParams {
  const uint16_t* q;   // [tokens, H, D], token stride q_stride (elements)
  const uint16_t* k;   // [tokens, KVH, D], token stride kv_stride
  const uint16_t* v;
  uint16_t* out;       // [tokens, H, D], token stride o_stride
  const int* cu_seqlens;  // [num_seqs + 1] token offsets of the prompts
  int64_t q_stride, kv_stride, o_stride;
  int num_heads, num_kv_heads;
  float scale;
  int tp_rank, local_blocks, vert_stride;
  int sb_shift;        // log2 of the sparse block size (16, 32, 64, 128)
  int head_sliding_step;
};

template <typename T, int D>
__global__ __launch_bounds__(256, FaPlan<D>::WAVES) void prefill_attention_blocksparse_kernel(const FaBsParams p) {
  static_assert(D % 16 == 0 && D <= 256, "head size");
  constexpr int KT = FaPlan<D>::KT;   // keys per iteration
  constexpr bool DB = FaPlan<D>::DB;
  constexpr int NT = KT / 16;         // 16-key sub-tiles of S
  constexpr int NS = KT / 32;         // 32-key steps of P.V
  constexpr int DC = D / 32;          // whole 32-wide head-dim chunks (MFMA k-steps of Q.K^T)
  constexpr bool TAIL = D % 32 != 0;  // and a 16-wide tail (head size 112): one v_mfma_f32_16x16x16
  constexpr int DT = D / 16;          // 16-wide head-dim tiles of the output
  constexpr int VS = D + 8;           // LDS row stride of a K / V tile (elements): odd multiple of 16 B
  static_assert((VS / 8) % 2 == 1, "row stride must be an odd multiple of 16 bytes");
  constexpr int TILE = KT * VS;       // elements of one tile image
  constexpr int PIECES = KT * D / 8;                // 16-byte pieces of a tile
  constexpr int PPT = (PIECES + 255) / 256;         // pieces per thread
  constexpr bool RAGGED = PIECES % 256 != 0;        // the last round is not whole (D = 112: 3.5 pieces per thread)
  __shared__ __attribute__((aligned(16))) uint16_t kv_s[(DB ? 2 : 1) * 2 * TILE];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int seq = blockIdx.z, head = blockIdx.y;
  const int kv_head = head / (p.num_heads / p.num_kv_heads);
  const int tok0 = p.cu_seqlens[seq];
  const int L = p.cu_seqlens[seq + 1] - tok0;
  const int qt0 = (gridDim.x - 1 - blockIdx.x) * FA_QT;   // heaviest (last) query tiles first
  if (qt0 >= L) return;  // uniform
  const int tr_off = (4 * g + (r >> 2)) * VS + 4 * (r & 3);  // this lane's address role in a tr read
  const int qw0 = qt0 + wave * 16;                  // the wave's first query (prompt-relative)
  const int q_row = qw0 + r;                        // this lane's query

  // ---- the sparsity pattern of this head, in uniform scalars ----
  const int sh = p.sb_shift, vs = p.vert_stride, local = p.local_blocks;
  const int off = p.head_sliding_step >= 0 ? (p.tp_rank * p.num_heads + head) * p.head_sliding_step + 1
                                           : (p.tp_rank * p.num_kv_heads + kv_head) * (-p.head_sliding_step) + 1;
  const int kb0 = (vs - off % vs) % vs;             // first strided block
  const int last_q = min(qt0 + FA_QT, L) - 1;       // causal: keys 0 .. last_q
  const int last_t = last_q / KT;                   // the diagonal tile: always visited (local >= 1)
  const int band_lo = max((qt0 >> sh) - local + 1, 0);   // first key block of the united local bands
  const int band_t = (band_lo << sh) / KT;               // and its key tile
  // first visited key tile >= t (t <= last_t): a band tile, or a tile of a strided block below the band
  auto visit = [&](int t) -> int {
    if (t >= band_t) return t;
    const int kmin = (t * KT) >> sh;                // block of the tile's first key: the first candidate
    int d = kb0 - kmin % vs;
    if (d < 0) d += vs;
    const int kb = kmin + d;                        // first strided block >= kmin
    if (kb >= band_lo) return band_t;
    return min(max(t, (kb << sh) / KT), band_t);
  };
  const bool fine = sh < 6;                         // sparse blocks smaller than the tiles: block rule per sub-tile
  const int qb_w = qw0 >> sh;                       // the wave's query block

  // ---- Q fragment of the wave (B operand of S^T = K . Q^T): 8 head dims per lane and chunk ----
  uint4 qf[DC];
  uint2 qtail;                                      // TAIL: dims D - 16 + 4 g .. + 3
  {
    const uint16_t* qp = p.q + (int64_t)(tok0 + min(q_row, L - 1)) * p.q_stride + (int64_t)head * D + g * 8;
#pragma unroll
    for (int c = 0; c < DC; ++c) qf[c] = ld16(qp + c * 32);
    if constexpr (TAIL) qtail = ld8(qp - g * 4 + DC * 32);
  }
  f32x4_t o[DT];
#pragma unroll
  for (int t = 0; t < DT; ++t) o[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;             // per lane = per query row (l: this lane's share)

  const uint16_t* kbase = p.k + (int64_t)tok0 * p.kv_stride + (int64_t)kv_head * D;
  const uint16_t* vbase = p.v + (int64_t)tok0 * p.kv_stride + (int64_t)kv_head * D;
  const float sc = p.scale;

  // tile loader: thread t owns pieces t, t+256, ... of the K and of the V tile (row = piece / (D/8))
  uint4 kreg[PPT], vreg[PPT];
  auto fetch = [&](int kt) {
    const int k0 = kt * KT;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int id = threadIdx.x + i * 256;
      if (RAGGED && i == PPT - 1 && id >= PIECES) break;
      const int row = id / (D / 8), c8 = id % (D / 8);
      const int64_t off8 = (int64_t)min(k0 + row, L - 1) * p.kv_stride + c8 * 8;   // rows past L: clamped,
      kreg[i] = ld16(kbase + off8);                                                // masked through P = 0
      vreg[i] = ld16(vbase + off8);
    }
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
      const int id = threadIdx.x + i * 256;
      if (RAGGED && i == PPT - 1 && id >= PIECES) break;
      const int row = id / (D / 8), c8 = id % (D / 8);
      *reinterpret_cast<uint4*>(&kv_s[(buf * 2 + 0) * TILE + row * VS + c8 * 8]) = kreg[i];
      *reinterpret_cast<uint4*>(&kv_s[(buf * 2 + 1) * TILE + row * VS + c8 * 8]) = vreg[i];
    }
  };
  int kt = visit(0);
  fetch(kt);
  park(0);
  __syncthreads();

  for (int buf = 0; kt <= last_t; buf ^= DB ? 1 : 0) {
    const int k0 = kt * KT;
    const uint16_t* k_s = &kv_s[(buf * 2 + 0) * TILE];
    const uint16_t* v_s = &kv_s[(buf * 2 + 1) * TILE];
    const int kt_next = kt < last_t ? visit(kt + 1) : last_t + 1;   // uniform
    if (kt_next <= last_t) fetch(kt_next);          // lands in registers while this tile is consumed

    // ---- which 16-key sub-tiles this wave attends: one bit each, wave-uniform ----
    uint32_t am = 0;
    {
      int kb_prev = k0 >> sh;
      int rem = fine ? (kb_prev + off) % vs : 0;    // (block + off) % vs, rolled forward over the sub-tiles
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int key0 = k0 + 16 * t;
        bool a = key0 <= qw0 + 15;                  // not wholly past the wave's last query
        if (fine) {
          const int kb = key0 >> sh;
          if (kb != kb_prev) rem = rem + 1 == vs ? 0 : rem + 1;
          kb_prev = kb;
          a = a && (qb_w - kb < local || rem == 0);
        }
        am |= (a ? 1u : 0u) << t;
      }
    }
    if (am != 0) {                                  // wave-uniform
      // ---- S^T = K . Q^T for the attended sub-tiles: K rows from LDS (shared by the 4 waves) ----
      f32x4_t s[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        s[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (!((am >> t) & 1)) continue;
        const uint16_t* kp = k_s + (t * 16 + r) * VS + g * 8;
#pragma unroll
        for (int c = 0; c < DC; ++c) s[t] = FaMfma<T>::run(*reinterpret_cast<const uint4*>(kp + c * 32), qf[c], s[t]);
        if constexpr (TAIL) {
          // into an accumulator of its own, added by the VALU: chaining a 16x16x16 onto the result of a 16x16x32
          // gave wrong logits on the hardware (see prefill_attention_kernel)
          const uint2 kf = *reinterpret_cast<const uint2*>(kp - g * 4 + DC * 32);
          s[t] += FaMfma<T>::run16(kf, qtail, f32x4_t{0.f, 0.f, 0.f, 0.f});
        }
      }
      // ---- scale, causal / length mask, online softmax (row = this lane's query) ----
      const bool edge = k0 + KT - 1 > qw0 || k0 + KT > L;   // uniform: the tile reaches the wave's diagonal or the end
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const bool att = (am >> t) & 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float x = s[t][i] * sc;
          if (edge) x = fa_mask(x, k0 + t * 16 + 4 * g + i, q_row, L, 0.f, 0);
          if (!att) x = -INFINITY;
          s[t][i] = x;
          mx = fmaxf(mx, x);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float m_new = fmaxf(m_run, mx);
      // a row that has met no key yet (rows past the end of the prompt only: a real row meets its own key in the
      // first sub-tile its wave attends) keeps exp() away from inf - inf
      const float m_use = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __expf(m_run - m_use);
      float psum = 0.f;
      uint32_t pp[2 * NT];                          // packed P: [t][pair]
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (!((am >> t) & 1)) {
          pp[2 * t] = pp[2 * t + 1] = 0u;
          continue;
        }
        float e[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          e[i] = T::to_float(T::from_float(__expf(s[t][i] - m_use)));   // P in the model dtype, and the sum of the same
          psum += e[i];
        }
        pp[2 * t] = T::pack2(e[0], e[1]);
        pp[2 * t + 1] = T::pack2(e[2], e[3]);
      }
      l_run = l_run * alpha + psum;
      m_run = m_new;
#pragma unroll
      for (int t = 0; t < DT; ++t) o[t] *= alpha;
      // ---- O^T += V^T . P^T : NS 32-key steps (skipped when both sub-tiles are unattended), DT output tiles ----
#pragma unroll
      for (int st = 0; st < NS; ++st) {
        if (!((am >> (2 * st)) & 3)) continue;
        const uint4 pb = make_uint4(pp[4 * st], pp[4 * st + 1], pp[4 * st + 2], pp[4 * st + 3]);
#pragma unroll
        for (int t = 0; t < DT; ++t) {
          // A operand: V^T row d = 16 t + r, keys 32 st + {4g..4g+3, 16+4g..16+4g+3}: two transposed LDS reads
          const uint16_t* vp = &v_s[(32 * st) * VS + 16 * t + tr_off];
          const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)vp);
          const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(vp + 16 * VS));
          const uint2 lo2 = __builtin_bit_cast(uint2, lo), hi2 = __builtin_bit_cast(uint2, hi);
          o[t] = FaMfma<T>::run(make_uint4(lo2.x, lo2.y, hi2.x, hi2.y), pb, o[t]);
        }
      }
    }
    if constexpr (DB) {
      if (kt_next <= last_t) park(buf ^ 1);   // the other buffer's readers finished before the last barrier
      __syncthreads();
    } else if (kt_next <= last_t) {           // uniform
      __syncthreads();                        // every wave has read this tile
      park(0);
      __syncthreads();                        // the next one is visible
    }
    kt = kt_next;
  }
  // ---- normalise and store: lane (q = r, g) holds d = 16 t + 4 g + i of its row ----
  float l = l_run;
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (q_row >= L) return;
  const float inv = 1.f / l;
  uint16_t* op = p.out + (int64_t)(tok0 + q_row) * p.o_stride + (int64_t)head * D + 4 * g;
#pragma unroll
  for (int t = 0; t < DT; ++t) {
    uint2 pk;
    pk.x = T::pack2(o[t][0] * inv, o[t][1] * inv);
    pk.y = T::pack2(o[t][2] * inv, o[t][3] * inv);
    *reinterpret_cast<uint2*>(op + 16 * t) = pk;
  }
}

}  // namespace nmv

using namespace nmv;

extern "C" int nmv_prefill_attention_supported(int head_size);
extern "C" int nmv_prefill_attention(void* out, const void* q, const void* k, const void* v,
                                     const int32_t* cu_seqlens, int num_seqs, int max_seq_len,
                                     int num_heads, int num_kv_heads, int head_size, float scale,
                                     int64_t q_stride, int64_t kv_stride, int64_t o_stride,
                                     const float* alibi_slopes, int sliding_window,
                                     nmv_dtype_t dtype, void* stream);

extern "C" int nmv_prefill_attention_blocksparse(void* out, const void* q, const void* k, const void* v,
                                                 const int32_t* cu_seqlens, int num_seqs, int max_seq_len,
                                                 int num_heads, int num_kv_heads, int head_size, float scale,
                                                 int64_t q_stride, int64_t kv_stride, int64_t o_stride,
                                                 int tp_rank, int blocksparse_local_blocks,
                                                 int blocksparse_vert_stride, int blocksparse_block_size,
                                                 int blocksparse_head_sliding_step, nmv_dtype_t dtype, void* stream) {
  if (blocksparse_vert_stride <= 1)   // every block is attended: the dense kernel, with its own checks
    return nmv_prefill_attention(out, q, k, v, cu_seqlens, num_seqs, max_seq_len, num_heads, num_kv_heads, head_size,
                                 scale, q_stride, kv_stride, o_stride, nullptr, 0, dtype, stream);
  NMV_CHECK(dtype == NMV_F16 || dtype == NMV_BF16, "prefill_attention_blocksparse: fp16 / bf16 only");
  NMV_CHECK(nmv_prefill_attention_supported(head_size),
            "prefill_attention_blocksparse: head size %d not built (64, 96, 112, 128, 192, 256)", head_size);
  NMV_CHECK(num_kv_heads > 0 && num_heads % num_kv_heads == 0, "prefill_attention_blocksparse: heads %% kv_heads != 0");
  NMV_CHECK(q_stride % 8 == 0 && kv_stride % 8 == 0 && o_stride % 4 == 0,
            "prefill_attention_blocksparse: token strides must keep 16-byte (q, k, v) / 8-byte (out) alignment");
  NMV_CHECK(blocksparse_local_blocks >= 1,
            "prefill_attention_blocksparse: local_blocks %d < 1 (a query could attend to nothing, not even itself)",
            blocksparse_local_blocks);
  NMV_CHECK(blocksparse_block_size == 16 || blocksparse_block_size == 32 || blocksparse_block_size == 64 ||
            blocksparse_block_size == 128,
            "prefill_attention_blocksparse: sparse block size %d (16, 32, 64, 128)", blocksparse_block_size);
  NMV_CHECK(tp_rank >= 0, "prefill_attention_blocksparse: tp_rank %d", tp_rank);
  if (num_seqs <= 0 || max_seq_len <= 0) return NMV_OK;
  FaBsParams p{(const uint16_t*)q, (const uint16_t*)k, (const uint16_t*)v, (uint16_t*)out, cu_seqlens,
               q_stride, kv_stride, o_stride, num_heads, num_kv_heads, scale, tp_rank, blocksparse_local_blocks,
               blocksparse_vert_stride, __builtin_ctz((unsigned)blocksparse_block_size), blocksparse_head_sliding_step};
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((max_seq_len + FA_QT - 1) / FA_QT, num_heads, num_seqs), block(256);
#define NMV_FABS_LAUNCH(T_, D_) hipLaunchKernelGGL((prefill_attention_blocksparse_kernel<T_, D_>), grid, block, 0, s, p);
#define NMV_FABS_HEADS(T_)                                  \
  switch (head_size) {                                      \
    case 64: NMV_FABS_LAUNCH(T_, 64) break;                 \
    case 96: NMV_FABS_LAUNCH(T_, 96) break;                 \
    case 112: NMV_FABS_LAUNCH(T_, 112) break;               \
    case 128: NMV_FABS_LAUNCH(T_, 128) break;               \
    case 192: NMV_FABS_LAUNCH(T_, 192) break;               \
    default: NMV_FABS_LAUNCH(T_, 256) break;                \
  }
  if (dtype == NMV_BF16) NMV_FABS_HEADS(BF16) else NMV_FABS_HEADS(F16)
#undef NMV_FABS_HEADS
#undef NMV_FABS_LAUNCH
  NMV_LAUNCH_CHECK();
  return NMV_OK;
}
