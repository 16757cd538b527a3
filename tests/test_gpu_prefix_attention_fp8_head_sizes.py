"""GPU parity of prefix-enabled prompt attention on an fp8 (e4m3) KV cache at head sizes 96, 112, 192 and 256
(csrc/prefix_attention_fp8_wide.hip) against plain fp32 causal attention on the CPU over the values the cache
actually holds.  Recipe, lengths and tolerances are those of test_gpu_prefix_attention_fp8 (64 / 128): 2e-3 for
half and 1.6e-2 for bfloat16, what the 16-bit kernels are held to at these head sizes -- widening e4m3 is exact."""
import itertools

import pytest
import torch

from test_gpu_prefill_attention import _slopes, ref_attention
from test_gpu_prefix_attention_fp8 import KV_SCALE, Q_LENS, SEQ_LENS, cached_kv, check, last_rows

pytestmark = pytest.mark.gpu

NUM_BLOCKS = 256
HEAD_SIZES = [96, 112, 192, 256]
CASES = [c + ((False, None), (8, 2)) for c in itertools.product([torch.half, torch.bfloat16], HEAD_SIZES, [8, 16, 32])] + \
        [(torch.half, 96, 16, (True, 40), (8, 2)), (torch.bfloat16, 112, 8, (True, 40), (8, 2)),
         (torch.half, 192, 32, (True, 40), (8, 2)), (torch.bfloat16, 256, 16, (True, 40), (8, 2)),
         (torch.half, 112, 16, (False, None), (4, 4))]


@pytest.mark.parametrize("dtype,head_size,block_size,bias,heads", CASES)
def test_prefix_prefill_attention_fp8_head_sizes(gpu_device, dtype, head_size, block_size, bias, heads):
    """a full 64-key context tile, no context, several tiles + a one-row second query tile + a one-key last tile
    (257 = 4 * 64 + 1), one partial tile; a window shorter than a tile; the cache pre-filled with 0xFF (fp8 NaN)
    behind and between the sequences; permuted block table"""
    from neural_magic_vllm_amd import _custom_ops as ops
    import helpers
    (alibi, window), (nq, nkv) = bias, heads
    dev = gpu_device
    g = torch.Generator().manual_seed(1)
    total, scale = sum(SEQ_LENS), head_size**-0.5
    q_all, k_all, v_all = ((torch.rand((total, n, head_size), generator=g) * 2 - 1).to(dtype) for n in (nq, nkv, nkv))
    max_blocks = (max(SEQ_LENS) + block_size - 1) // block_size
    perm = torch.randperm(NUM_BLOCKS, generator=g)[:len(SEQ_LENS) * max_blocks].view(len(SEQ_LENS), max_blocks)
    kshape, vshape = helpers.kv_cache_shapes(NUM_BLOCKS, block_size, nkv, head_size, 1)
    kc = torch.full(kshape, 0xFF, dtype=torch.uint8, device=dev)
    vc = torch.full(vshape, 0xFF, dtype=torch.uint8, device=dev)
    slots = torch.cat([perm[i][torch.arange(L) // block_size] * block_size + torch.arange(L) % block_size
                       for i, L in enumerate(SEQ_LENS)]).to(torch.int64).to(dev)
    ops.reshape_and_cache(k_all.to(dev), v_all.to(dev), kc, vc, slots, "fp8", KV_SCALE)
    q_new = last_rows(q_all, SEQ_LENS, Q_LENS).to(dev)
    out = torch.full_like(q_new, float("nan"))
    qsl = torch.tensor([0] + torch.tensor(Q_LENS).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    sl = torch.tensor(SEQ_LENS, dtype=torch.int32, device=dev)
    cl = torch.tensor([L - ql for L, ql in zip(SEQ_LENS, Q_LENS)], dtype=torch.int32, device=dev)
    slopes = _slopes(nq) if alibi else None
    ops.prefix_prefill_attention(out, q_new, kc, vc, perm.to(torch.int32).to(dev), qsl, sl, cl, max(Q_LENS), scale,
                                 slopes.to(dev) if alibi else None, window, "fp8", KV_SCALE)
    k_deq, v_deq = cached_kv(kc, vc, slots, block_size)
    ref = ref_attention(q_all.float(), k_deq, v_deq, SEQ_LENS, scale, slopes, window)
    check(out, last_rows(ref, SEQ_LENS, Q_LENS), dtype)


@pytest.mark.parametrize("dtype,d", [(torch.half, 96), (torch.bfloat16, 256)])
def test_backend_chunked_prefill_on_fp8_cache_head_sizes(gpu_device, dtype, d):
    """ROCmHipAttentionImpl.forward with kv_cache_dtype fp8, a prompt in two chunks: the second is a prompt-only
    batch with a non-zero context and must match attention over the cached values of both chunks"""
    from neural_magic_vllm_amd.attention.backends.rocm_hip_attn import (ROCmHipAttentionBackend, ROCmHipAttentionImpl,
                                                                        ROCmHipAttentionMetadata)
    from neural_magic_vllm_amd.attention.ops.paged_attn import PagedAttention
    dev, nq, nkv, bs = gpu_device, 8, 2, 16
    seq_lens, firsts, starts = [100, 37], [64, 20], [0, 100]
    impl = ROCmHipAttentionImpl(nq, d, d**-0.5, nkv, kv_cache_dtype="fp8")
    g = torch.Generator().manual_seed(2)
    total = sum(seq_lens)
    q_all, k_all, v_all = ((torch.rand((total, n * d), generator=g) * 2 - 1).to(dtype) for n in (nq, nkv, nkv))
    kv_cache = torch.full(ROCmHipAttentionBackend.get_kv_cache_shape(32, bs, nkv, d), 0xFF, dtype=torch.uint8,
                          device=dev)
    tables = torch.randperm(32, generator=g)[:2 * 7].view(2, 7).to(torch.int32)

    def slots_of(los, his):
        return torch.cat([tables[i][torch.arange(lo, hi) // bs].long() * bs + torch.arange(lo, hi) % bs
                          for i, (lo, hi) in enumerate(zip(los, his))])

    def chunk(los, his):
        rows = torch.cat([torch.arange(s + lo, s + hi) for s, lo, hi in zip(starts, los, his)])
        lens = [hi - lo for lo, hi in zip(los, his)]
        cu = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32, device=dev)
        md = ROCmHipAttentionMetadata(
            num_prefills=2, num_prefill_tokens=sum(lens), num_decode_tokens=0, slot_mapping=slots_of(los, his).to(dev),
            seq_lens=list(his), seq_lens_tensor=torch.tensor(his, dtype=torch.int32, device=dev),
            max_query_len=max(lens), max_prefill_seq_len=max(his), max_decode_seq_len=0, query_start_loc=cu,
            seq_start_loc=cu if max(los) == 0 else None,
            context_lens_tensor=torch.tensor(los, dtype=torch.int32, device=dev), block_tables=tables.to(dev),
            use_cuda_graph=False)
        return rows, impl.forward(q_all[rows].to(dev), k_all[rows].to(dev), v_all[rows].to(dev), kv_cache, md, KV_SCALE)

    chunk([0, 0], firsts)
    rows, out = chunk(firsts, seq_lens)
    k_deq, v_deq = cached_kv(*PagedAttention.split_kv_cache(kv_cache, nkv, d), slots_of([0, 0], seq_lens), bs)
    ref = ref_attention(q_all.float().view(total, nq, d), k_deq, v_deq, seq_lens, d**-0.5)
    check(out.view(-1, nq, d), ref[rows], dtype)
