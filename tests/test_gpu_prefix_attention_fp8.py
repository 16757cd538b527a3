"""GPU parity of prefix-enabled prompt attention on an fp8 (e4m3) KV cache (csrc/prefix_attention_fp8.hip)
against plain fp32 causal attention on the CPU over the values the cache actually holds (its bytes read back,
viewed as e4m3, times kv_scale).  Geometry and tolerances are those of test_prefix_prefill_attention: widening
e4m3 to fp16 / bf16 is exact and kv_scale is folded in fp32, so the error sources are the same."""
import itertools

import pytest
import torch

from test_gpu_prefill_attention import _slopes, ref_attention

pytestmark = pytest.mark.gpu

SEQ_LENS = [70, 33, 257, 16]
Q_LENS = [6, 33, 65, 1]            # context: 64, 0, 192, 15 tokens
KV_SCALE = 1.5                     # not a power of two: a missing or misplaced scale shows
NUM_BLOCKS = 256


def cached_kv(kc, vc, slots, block_size):
    """what the uint8 cache holds at `slots`, dequantised: k, v [tokens, KVH, D] fp32 on the CPU"""
    kq = kc.cpu().view(torch.float8_e4m3fn).float() * KV_SCALE       # [NB, KVH, D/16, BS, 16]
    vq = vc.cpu().view(torch.float8_e4m3fn).float() * KV_SCALE       # [NB, KVH, D, BS]
    blk, off = slots.cpu() // block_size, slots.cpu() % block_size
    k = kq[blk, :, :, off, :]                                         # [tokens, KVH, D/16, 16]
    return k.reshape(k.shape[0], k.shape[1], -1), vq[blk, :, :, off]


def last_rows(x, seq_lens, q_lens):
    """the last q_len rows of every sequence of a [sum(seq_lens), ...] tensor"""
    ends = torch.tensor(seq_lens).cumsum(0).tolist()
    return torch.cat([x[e - ql:e] for e, ql in zip(ends, q_lens)])


def check(got, ref, dtype):
    got = got.float().cpu()
    assert not torch.isnan(got).any()
    tol = 2e-3 if dtype == torch.half else 1.6e-2
    torch.testing.assert_close(got, ref, atol=tol, rtol=tol)


CASES = [c + ((8, 2), ) for c in itertools.product([torch.half, torch.bfloat16], [64, 128], [8, 16, 32],
                                                   [(False, None), (True, 40)])] + \
        [(torch.half, 64, 8, (False, None), (4, 4)), (torch.bfloat16, 128, 16, (True, 40), (4, 4)),
         (torch.half, 128, 32, (True, 40), (4, 4)), (torch.bfloat16, 64, 16, (False, None), (4, 4))]


@pytest.mark.parametrize("dtype,head_size,block_size,bias,heads", CASES)
def test_prefix_prefill_attention_fp8(gpu_device, dtype, head_size, block_size, bias, heads):
    """a full 64-key context tile, no context, three context tiles + a one-row second query tile + a one-key
    last tile, one partial tile; lengths that are no multiple of 4; a window shorter than a tile; the cache
    pre-filled with 0xFF (fp8 NaN) behind and between the sequences; permuted block table"""
    from neural_magic_vllm_amd import _custom_ops as ops
    import helpers
    (alibi, window), (nq, nkv) = bias, heads
    dev = gpu_device
    g = torch.Generator().manual_seed(1)
    total, scale = sum(SEQ_LENS), head_size**-0.5
    q_all = (torch.rand((total, nq, head_size), generator=g) * 2 - 1).to(dtype)
    k_all = (torch.rand((total, nkv, head_size), generator=g) * 2 - 1).to(dtype)
    v_all = (torch.rand((total, nkv, head_size), generator=g) * 2 - 1).to(dtype)
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


@pytest.mark.parametrize("dtype", [torch.half, torch.bfloat16])
def test_backend_chunked_prefill_on_fp8_cache(gpu_device, dtype):
    """ROCmHipAttentionImpl.forward with kv_cache_dtype fp8: the first chunk of every prompt goes through the
    plain prompt path (which writes it to the cache), the second is a prompt-only batch with a non-zero
    context and must match attention over the cached (quantised) keys and values of both chunks"""
    from neural_magic_vllm_amd.attention.backends.rocm_hip_attn import (ROCmHipAttentionBackend, ROCmHipAttentionImpl,
                                                                        ROCmHipAttentionMetadata)
    from neural_magic_vllm_amd.attention.ops.paged_attn import PagedAttention
    dev, nq, nkv, d, bs = gpu_device, 8, 2, 128, 16
    seq_lens, firsts = [100, 37], [64, 20]
    impl = ROCmHipAttentionImpl(nq, d, d**-0.5, nkv, kv_cache_dtype="fp8")
    g = torch.Generator().manual_seed(2)
    total = sum(seq_lens)
    q_all, k_all, v_all = ((torch.rand((total, n * d), generator=g) * 2 - 1).to(dtype) for n in (nq, nkv, nkv))
    kv_cache = torch.full(ROCmHipAttentionBackend.get_kv_cache_shape(32, bs, nkv, d), 0xFF, dtype=torch.uint8,
                          device=dev)
    tables = torch.randperm(32, generator=g)[:2 * 7].view(2, 7).to(torch.int32)
    starts = [0, seq_lens[0]]

    def chunk(los, his):
        rows = torch.cat([torch.arange(s + lo, s + hi) for s, lo, hi in zip(starts, los, his)])
        slots = torch.cat([tables[i][torch.arange(lo, hi) // bs].long() * bs + torch.arange(lo, hi) % bs
                           for i, (lo, hi) in enumerate(zip(los, his))])
        lens = [hi - lo for lo, hi in zip(los, his)]
        cu = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32, device=dev)
        md = ROCmHipAttentionMetadata(
            num_prefills=2, num_prefill_tokens=sum(lens), num_decode_tokens=0, slot_mapping=slots.to(dev),
            seq_lens=list(his), seq_lens_tensor=torch.tensor(his, dtype=torch.int32, device=dev),
            max_query_len=max(lens), max_prefill_seq_len=max(his), max_decode_seq_len=0, query_start_loc=cu,
            seq_start_loc=cu if max(los) == 0 else None,
            context_lens_tensor=torch.tensor(los, dtype=torch.int32, device=dev), block_tables=tables.to(dev),
            use_cuda_graph=False)
        out = impl.forward(q_all[rows].to(dev), k_all[rows].to(dev), v_all[rows].to(dev), kv_cache, md, KV_SCALE)
        return rows, slots, out

    chunk([0, 0], firsts)
    rows, _, out = chunk(firsts, seq_lens)
    all_slots = torch.cat([tables[i][torch.arange(L) // bs].long() * bs + torch.arange(L) % bs
                           for i, L in enumerate(seq_lens)])
    k_deq, v_deq = cached_kv(*PagedAttention.split_kv_cache(kv_cache, nkv, d), all_slots, bs)
    ref = ref_attention(q_all.float().view(total, nq, d), k_deq, v_deq, seq_lens, d**-0.5)
    check(out.view(-1, nq, d), ref[rows], dtype)


@pytest.mark.parametrize("kv_cache_dtype,head_size", [("fp8_e5m2", 128), ("fp8", 80)])
def test_prefix_prefill_attention_fp8_rejects(gpu_device, kv_cache_dtype, head_size):
    from neural_magic_vllm_amd import _custom_ops as ops
    from neural_magic_vllm_amd._lib import NmvError
    import helpers
    q = torch.zeros((4, 2, head_size), dtype=torch.half, device=gpu_device)
    kshape, vshape = helpers.kv_cache_shapes(4, 16, 2, head_size, 1)
    kc = torch.zeros(kshape, dtype=torch.uint8, device=gpu_device)
    vc = torch.zeros(vshape, dtype=torch.uint8, device=gpu_device)
    i32 = dict(dtype=torch.int32, device=gpu_device)
    with pytest.raises(NmvError):
        ops.prefix_prefill_attention(torch.empty_like(q), q, kc, vc, torch.zeros((1, 1), **i32),
                                     torch.tensor([0, 4], **i32), torch.tensor([4], **i32), torch.tensor([0], **i32),
                                     4, 1.0, None, None, kv_cache_dtype, 1.0)
