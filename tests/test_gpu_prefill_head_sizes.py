"""GPU parity of prompt attention at head sizes 96, 112, 192 and 256 against plain fp32 causal attention on the
CPU: the varlen prompt kernel (csrc/prefill_attention.hip: 32 keys per iteration at 192 / 256, one LDS buffer at
256, the 16-wide MFMA tail and the ragged tile loader at 112), the staged 16-bit prefix kernel
(csrc/prefix_attention_staged.hip) and the backend branches that reach them.  Tolerances are those of
test_gpu_prefill_attention.py: P and the output are rounded to the model dtype, and the error does not grow with
the head size."""
import pytest
import torch

from test_gpu_prefill_attention import _slopes, ref_attention

pytestmark = pytest.mark.gpu

HEAD_SIZES = [96, 112, 192, 256]
DTYPES = [torch.half, torch.bfloat16]


def check(got, ref, dtype):
    got = got.float().cpu()
    assert not torch.isnan(got).any()
    tol = 2e-3 if dtype == torch.half else 1.6e-2
    torch.testing.assert_close(got, ref, atol=tol, rtol=tol)


def cu_of(lens, dev):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("heads", [(8, 2), (4, 4)])
@pytest.mark.parametrize("head_size", HEAD_SIZES)
@pytest.mark.parametrize("seq_lens", [[1], [37, 64, 1, 200], [33, 65, 129]])
def test_prefill_attention_head_sizes(gpu_device, dtype, heads, head_size, seq_lens):
    """a lone token; prompts ending inside, on and just past a 32- and a 64-key tile; several tiles and a ragged
    last query tile; q, k and v as strided slices of one qkv tensor"""
    from neural_magic_vllm_amd import _custom_ops as ops
    (nq, nkv), d, t = heads, head_size, sum(seq_lens)
    g = torch.Generator().manual_seed(0)
    qkv = (torch.rand((t, (nq + 2 * nkv) * d), generator=g) * 2 - 1).to(dtype)
    q, k, v = (x.view(t, -1, d) for x in qkv.to(gpu_device).split([nq * d, nkv * d, nkv * d], dim=-1))
    out = torch.full((t, nq, d), float("nan"), dtype=dtype, device=gpu_device)
    ops.prefill_attention(out, q, k, v, cu_of(seq_lens, gpu_device), max(seq_lens), d**-0.5)
    qc, kc, vc = (x.view(t, -1, d) for x in qkv.float().split([nq * d, nkv * d, nkv * d], dim=-1))
    check(out, ref_attention(qc, kc, vc, seq_lens, d**-0.5), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_size", [112, 256])
@pytest.mark.parametrize("alibi,window", [(True, None), (False, 40), (True, 100), (False, 1)])
def test_prefill_attention_head_sizes_alibi_and_window(gpu_device, dtype, head_size, alibi, window):
    """windows shorter and longer than either tile width; at 256 a window of 40 spans two 32-key tiles, so the
    tiles before it are skipped"""
    from neural_magic_vllm_amd import _custom_ops as ops
    nq, nkv, d, seq_lens = 8, 2, head_size, [300, 17, 129, 64]
    t = sum(seq_lens)
    g = torch.Generator().manual_seed(3)
    q, k, v = ((torch.rand((t, n, d), generator=g) * 2 - 1).to(dtype) for n in (nq, nkv, nkv))
    slopes = _slopes(nq) if alibi else None
    out = torch.full((t, nq, d), float("nan"), dtype=dtype, device=gpu_device)
    ops.prefill_attention(out, q.to(gpu_device), k.to(gpu_device), v.to(gpu_device), cu_of(seq_lens, gpu_device),
                          max(seq_lens), d**-0.5, slopes.to(gpu_device) if alibi else None, window)
    check(out, ref_attention(q.float(), k.float(), v.float(), seq_lens, d**-0.5, slopes, window), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_size", HEAD_SIZES)
@pytest.mark.parametrize("block_size", [8, 16, 32])
@pytest.mark.parametrize("alibi,window", [(False, None), (True, 40)])
def test_prefix_prefill_attention_head_sizes(gpu_device, dtype, head_size, block_size, alibi, window):
    """the geometry of test_prefix_prefill_attention: contexts of 64, 0, 192 and 15 tokens, a shuffled block table,
    caches pre-filled with NaN and written by reshape_and_cache"""
    from neural_magic_vllm_amd import _custom_ops as ops
    import helpers
    nq, nkv, d, dev = 8, 2, head_size, gpu_device
    seq_lens, q_lens = [70, 33, 257, 16], [6, 33, 65, 1]
    g = torch.Generator().manual_seed(1)
    total = sum(seq_lens)
    q_all, k_all, v_all = ((torch.rand((total, n, d), generator=g) * 2 - 1).to(dtype) for n in (nq, nkv, nkv))
    nb = 256
    max_blocks = (max(seq_lens) + block_size - 1) // block_size
    perm = torch.randperm(nb, generator=g)[:len(seq_lens) * max_blocks].view(len(seq_lens), max_blocks)
    kshape, vshape = helpers.kv_cache_shapes(nb, block_size, nkv, d, 2)
    kc = torch.full(kshape, float("nan"), dtype=dtype, device=dev)   # garbage outside the sequences
    vc = torch.full(vshape, float("nan"), dtype=dtype, device=dev)
    slots = torch.cat([perm[i][torch.arange(L) // block_size] * block_size + torch.arange(L) % block_size
                       for i, L in enumerate(seq_lens)]).to(torch.int64).to(dev)
    ops.reshape_and_cache(k_all.to(dev), v_all.to(dev), kc, vc, slots, "auto", 1.0)
    ends = torch.tensor(seq_lens).cumsum(0).tolist()
    rows = torch.cat([torch.arange(e - ql, e) for e, ql in zip(ends, q_lens)])   # the last q_len tokens of each
    q_new = q_all[rows].to(dev)
    out = torch.full_like(q_new, float("nan"))
    sl = torch.tensor(seq_lens, dtype=torch.int32, device=dev)
    cl = torch.tensor([L - ql for L, ql in zip(seq_lens, q_lens)], dtype=torch.int32, device=dev)
    slopes = _slopes(nq) if alibi else None
    ops.prefix_prefill_attention(out, q_new, kc, vc, perm.to(torch.int32).to(dev), cu_of(q_lens, dev), sl, cl,
                                 max(q_lens), d**-0.5, slopes.to(dev) if alibi else None, window)
    ref = ref_attention(q_all.float(), k_all.float(), v_all.float(), seq_lens, d**-0.5, slopes, window)
    check(out, ref[rows], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("head_size", [96, 256])
@pytest.mark.parametrize("chunked", [False, True])
def test_backend_head_sizes(gpu_device, dtype, head_size, chunked):
    """ROCmHipAttentionImpl.forward.  Not chunked: a pure-prompt batch with a sliding window.  Chunked: one prompt
    in two chunks, the second taking the prefix branch over the cache the first has written.  Both against plain
    attention over the whole prompt."""
    from neural_magic_vllm_amd.attention.backends.rocm_hip_attn import (ROCmHipAttentionBackend, ROCmHipAttentionImpl,
                                                                        ROCmHipAttentionMetadata)
    dev, nq, nkv, d, bs = gpu_device, 8, 2, head_size, 16
    seq_lens, window = ([150], None) if chunked else ([100, 37], 40)
    impl = ROCmHipAttentionImpl(nq, d, d**-0.5, nkv, sliding_window=window)
    g = torch.Generator().manual_seed(2)
    total = sum(seq_lens)
    q_all, k_all, v_all = ((torch.rand((total, n * d), generator=g) * 2 - 1).to(dtype) for n in (nq, nkv, nkv))
    kv_cache = torch.full(ROCmHipAttentionBackend.get_kv_cache_shape(32, bs, nkv, d), float("nan"), dtype=dtype,
                          device=dev)
    tables = torch.randperm(32, generator=g)[:len(seq_lens) * 10].view(len(seq_lens), 10).to(torch.int32)
    starts = [0] + torch.tensor(seq_lens).cumsum(0).tolist()[:-1]

    def chunk(los, his):
        rows = torch.cat([torch.arange(s + lo, s + hi) for s, lo, hi in zip(starts, los, his)])
        slots = torch.cat([tables[i][torch.arange(lo, hi) // bs].long() * bs + torch.arange(lo, hi) % bs
                           for i, (lo, hi) in enumerate(zip(los, his))])
        lens = [hi - lo for lo, hi in zip(los, his)]
        cu = cu_of(lens, dev)
        md = ROCmHipAttentionMetadata(
            num_prefills=len(lens), num_prefill_tokens=sum(lens), num_decode_tokens=0, slot_mapping=slots.to(dev),
            seq_lens=list(his), seq_lens_tensor=torch.tensor(his, dtype=torch.int32, device=dev),
            max_query_len=max(lens), max_prefill_seq_len=max(his), max_decode_seq_len=0, query_start_loc=cu,
            seq_start_loc=cu if max(los) == 0 else None,
            context_lens_tensor=torch.tensor(los, dtype=torch.int32, device=dev), block_tables=tables.to(dev),
            use_cuda_graph=False)
        return rows, impl.forward(q_all[rows].to(dev), k_all[rows].to(dev), v_all[rows].to(dev), kv_cache, md)

    ref = ref_attention(q_all.float().view(total, nq, d), k_all.float().view(total, nkv, d),
                        v_all.float().view(total, nkv, d), seq_lens, d**-0.5, None, window)
    firsts = [70] if chunked else seq_lens
    rows, out = chunk([0] * len(seq_lens), firsts)
    check(out.view(-1, nq, d), ref[rows], dtype)
    if chunked:
        rows, out = chunk(firsts, seq_lens)
        check(out.view(-1, nq, d), ref[rows], dtype)


@pytest.mark.parametrize("head_size,built", [(96, True), (112, True), (192, True), (256, True), (80, False),
                                             (72, False)])
def test_prefill_attention_supported_head_sizes(gpu_device, head_size, built):
    from neural_magic_vllm_amd import _custom_ops as ops
    assert ops.prefill_attention_supported(head_size) == built
