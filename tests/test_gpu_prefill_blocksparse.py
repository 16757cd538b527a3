"""GPU parity of block-sparse prompt attention (csrc/prefill_attention_blocksparse.hip) against a dense fp32
reference on the CPU whose boolean mask is built from the rule itself; inputs, NaN-filled output and tolerances as in
test_gpu_prefill_attention.py::test_prefill_attention."""
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

# name: sparse block, local blocks, vertical stride, head sliding step, tp rank, (H, KVH), prompt lengths.  Together: a
# skipped tile, a strided tile below the band, the band, the diagonal, a ragged last tile, a one-token prompt, sparse
# blocks smaller (B) and larger (C) than the 64-key tile; D is Phi-3-small's pattern
PATTERNS = {"A": (64, 2, 3, 1, 0, (4, 2), [581, 1, 64, 65, 200]),
            "B": (16, 3, 4, 1, 0, (4, 2), [333, 150]),
            "C": (128, 1, 2, -1, 1, (4, 2), [700]),
            "D": (64, 16, 8, 0, 0, (8, 2), [1300])}
TOL = {torch.half: 2e-3, torch.bfloat16: 1.6e-2}   # P and the output are rounded to the model dtype


def ref_blocksparse(q, k, v, seq_lens, scale, sb, local, vs, step, tp_rank):
    """q [T, H, D], k / v [T, KVH, D] fp32: query i of head h attends key j iff j <= i and
    (i // sb - j // sb < local or (j // sb + off_h) % vs == 0)"""
    nq, nkv = q.shape[1], k.shape[1]
    h = torch.arange(nq)
    off = (tp_rank * nq + h) * step + 1 if step >= 0 else (tp_rank * nkv + h // (nq // nkv)) * -step + 1
    out, start = torch.empty_like(q), 0
    for L in seq_lens:
        qs, ks, vs_ = (x[start:start + L].transpose(0, 1) for x in (q, k, v))
        ks, vs_ = ks.repeat_interleave(nq // nkv, dim=0), vs_.repeat_interleave(nq // nkv, dim=0)
        pos = torch.arange(L)
        qb, kb = pos[:, None] // sb, pos[None, :] // sb
        allow = (pos[None, :] <= pos[:, None]) & ((qb - kb < local) | ((kb + off[:, None, None]) % vs == 0))
        s = ((qs @ ks.transpose(1, 2)) * scale).masked_fill(~allow, float("-inf"))
        out[start:start + L] = (torch.softmax(s, dim=-1) @ vs_).transpose(0, 1)
        start += L
    return out


def make_qkv(seq_lens, nq, nkv, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((sum(seq_lens), (nq + 2 * nkv) * d), generator=g) * 2 - 1).to(dtype)


def split(qkv, nq, nkv, d):
    q, k, v = qkv.split([nq * d, nkv * d, nkv * d], dim=-1)
    return q.view(-1, nq, d), k.view(-1, nkv, d), v.view(-1, nkv, d)


def check(got, ref, dtype):
    got = got.float().cpu()
    assert not torch.isnan(got).any()
    torch.testing.assert_close(got, ref, atol=TOL[dtype], rtol=TOL[dtype])


def cu_of(lens, dev):
    return torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)


@pytest.mark.parametrize("dtype", [torch.half, torch.bfloat16])
@pytest.mark.parametrize("pattern,head_size", [(p, d) for p in "ABCD" for d in (64, 128)] +
                         [("A", d) for d in (96, 112, 192, 256)])
def test_prefill_attention_blocksparse(gpu_device, dtype, pattern, head_size):
    from neural_magic_vllm_amd import _custom_ops as ops
    sb, local, vs, step, tp_rank, (nq, nkv), seq_lens = PATTERNS[pattern]
    d, scale = head_size, head_size**-0.5
    qkv = make_qkv(seq_lens, nq, nkv, d, dtype)
    q, k, v = split(qkv.to(gpu_device), nq, nkv, d)
    out = torch.full((sum(seq_lens), nq, d), float("nan"), dtype=dtype, device=gpu_device)
    ops.prefill_attention(out, q, k, v, cu_of(seq_lens, gpu_device), max(seq_lens), scale, tp_rank=tp_rank,
                          blocksparse_local_blocks=local, blocksparse_vert_stride=vs, blocksparse_block_size=sb,
                          blocksparse_head_sliding_step=step)
    check(out, ref_blocksparse(*split(qkv.float(), nq, nkv, d), seq_lens, scale, sb, local, vs, step, tp_rank), dtype)


def make_backend(dev, dtype, d=128, bs=16, num_blocks=256):
    """a block-sparse ROCmHipAttentionImpl of pattern A, a NaN-filled paged cache, and a metadata builder"""
    from neural_magic_vllm_amd.attention.backends.rocm_hip_attn import (ROCmHipAttentionBackend, ROCmHipAttentionImpl,
                                                                        ROCmHipAttentionMetadata)
    sb, local, vs, _, _, (nq, nkv), seq_lens = PATTERNS["A"]
    per_seq = (max(seq_lens) + bs) // bs   # blocks per sequence: the block tables span the model's longest sequence
    impl = ROCmHipAttentionImpl(nq, d, d**-0.5, nkv, blocksparse_params=dict(
        max_seqlen=per_seq * bs, block_size=sb, local_blocks=local, vert_stride=vs))
    kv_cache = torch.full(ROCmHipAttentionBackend.get_kv_cache_shape(num_blocks, bs, nkv, d), float("nan"),
                          dtype=dtype, device=dev)
    tables = torch.randperm(num_blocks, generator=torch.Generator().manual_seed(1))[:len(seq_lens) * per_seq]
    tables = tables.view(len(seq_lens), per_seq).to(torch.int32)

    def metadata(los, his, decode=False):
        """tokens [lo, hi) of the first len(los) sequences: a prompt batch, or (decode) one decode token each"""
        slots = torch.cat([tables[i][torch.arange(lo, hi) // bs].long() * bs + torch.arange(lo, hi) % bs
                           for i, (lo, hi) in enumerate(zip(los, his))])
        lens = [hi - lo for lo, hi in zip(los, his)]
        cu = cu_of(lens, dev)
        return ROCmHipAttentionMetadata(
            num_prefills=0 if decode else len(lens), num_prefill_tokens=0 if decode else sum(lens),
            num_decode_tokens=len(lens) if decode else 0, slot_mapping=slots.to(dev), seq_lens=list(his),
            seq_lens_tensor=torch.tensor(his, dtype=torch.int32, device=dev), max_query_len=max(lens),
            max_prefill_seq_len=0 if decode else max(his), max_decode_seq_len=max(his) if decode else 0,
            query_start_loc=cu, seq_start_loc=cu if max(los) == 0 else None,
            context_lens_tensor=torch.tensor(los, dtype=torch.int32, device=dev),
            block_tables=tables[:len(los)].to(dev),
            use_cuda_graph=False)
    return impl, kv_cache, tables, metadata


@pytest.mark.parametrize("dtype", [torch.half, torch.bfloat16])
def test_backend_blocksparse_prompt_then_decode(gpu_device, dtype):
    """ROCmHipAttentionImpl.forward of a block-sparse layer: a prompt batch through the prompt kernel, then one
    decode step of the same sequences through paged attention over the cache the prompt wrote -- both against the
    same rule (the decode side through helpers.ref_paged_attention_torch)"""
    from neural_magic_vllm_amd.attention.ops.paged_attn import PagedAttention
    sb, local, vs, step, tp_rank, (nq, nkv), seq_lens = PATTERNS["A"]
    d, dev = 128, gpu_device
    impl, kv_cache, tables, metadata = make_backend(dev, dtype, d)
    assert impl.blocksparse_params.head_sliding_step == step
    grown = [L + 1 for L in seq_lens]
    q, k, v = (x.reshape(x.shape[0], -1) for x in split(make_qkv(grown, nq, nkv, d, dtype), nq, nkv, d))
    starts = [0] + torch.tensor(grown).cumsum(0).tolist()[:-1]
    prompt = torch.cat([torch.arange(s, s + L) for s, L in zip(starts, seq_lens)])
    last = torch.tensor([s + L for s, L in zip(starts, seq_lens)])

    out = impl.forward(q[prompt].to(dev), k[prompt].to(dev), v[prompt].to(dev), kv_cache,
                       metadata([0] * len(seq_lens), seq_lens))
    ref = ref_blocksparse(q[prompt].float().view(-1, nq, d), k[prompt].float().view(-1, nkv, d),
                          v[prompt].float().view(-1, nkv, d), seq_lens, d**-0.5, sb, local, vs, step, tp_rank)
    check(out.view(-1, nq, d), ref, dtype)

    out = impl.forward(q[last].to(dev), k[last].to(dev), v[last].to(dev), kv_cache, metadata(seq_lens, grown, True))
    kc, vc = PagedAttention.split_kv_cache(kv_cache.cpu(), nkv, d)
    ref = helpers.ref_paged_attention_torch(
        dict(query=q[last].view(-1, nq, d), key_cache=kc, value_cache=vc, block_tables=tables,
             seq_lens=torch.tensor(grown, dtype=torch.int32), scale=d**-0.5, alibi_slopes=None),
        blocksparse=dict(tp_rank=tp_rank, local_blocks=local, vert_stride=vs, block_size=sb, head_sliding_step=step))
    check(out.view(-1, nq, d), ref, dtype)


@pytest.mark.parametrize("case", ["local_blocks=0", "block_size=48", "alibi", "prefix"])
def test_blocksparse_rejections(gpu_device, case):
    from neural_magic_vllm_amd import _custom_ops as ops
    from neural_magic_vllm_amd._lib import NmvError
    dev, dtype, nq, nkv, d = gpu_device, torch.half, 4, 2, 128
    if case == "prefix":   # a block-sparse layer given a prefix-enabled batch (context 16, 8 new tokens)
        impl, kv_cache, _, metadata = make_backend(dev, dtype, d)
        q, k, v = (x.reshape(8, -1).to(dev) for x in split(make_qkv([8], nq, nkv, d, dtype), nq, nkv, d))
        with pytest.raises(NotImplementedError, match="prefix"):
            impl.forward(q, k, v, kv_cache, metadata([16], [24]))
        return
    q, k, v = split(make_qkv([100], nq, nkv, d, dtype).to(dev), nq, nkv, d)
    kw = dict(blocksparse_local_blocks=2, blocksparse_vert_stride=3, blocksparse_block_size=64)
    slopes = torch.ones(nq, dtype=torch.float32, device=dev) if case == "alibi" else None
    if case != "alibi":
        name, value = case.split("=")
        kw["blocksparse_" + name] = int(value)
    with pytest.raises(NmvError, match="ALiBi" if case == "alibi" else "prefill_attention_blocksparse"):
        ops.prefill_attention(torch.empty_like(q), q, k, v, cu_of([100], dev), 100, d**-0.5, slopes, **kw)
