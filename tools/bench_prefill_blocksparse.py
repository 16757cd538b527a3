"""GPU microbenchmark of block-sparse prompt attention (csrc/prefill_attention_blocksparse.hip), method of
tools/bench_prefill_head_sizes.py: one process, every path warmed up, paths alternated, device events around `iters`
launches, median and range of `reps` windows.  One prompt of L tokens, Phi-3-small's pattern (sparse block 64, 16 local
blocks, vertical stride 8, 32 / 8 heads, D = 128, bf16), on the same tensors:
  sparse  ops.prefill_attention with the five block-sparse ints
  dense   ops.prefill_attention without them (the unchanged dense causal kernel: more work, another result)
  sdpa    what the reference runs on ROCm: torch SDPA under a dense [H, L, L] bias (its
          blocksparse_attention/interface.py), where the bias fits in --sdpa-gib of memory
and beside them the share of the causal 64-key tiles the sparse kernel visits, counted on the CPU with the kernel's
own arithmetic (visited_tiles).
usage: python tools/bench_prefill_blocksparse.py [--lens 2048 8192 32768] [--iters 200] [--reps 7] [--step 1]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from neural_magic_vllm_amd import _custom_ops as ops  # noqa: E402
from bench_prefill_head_sizes import compare  # noqa: E402

NQ, NKV, D, SB, LOCAL, VS, KT = 32, 8, 128, 64, 16, 8, 64


def head_offset(h, step, tp_rank=0):
    return (tp_rank * NQ + h) * step + 1 if step >= 0 else (tp_rank * NKV + h // (NQ // NKV)) * -step + 1


def visited_tiles(L, step):
    """(visited, causal) 64-key tiles summed over heads and 64-query tiles: the kernel's enumeration (SB % 64 == 0:
    a tile lies in one block; strided blocks below the band, then the band up to the diagonal)"""
    visited = causal = 0
    for h in range(NQ):
        off = head_offset(h, step)
        for qt in range((L + 63) // 64):
            qb = qt * 64 // SB
            band_lo = max(qb - LOCAL + 1, 0)
            strided = sum(1 for kb in range(band_lo) if (kb + off) % VS == 0)
            last_t = (min(qt * 64 + 64, L) - 1) // KT
            visited += strided * (SB // KT) + last_t - band_lo * SB // KT + 1
            causal += last_t + 1
    return visited, causal


def dense_bias(L, step, dev):
    """the reference's [H, L, L] additive mask (0 / -inf) of the pattern, causal included"""
    pos = torch.arange(L, device=dev)
    qb, kb = pos[:, None] // SB, pos[None, :] // SB
    off = torch.tensor([head_offset(h, step) for h in range(NQ)], device=dev)
    allow = (pos[None, :] <= pos[:, None]) & ((qb - kb < LOCAL) | ((kb + off[:, None, None]) % VS == 0))
    return torch.zeros((NQ, L, L), dtype=torch.bfloat16, device=dev).masked_fill_(~allow, float("-inf"))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", type=int, nargs="+", default=[2048, 8192, 32768])
    ap.add_argument("--iters", type=int, default=200, help="launches per window at L = 2048; fewer at longer L")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", type=int, default=1, help="head sliding step (Phi-3-small: max(1, 8 // 32) = 1)")
    ap.add_argument("--sdpa-gib", type=float, default=8.0, help="largest dense bias the sdpa path may allocate")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    for L in args.lens:
        g = torch.Generator(device=dev).manual_seed(0)
        qkv = (torch.rand((L, (NQ + 2 * NKV) * D), device=dev, generator=g) - 0.5).to(torch.bfloat16)
        q, k, v = (x.view(L, -1, D) for x in qkv.split([NQ * D, NKV * D, NKV * D], dim=-1))
        out = torch.empty((L, NQ, D), dtype=torch.bfloat16, device=dev)
        cu = torch.tensor([0, L], dtype=torch.int32, device=dev)
        visited, causal = visited_tiles(L, args.step)
        dense_flops = 4.0 * D * NQ * L * (L + 1) / 2
        fns = {"sparse": lambda: ops.prefill_attention(out, q, k, v, cu, L, D**-0.5, blocksparse_local_blocks=LOCAL,
                                                       blocksparse_vert_stride=VS, blocksparse_block_size=SB,
                                                       blocksparse_head_sliding_step=args.step),
               "dense": lambda: ops.prefill_attention(out, q, k, v, cu, L, D**-0.5)}
        flops = {"sparse": dense_flops * visited / causal, "dense": dense_flops}
        if NQ * L * L * 2 <= args.sdpa_gib * 2**30:
            bias = dense_bias(L, args.step, dev)
            qs = q.movedim(0, 1).unsqueeze(0)
            ks, vs_ = (x.movedim(0, 1).repeat_interleave(NQ // NKV, dim=0).unsqueeze(0) for x in (k, v))
            fns["sdpa"] = lambda: torch.nn.functional.scaled_dot_product_attention(qs, ks, vs_, attn_mask=bias,
                                                                                   scale=D**-0.5)
            flops["sdpa"] = dense_flops * 2   # the whole square
        med = compare(f"L={L} heads={NQ}/{NKV} D={D} block={SB} local={LOCAL} stride={VS} step={args.step} bf16", fns,
                      flops, max(2, args.iters * 2048 // L), args.reps)
        print(f"    tiles visited {visited} of {causal} ({visited / causal:.3f})  sparse/dense time "
              f"{med['sparse'] / med['dense']:.3f}" + (f"  sdpa/sparse {med['sdpa'] / med['sparse']:.1f}"
                                                        if "sdpa" in med else "  sdpa: bias too large"), flush=True)
        fns = bias = qs = ks = vs_ = None   # give the bias back before the next length
        torch.cuda.empty_cache()
