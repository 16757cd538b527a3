"""GPU microbenchmark of prefix-enabled prompt attention (chunked prefill): the 16-bit prefix_attention_kernel
against the fp8-cache kernel at the same geometry, the two alternated in one process, device events around
`iters` launches, median of `reps` windows after a warm-up of both.
usage: python tools/bench_prefix_attn.py [--cases NSEQ:CONTEXT:CHUNK,...] [--heads 32:8] [--head-size 128] [--block 16]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_magic_vllm_amd import _custom_ops as ops  # noqa: E402


def make(kv, nseq, ctx, chunk, nq, nkv, d, bs, dev):
    L = ctx + chunk
    blocks = (L + bs - 1) // bs
    g = torch.Generator(device=dev).manual_seed(0)
    if kv == "fp8":   # bytes 0..119: finite e4m3 values
        kc = torch.randint(0, 120, (nseq * blocks, nkv, d // 16, bs, 16), dtype=torch.uint8, device=dev, generator=g)
        vc = torch.randint(0, 120, (nseq * blocks, nkv, d, bs), dtype=torch.uint8, device=dev, generator=g)
    else:
        kc = (torch.rand((nseq * blocks, nkv, d // 8, bs, 8), device=dev, generator=g) - 0.5).to(torch.bfloat16)
        vc = (torch.rand((nseq * blocks, nkv, d, bs), device=dev, generator=g) - 0.5).to(torch.bfloat16)
    q = torch.randn((nseq * chunk, nq, d), device=dev, dtype=torch.bfloat16, generator=g) * 0.1
    out = torch.empty_like(q)
    tables = torch.randperm(nseq * blocks, device=dev, generator=g).to(torch.int32).view(nseq, blocks)
    qsl = torch.arange(0, (nseq + 1) * chunk, chunk, dtype=torch.int32, device=dev)
    sl = torch.full((nseq, ), L, dtype=torch.int32, device=dev)
    cl = torch.full((nseq, ), ctx, dtype=torch.int32, device=dev)
    return lambda: ops.prefix_prefill_attention(out, q, kc, vc, tables, qsl, sl, cl, chunk, d**-0.5, None, None,
                                                kv, 0.5 if kv == "fp8" else 1.0)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1:3584:512,4:3584:512,1:0:4096")
    ap.add_argument("--heads", default="32:8")
    ap.add_argument("--head-size", type=int, default=128)
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    nq, nkv = (int(v) for v in args.heads.split(":"))
    for case in args.cases.split(","):
        nseq, ctx, chunk = (int(v) for v in case.split(":"))
        fns = {kv: make(kv, nseq, ctx, chunk, nq, nkv, args.head_size, args.block, dev) for kv in ("auto", "fp8")}
        for fn in fns.values():
            window(fn, 5)
        us = {kv: [] for kv in fns}
        for _ in range(args.reps):
            for kv, fn in fns.items():
                us[kv].append(window(fn, args.iters))
        # causal pairs of (new token, key): chunk * ctx + chunk * (chunk + 1) / 2 per head, 4 D flops each
        flops = 4.0 * args.head_size * nq * nseq * (chunk * ctx + chunk * (chunk + 1) / 2)
        med = {kv: statistics.median(v) for kv, v in us.items()}
        print(f"prefix attn nseq={nseq} context={ctx} chunk={chunk} heads={nq}/{nkv} D={args.head_size} block={args.block}: "
              + "  ".join(f"{kv} {med[kv]:8.1f} us ({min(us[kv]):.1f}-{max(us[kv]):.1f}) {flops / med[kv] / 1e6:6.1f} TFLOP/s"
                          for kv in fns) + f"   fp8/auto {med['fp8'] / med['auto']:.2f}", flush=True)
