"""GPU microbenchmark of prompt attention at the head sizes beyond 64 / 128 (method of tools/bench_prefix_attn.py:
one process, every path warmed up, paths alternated, device events around `iters` launches, median and range of
`reps` windows).
  varlen  ops.prefill_attention against the torch SDPA loop it replaces (_sdpa_prefill, the backend's path for
          head sizes without a kernel), 32/8 heads, bf16, at D = 96 and 256
  prefix  ops.prefix_prefill_attention on a 16-bit cache, a 512-token chunk on a 3584-token context, block 16:
          the staged kernel at D = 96 / 112 / 192 / 256 beside prefix_attention_kernel at D = 128
  --alt-lib PATH  a second build of the same C ABI (make -C neural_magic_vllm_amd/csrc BUILD=... OUT=PATH after a
          local change to a kernel): its nmv_prefill_attention joins the varlen comparison as "alt", alternated with
          the product library's in the same process
usage: python tools/bench_prefill_head_sizes.py [--iters 20] [--reps 7] [--alt-lib PATH]"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_magic_vllm_amd import _custom_ops as ops  # noqa: E402
from neural_magic_vllm_amd import _lib  # noqa: E402
from neural_magic_vllm_amd.attention.backends.rocm_hip_attn import _sdpa_prefill  # noqa: E402

NQ, NKV, BLOCK = 32, 8, 16


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def compare(title, fns, flops, iters, reps):
    """alternate the paths; print median (min-max) microseconds and TFLOP/s of each"""
    for fn in fns.values():
        window(fn, 3)
    us = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            us[k].append(window(fn, iters))
    med = {k: statistics.median(v) for k, v in us.items()}
    print(title + ": " + "  ".join(f"{k} {med[k]:8.1f} us ({min(us[k]):.1f}-{max(us[k]):.1f}) "
                                   f"{flops[k] / med[k] / 1e6:6.1f} TFLOP/s" for k in fns), flush=True)
    return med


def varlen(d, seq_lens, dev, alt=None):
    t = sum(seq_lens)
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = (torch.rand((t, (NQ + 2 * NKV) * d), device=dev, generator=g) - 0.5).to(torch.bfloat16)
    q, k, v = (x.view(t, -1, d) for x in qkv.split([NQ * d, NKV * d, NKV * d], dim=-1))
    out = torch.empty((t, NQ, d), dtype=torch.bfloat16, device=dev)
    cu = torch.tensor([0] + torch.tensor(seq_lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    flops = 4.0 * d * NQ * sum(L * (L + 1) / 2 for L in seq_lens)
    fns = {"hip": lambda: ops.prefill_attention(out, q, k, v, cu, max(seq_lens), d**-0.5),
           "sdpa": lambda: _sdpa_prefill(q, k, v, seq_lens, NQ // NKV, d**-0.5, None)}
    if alt is not None:
        stream = torch.cuda.current_stream().cuda_stream

        def call():   # the closure keeps the tensors behind the raw pointers alive
            rc = alt.nmv_prefill_attention(out.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(), cu.data_ptr(),
                                           len(seq_lens), max(seq_lens), NQ, NKV, d, d**-0.5, q.stride(0), k.stride(0),
                                           out.stride(0), None, 0, _lib.NMV_BF16, stream)
            assert rc == 0
        fns["alt"] = call
    return fns, flops


def prefix(d, ctx, chunk, dev):
    L = ctx + chunk
    blocks = (L + BLOCK - 1) // BLOCK
    g = torch.Generator(device=dev).manual_seed(0)
    kc = (torch.rand((blocks, NKV, d // 8, BLOCK, 8), device=dev, generator=g) - 0.5).to(torch.bfloat16)
    vc = (torch.rand((blocks, NKV, d, BLOCK), device=dev, generator=g) - 0.5).to(torch.bfloat16)
    q = torch.randn((chunk, NQ, d), device=dev, dtype=torch.bfloat16, generator=g) * 0.1
    out = torch.empty_like(q)
    tables = torch.randperm(blocks, device=dev, generator=g).to(torch.int32).view(1, blocks)
    qsl = torch.tensor([0, chunk], dtype=torch.int32, device=dev)
    sl = torch.tensor([L], dtype=torch.int32, device=dev)
    cl = torch.tensor([ctx], dtype=torch.int32, device=dev)
    flops = 4.0 * d * NQ * (chunk * ctx + chunk * (chunk + 1) / 2)
    return (lambda: ops.prefix_prefill_attention(out, q, kc, vc, tables, qsl, sl, cl, chunk, d**-0.5)), flops


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--alt-lib", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    alt = None
    if args.alt_lib:
        alt = ctypes.CDLL(args.alt_lib)
        alt.nmv_prefill_attention.restype, alt.nmv_prefill_attention.argtypes = _lib.SIGNATURES["nmv_prefill_attention"]
    for d in (96, 256):
        for seq_lens in ([2048], [512] * 8):
            fns, flops = varlen(d, seq_lens, dev, alt)
            med = compare(f"varlen D={d} prompts={len(seq_lens)}x{seq_lens[0]} heads={NQ}/{NKV} bf16", fns,
                          {k: flops for k in fns}, args.iters, args.reps)
            print(f"    sdpa/hip {med['sdpa'] / med['hip']:.2f}", flush=True)
    fns, flops = {}, {}
    for d in (96, 112, 128, 192, 256):
        fns[f"D={d}"], flops[f"D={d}"] = prefix(d, 3584, 512, dev)
    compare(f"prefix context=3584 chunk=512 heads={NQ}/{NKV} block={BLOCK} bf16", fns, flops, args.iters, args.reps)
