"""Packed-document GatedDeltaNet recurrence: varlen kernels vs the dense
kernels on the same packed row vs a Python loop of dense calls.

H = 16 heads, T = 32768 packed tokens, document lengths drawn once from a
seeded log-uniform distribution over [32, 8192]. Three variants, forward
and forward+backward (through `chunk_gated_delta_rule` on the kernel-scan
path):
  (a) varlen : cu_seqlens path, one workgroup per (document, head)
  (b) dense  : the dense kernels on (1, H, T), IGNORING boundaries — the
               wrong model, but the cost baseline for the same tokens
  (c) loop   : one dense call per document
Timed with device events after warm-up; the variants alternate inside every
round and the rounds repeat, so the spread is measured under the same
conditions as the medians. Prints a table and one JSON line.
"""
import argparse
import json
import math
import pathlib
import random
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch
import torch.nn.functional as F

from d9d_amd.module.block.attention.linear.gated_deltanet import chunk_gated_delta_rule
from d9d_amd.ops._ext import get_ext


def draw_lengths(total: int, lo: int, hi: int, seed: int) -> list[int]:
    rng = random.Random(seed)
    lens, used = [], 0
    while used < total:
        n = int(round(math.exp(rng.uniform(math.log(lo), math.log(hi)))))
        n = min(n, total - used)
        lens.append(n)
        used += n
    return lens


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; no fallback"

    ext = get_ext()
    H, T, D = args.heads, args.tokens, 64
    lens = draw_lengths(T, 32, 8192, args.seed)
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)
    spans = list(zip(cu[:-1].tolist(), cu[1:].tolist()))
    cu = cu.cuda()
    nc = sum((n + 63) // 64 for n in lens)

    torch.manual_seed(args.seed)
    q = F.normalize(torch.randn(1, H, T, D, device="cuda"), dim=-1).bfloat16()
    k = F.normalize(torch.randn(1, H, T, D, device="cuda"), dim=-1).bfloat16()
    v = (torch.randn(1, H, T, D, device="cuda") * 0.5).bfloat16()
    beta = torch.rand(1, H, T, device="cuda")
    g = -torch.rand(1, H, T, device="cuda") * 0.2
    do = torch.randn(1, H, T, D, device="cuda").bfloat16()
    leaves = [t.detach().requires_grad_(True) for t in (q, k, v, beta, g)]

    def fwd_varlen():
        return ext.gdn_chunk_fwd_varlen(q, k, v, beta, g, cu, False, False, False)[0]

    def fwd_dense():
        return ext.gdn_chunk_fwd(q, k, v, beta, g, False, False, False)[0]

    def fwd_loop():
        return [
            ext.gdn_chunk_fwd(
                q[:, :, s:e], k[:, :, s:e], v[:, :, s:e],
                beta[:, :, s:e], g[:, :, s:e], False, False, False,
            )[0]
            for s, e in spans
        ]

    def fb_varlen():
        out = chunk_gated_delta_rule(*leaves, cu_seqlens=cu)
        return torch.autograd.grad(out, leaves, do)

    def fb_dense():
        out = chunk_gated_delta_rule(*leaves)
        return torch.autograd.grad(out, leaves, do)

    def fb_loop():
        grads = []
        for s, e in spans:
            part = [t[:, :, s:e] for t in leaves]
            out = chunk_gated_delta_rule(*part)
            grads.append(torch.autograd.grad(out, leaves, do[:, :, s:e]))
        return grads

    def window(fn) -> float:
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.iters):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / args.iters

    groups = {
        "fwd": {"varlen": fwd_varlen, "dense": fwd_dense, "loop": fwd_loop},
        "fwd_bwd": {"varlen": fb_varlen, "dense": fb_dense, "loop": fb_loop},
    }
    result = {
        "heads": H, "tokens": T, "ndocs": len(lens), "chunks": nc,
        "longest_doc": max(lens), "padded_row_overhead": 64 * nc / T,
        "rounds": args.rounds, "iters": args.iters,
    }
    print(f"H={H} T={T} docs={len(lens)} longest={max(lens)} NC={nc} "
          f"padded rows 64*NC/T = {64 * nc / T:.4f}")
    for gname, variants in groups.items():
        for fn in variants.values():  # warm-up: every shape the window uses
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():  # alternate inside each round
                times[name].append(window(fn))
        for name, ts in times.items():
            med = statistics.median(ts)
            result[f"{gname}_{name}_ms"] = round(med, 4)
            result[f"{gname}_{name}_min_ms"] = round(min(ts), 4)
            result[f"{gname}_{name}_max_ms"] = round(max(ts), 4)
            print(f"{gname:8s} {name:7s} median {med:8.3f} ms   "
                  f"min {min(ts):8.3f}  max {max(ts):8.3f}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
