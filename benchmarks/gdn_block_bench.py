"""GatedDeltaNet block with the fused HIP prologue (D9D_GDN_PREP=1) against
the torch chain (=0), and the two prologue kernels alone.

B8 S4096, hidden 2048, 16 qk / 32 v heads, D 128, bf16 (Qwen3-Next's layer
shape), forward and forward+backward, both decay gates' kernels behind
--gate. The two paths alternate inside every round in one process; windows
are timed with device events after both paths are warm; the outputs and
input gradients of the two paths are compared before any time counts. The
kernels alone are reported with the bytes their shapes require (every input
read once, every output written once) over the measured time. Prints a table
and one JSON line. No GPU: it fails.
"""
import argparse
import json
import os
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch

from d9d_amd.module.block.attention.linear import GatedDeltaNet
from d9d_amd.ops._ext import get_ext


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=4096)
    ap.add_argument("--hidden", type=int, default=2048)
    ap.add_argument("--gate", choices=("logsigmoid", "mamba"), default="mamba")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8, help="calls per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; no fallback"
    B, S, H, Hkv, D = args.batch, args.seq, 32, 16, 128

    torch.manual_seed(0)
    m = GatedDeltaNet(args.hidden, num_heads=H, num_kv_heads=Hkv, head_k_dim=D,
                      head_v_dim=D, decay_gate=args.gate)
    m.reset_parameters()
    with torch.no_grad():
        for lin in (m.q_proj, m.k_proj, m.v_proj, m.beta_proj, m.out_gate, m.o_proj):
            torch.nn.init.normal_(lin.weight, std=0.5 * lin.in_features ** -0.5)
    m = m.cuda().bfloat16()
    x = torch.randn(B, S, args.hidden, device="cuda").bfloat16().requires_grad_(True)
    dout = torch.randn(B, S, args.hidden, device="cuda").bfloat16()

    def with_flag(flag, fn):
        def run():
            os.environ["D9D_GDN_PREP"] = flag
            try:
                return fn()
            finally:
                del os.environ["D9D_GDN_PREP"]
        return run

    def fwd():
        with torch.no_grad():
            return m(x)

    def fwd_bwd():
        m.zero_grad(set_to_none=True)
        out = m(x)
        return out, torch.autograd.grad(out, [x, *m.parameters()], dout)[0]

    # the prologue kernels on their own, at the block's shapes
    ext = get_ext()
    q, k = (torch.randn(B, S, Hkv, D, device="cuda").bfloat16() for _ in range(2))
    v = torch.randn(B, S, H, D, device="cuda").bfloat16()
    b_raw, a_raw = (torch.randn(B, S, H, device="cuda").bfloat16() for _ in range(2))
    gate = [None, None]
    if args.gate == "mamba":
        gate = [m.decay_gate.A_log.detach().float(), m.decay_gate.dt_bias.detach().float()]
    grads = [torch.randn(B, H, S, D, device="cuda") for _ in range(3)]
    grads += [torch.randn(B, H, S, device="cuda") for _ in range(2)]
    small, big, gates = B * S * Hkv * D, B * S * H * D, B * S * H
    kernel_bytes = {
        "prep_fwd": 2 * (2 * small + big + 2 * gates) + 2 * 3 * big + 4 * 2 * gates,
        "prep_bwd": 2 * (2 * small + 2 * gates) + 4 * (3 * big + 2 * gates)
                    + 2 * (2 * small + big + 2 * gates),
    }
    kernels = {
        "prep_fwd": lambda: ext.gdn_prep_fwd(q, k, v, b_raw, a_raw, *gate),
        "prep_bwd": lambda: ext.gdn_prep_bwd(q, k, b_raw, a_raw, *gate, *grads),
    }

    def window(fn, iters) -> float:
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / iters

    # agreement first: output and dx of the two paths, bf16 tolerances
    out0, dx0 = with_flag("0", fwd_bwd)()
    out1, dx1 = with_flag("1", fwd_bwd)()
    for name, a, b, atol in (("out", out1, out0, 3e-2), ("dx", dx1, dx0, 1e-1)):
        a, b = a.detach().float(), b.detach().float()
        err = (a - b).abs()
        bound = atol + 5e-2 * b.abs()
        assert bool((err <= bound).all()), f"{name}: the paths disagree, max err {float(err.max()):.4g}"
        print(f"{name}: max |fused - chain| {float(err.max()):.4g}, max |chain| "
              f"{float(b.abs().max()):.4g}")
    del out0, dx0, out1, dx1

    groups = {
        "fwd": ({"chain": with_flag("0", fwd), "fused": with_flag("1", fwd)}, args.iters),
        "fwd_bwd": ({"chain": with_flag("0", fwd_bwd), "fused": with_flag("1", fwd_bwd)},
                    args.iters),
        "kernel": (kernels, 50 * args.iters),
    }
    result = {"batch": B, "seq": S, "hidden": args.hidden, "heads": H, "kv_heads": Hkv,
              "head_dim": D, "gate": args.gate, "rounds": args.rounds, "iters": args.iters}
    for gname, (variants, iters) in groups.items():
        for fn in variants.values():  # warm both paths
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():  # alternate inside each round
                times[name].append(window(fn, iters))
        for name, ts in times.items():
            med = statistics.median(ts)
            key = name if gname == "kernel" else f"{gname}_{name}"
            result[f"{key}_ms"] = round(med, 4)
            result[f"{key}_min_ms"] = round(min(ts), 4)
            result[f"{key}_max_ms"] = round(max(ts), 4)
            line = f"{gname:8s} {name:9s} median {med:8.3f} ms   min {min(ts):8.3f}  max {max(ts):8.3f}"
            if gname == "kernel":
                result[f"{key}_tb_s"] = round(kernel_bytes[name] / med / 1e9, 3)
                line += f"   {kernel_bytes[name] / 1e9:.3f} GB, {result[f'{key}_tb_s']:.2f} TB/s"
            print(line)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
