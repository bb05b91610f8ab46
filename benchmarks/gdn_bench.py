import sys, pathlib, time, statistics
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch
import torch.nn.functional as F
from d9d_amd.ops._ext import get_ext
from d9d_amd.module.block.attention.linear.gated_deltanet import (
    _chunk_gated_delta_rule_torch,
)

ext = get_ext()
torch.manual_seed(0)
# --head-dim 128: the wide chunk kernels (forward, aux, reverse scan) against
# the torch path; everything below bench_wide() is the D = 64 report
D = int(sys.argv[sys.argv.index("--head-dim") + 1]) if "--head-dim" in sys.argv else 64
assert D in (64, 128), "--head-dim takes 64 or 128"
B, H, S = 8, 16, 4096
q = F.normalize(torch.randn(B, H, S, D, device="cuda"), dim=-1).bfloat16()
k = F.normalize(torch.randn(B, H, S, D, device="cuda"), dim=-1).bfloat16()
v = (torch.randn(B, H, S, D, device="cuda") * 0.5).bfloat16()
beta = torch.rand(B, H, S, device="cuda")
g = -torch.rand(B, H, S, device="cuda") * 0.2

# backward leaf stage: gdn_chunk_bwd_leaf, or gdn_chunk_bwd_leaf_wide with
# --head-dim 128 (D9D_GDN_BWD_LEAF=1), against the torch stage (=0) in one process. Device events around windows of ITERS
# calls, the two paths alternating inside every round, so the spread is taken
# under the same conditions as the medians. `--bwd-leaf` runs only this.
def bench_bwd_leaf(rounds=9, iters=10):
    import json, os
    from d9d_amd.module.block.attention.linear.gated_deltanet import _chunk_gdn_backward

    qf, kf, vf = q.float(), k.float(), v.float()
    # bf16 values, as the gradient of the op's bf16 output is: the kernels
    # take dout in bf16, so both paths then see the same numbers
    do = torch.randn(B, H, S, D, device="cuda").bfloat16().float()

    def run(flag):
        os.environ["D9D_GDN_BWD_LEAF"] = flag
        return _chunk_gdn_backward(qf, kf, vf, beta, g, do)

    def window(flag):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            run(flag)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / iters

    # same inputs, both paths: the results must agree before the times count
    for name, a, b in zip(("dq", "dk", "dv", "dbeta", "dg"), run("0"), run("1")):
        print(f"bwd leaf kernel vs torch stage {name}: max abs diff "
              f"{(a - b).abs().max().item():.3e} (max abs {a.abs().max().item():.3g})")
    for flag in ("0", "1", "0", "1"):
        run(flag)
    times = {"0": [], "1": []}
    for _ in range(rounds):
        for flag in times:
            times[flag].append(window(flag))
    res = {"shape": [B, H, S, D], "rounds": rounds, "iters": iters}
    for flag, name in (("0", "torch_stage"), ("1", "leaf_kernel")):
        ts = times[flag]
        res[f"bwd_{name}_ms"] = round(statistics.median(ts), 4)
        res[f"bwd_{name}_min_ms"] = round(min(ts), 4)
        res[f"bwd_{name}_max_ms"] = round(max(ts), 4)
        print(f"gdn bwd D9D_GDN_BWD_LEAF={flag} ({name}): median {statistics.median(ts):.3f} ms"
              f"  min {min(ts):.3f}  max {max(ts):.3f}")
    os.environ.pop("D9D_GDN_BWD_LEAF")

    # the kernel alone, on the scan kernels' outputs
    do16 = do.bfloat16()
    r, s0 = ext.gdn_chunk_fwd(q, k, v, beta, g, False, True, True)
    drhs, ds0 = ext.gdn_chunk_bwd_scan(q, k, do16, beta, g)
    leaf = ext.gdn_chunk_bwd_leaf_wide if D == 128 else ext.gdn_chunk_bwd_leaf
    run = lambda flag: leaf(q, k, v, do16, beta, g, r, drhs, s0, ds0)
    run("1")
    ts = [window("1") for _ in range(rounds)]
    res["leaf_kernel_alone_ms"] = round(statistics.median(ts), 4)
    # per chunk: q, k, v, dout bf16 + r, drhs fp32 + s0, ds0 fp32 in; dq, dk, dv fp32 out
    nbytes = B * H * (S // 64) * (4 * 64 * D * 2 + 2 * 64 * D * 4 + 2 * D * D * 4 + 3 * 64 * D * 4)
    print(f"{leaf.__name__} alone: median {statistics.median(ts):.3f} ms  min {min(ts):.3f}"
          f"  max {max(ts):.3f}  ({nbytes / statistics.median(ts) / 1e9:.2f} TB/s of {nbytes / 1e9:.2f} GB)")
    print(json.dumps(res))

# head dim 128: the op on the chunk kernels (forward; aux forward + reverse
# scan + leaf kernel in the backward) against the torch path it took
# before they existed (torch WY forward, D9D_GDN_BWD_SCAN=0 backward). Device
# events around windows of ITERS calls, the two paths alternating inside
# every round.
def bench_wide(rounds=7, iters=4):
    import json, os
    from d9d_amd.module.block.attention.linear.gated_deltanet import (
        _GdnChunkFunction, chunk_gated_delta_rule,
    )

    do = torch.randn(B, H, S, D, device="cuda").bfloat16()

    def fwd(kernel):
        with torch.no_grad():
            if kernel:
                return chunk_gated_delta_rule(q, k, v, beta, g)
            return _chunk_gated_delta_rule_torch(q, k, v, beta, g)

    def fwd_bwd(kernel):
        os.environ["D9D_GDN_BWD_SCAN"] = "1" if kernel else "0"
        leaves = [t.detach().requires_grad_(True) for t in (q, k, v, beta, g)]
        out = _GdnChunkFunction.apply(*leaves, 64, kernel, None)
        out.backward(do)
        return [out.detach()] + [t.grad for t in leaves]

    def window(fn, kernel):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            fn(kernel)
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / iters

    # same inputs, both paths: the results must agree before the times count
    for name, a, b in zip(("out", "dq", "dk", "dv", "dbeta", "dg"), fwd_bwd(False), fwd_bwd(True)):
        print(f"kernel vs torch path {name}: max abs diff "
              f"{(a.float() - b.float()).abs().max().item():.3e} (max abs {a.float().abs().max().item():.3g})")
    res = {"shape": [B, H, S, D], "rounds": rounds, "iters": iters}
    for what, fn in (("fwd", fwd), ("fwd_bwd", fwd_bwd)):
        for kernel in (False, True, False, True):
            fn(kernel)
        times = {False: [], True: []}
        for _ in range(rounds):
            for kernel in times:
                times[kernel].append(window(fn, kernel))
        for kernel, name in ((False, "torch"), (True, "kernel")):
            ts = times[kernel]
            res[f"{what}_{name}_ms"] = round(statistics.median(ts), 4)
            res[f"{what}_{name}_min_ms"] = round(min(ts), 4)
            res[f"{what}_{name}_max_ms"] = round(max(ts), 4)
            print(f"gdn D={D} {what} ({name} path): median {statistics.median(ts):.3f} ms"
                  f"  min {min(ts):.3f}  max {max(ts):.3f}")
    os.environ.pop("D9D_GDN_BWD_SCAN")
    print(json.dumps(res))

if D == 128 and "--bwd-leaf" not in sys.argv:
    bench_wide()
    sys.exit(0)

bench_bwd_leaf()
if "--bwd-leaf" in sys.argv:
    sys.exit(0)

def bench(fn, name, flops):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(10):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = statistics.median(ts)
    print(f"{name}: {t*1e3:.2f} ms  {flops/t/1e12:.1f} TF/s")

# per chunk of 64: KK(64*64*64) + K@S + Q@S + N@R + K^T@R (64*64*64 each)
# + solve ~64^3/2 -> ~5.5 * 2*64^3 FLOP per chunk per (B,H)
chunks = S // 64
fl = B * H * chunks * 5.5 * 2 * 64**3
bench(lambda: ext.gdn_chunk_fwd(q, k, v, beta, g, False, False, False), "gdn_chunk_fwd(kernel)", fl)
bench(lambda: _chunk_gated_delta_rule_torch(q.float(), k.float(), v.float(), beta, g),
      "gdn_chunk_fwd(torch WY)", fl)

C = 1024
x = torch.randn(B, S, C, device="cuda", dtype=torch.bfloat16)
w = torch.randn(C, 4, device="cuda", dtype=torch.bfloat16)
by = 2 * B * S * C * 2  # read+write bf16
bench(lambda: ext.causal_conv_silu_fwd(x, w), "causal_conv_silu_fwd", 0.001)
fn = lambda: ext.causal_conv_silu_fwd(x, w)
fn(); torch.cuda.synchronize()
ts = []
for _ in range(10):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
t = statistics.median(ts)
print(f"causal_conv_silu_fwd: {by/t/1e12:.2f} TB/s")

# backward: derived closed-form vs autograd through the torch WY graph
from d9d_amd.module.block.attention.linear.gated_deltanet import _chunk_gdn_backward

qf, kf, vf = q.float(), k.float(), v.float()
do = torch.randn(B, H, S, D, device="cuda")

def bwd_derived():
    return _chunk_gdn_backward(qf, kf, vf, beta, g, do)

def bwd_autograd():
    with torch.enable_grad():
        qs = qf.detach().requires_grad_(True)
        ks = kf.detach().requires_grad_(True)
        vs = vf.detach().requires_grad_(True)
        bs = beta.detach().requires_grad_(True)
        gs = g.detach().requires_grad_(True)
        ref = _chunk_gated_delta_rule_torch(qs, ks, vs, bs, gs)
        return torch.autograd.grad(ref, (qs, ks, vs, bs, gs), do)

bench(bwd_derived, "gdn bwd (derived)", 3 * fl)
bench(bwd_autograd, "gdn bwd (autograd-through-graph)", 3 * fl)
