"""CCE backward per chunk: library-GEMM route against the tile-skipping route
at planted tile densities (bench shape: 16384 rows, V 151669, K 768).

The logits GEMM is common to both routes and left out. Each density plants one
above-threshold logit in a random share of the 64 x 128 tiles; the routes are
timed alternately with device events on the same planted logits.
"""
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch

from d9d_amd.ops._ext import get_ext

R, V, K = 16384, 151669, 768
EPS = 2.0 ** -12
ext = get_ext()
torch.manual_seed(0)
dev = "cuda"
e = torch.randn(R, K, device=dev).to(torch.bfloat16)
c = (torch.randn(V, K, device=dev) * 0.02).to(torch.bfloat16)
base = torch.mm(e, c.t())
lse = torch.logsumexp(base.float(), -1)
dl = torch.full((R,), 1.0 / R, device=dev)
n_rb, n_vt = R // 64, -(-V // 128)
work = torch.empty_like(base)
dc32 = torch.zeros(V, K, device=dev)
de = torch.empty(R, K, dtype=torch.bfloat16, device=dev)
mask = torch.empty(n_rb, n_vt, dtype=torch.uint8, device=dev)


def dense(tg, masked):
    if masked:
        pb = ext.cce_dlogits_mask_(work, lse, tg, dl, None, mask, 0, -100, EPS, True)
        mask.sum()
    else:
        pb = ext.cce_dlogits_(work, lse, tg, dl, None, 0, -100, EPS)
    de.copy_(torch.matmul(pb, c))
    part = torch.matmul(pb.t(), e)
    ext.add_bf16_into_f32_(dc32, part)


def sparse(tg):
    pb = ext.cce_dlogits_mask_(work, lse, tg, dl, None, mask, 0, -100, EPS, False)
    mask.sum()
    ext.cce_bwd_de(pb, c, mask, de)
    ext.cce_bwd_dc(pb, e, mask, dc32, True)


def timed(fn, planted):
    work.copy_(planted)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


print("| planted | tiles set | library GEMMs ms | GEMMs + mask ms | tile-skipping ms |")
print("|---|---|---|---|---|")
for share in (0.02, 0.05, 0.10, 0.15, 0.20, 0.25, 0.35, 0.50, 1.00):
    planted = base.clone()
    tg = torch.full((R,), -100, dtype=torch.int64, device=dev)  # no targets: spikes only
    pick = torch.rand(n_rb, n_vt, device=dev) < share
    rb, vt = pick.nonzero(as_tuple=True)
    rows = rb * 64 + torch.randint(0, 64, rb.shape, device=dev)
    cols = (vt * 128 + torch.randint(0, 128, vt.shape, device=dev)).clamp(max=V - 1)
    planted[rows, cols] = (lse[rows] - 2.0).to(torch.bfloat16)
    fns = {
        "dense": lambda: dense(tg, False),
        "dense+mask": lambda: dense(tg, True),
        "sparse": lambda: sparse(tg),
    }
    times = {k: [] for k in fns}
    for k in fns:
        timed(fns[k], planted)  # warm-up
    for _ in range(5):
        for k in fns:
            times[k].append(timed(fns[k], planted))
    got = float(mask.float().mean())
    print(f"| {share:.0%} | {got:.1%} | {statistics.median(times['dense']):.2f} | "
          f"{statistics.median(times['dense+mask']):.2f} | "
          f"{statistics.median(times['sparse']):.2f} |", flush=True)
    del planted
