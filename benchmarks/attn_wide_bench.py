"""Flash attention at the MLA head dims (qk 192 / v 128) next to (128, 128).

Part 1: forward and backward time and TF/s at B=8, S=4096, Hq=Hkv=16, causal,
for both head-dim pairs in one run. Part 2: at B=2, S=2048 the same two
passes through the eager fp32 oracle on the GPU, which materialises the S^2
scores and is what a user had for qk 192 before the <192, 128> kernels.

FLOPs (causal, so half of S^2): forward 2*B*H*S^2/2*(Dqk+Dv), backward
2*B*H*S^2/2*(3*Dqk+2*Dv). Times are medians of host-clock windows that end in
a device synchronise, after a warm-up of the same shape.
"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import statistics
import time

import torch

from d9d_amd.ops.attention import _eager_attention, flash_attn_func

REPS = 10


def fwd_flops(B, H, S, Dqk, Dv):
    return 2 * B * H * S * S / 2 * (Dqk + Dv)


def bwd_flops(B, H, S, Dqk, Dv):
    return 2 * B * H * S * S / 2 * (3 * Dqk + 2 * Dv)


def timed(fn, setup=None, reps=REPS):
    ts = []
    for _ in range(reps):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg) if setup else fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def bench(attn, label, B, S, H, Dqk, Dv, reps=REPS):
    """Median forward and backward seconds of attn(q, k, v) -> out."""
    mk = lambda d: torch.randn(  # noqa: E731
        B, S, H, d, dtype=torch.bfloat16, device="cuda", requires_grad=True
    )
    q, k, v = mk(Dqk), mk(Dqk), mk(Dv)
    do = torch.randn(B, S, H, Dv, dtype=torch.bfloat16, device="cuda")
    attn(q, k, v).backward(do)  # warm-up of both passes at this shape
    torch.cuda.synchronize()
    t_f = timed(lambda: attn(q, k, v), reps=reps)
    t_b = timed(lambda o: o.backward(do), setup=lambda: attn(q, k, v), reps=reps)
    ff, fb = fwd_flops(B, H, S, Dqk, Dv), bwd_flops(B, H, S, Dqk, Dv)
    print(f"{label} B{B} S{S} H{H} ({Dqk},{Dv}): "
          f"fwd {t_f * 1e3:.2f} ms {ff / t_f / 1e12:.0f} TF/s | "
          f"bwd {t_b * 1e3:.2f} ms {fb / t_b / 1e12:.0f} TF/s | "
          f"fwd+bwd {(t_f + t_b) * 1e3:.2f} ms")
    return t_f, t_b


def main():
    if not torch.cuda.is_available():
        raise SystemExit("attn_wide_bench needs a GPU")
    torch.manual_seed(0)
    flash = lambda q, k, v: flash_attn_func(q, k, v, causal=True)  # noqa: E731
    eager = lambda q, k, v: _eager_attention(  # noqa: E731
        q, k, v, True, q.shape[-1] ** -0.5, (-1, -1), None
    )[0]

    print("-- part 1: kernels, B=8 S=4096 Hq=Hkv=16 causal")
    res = {d: bench(flash, "flash", 8, 4096, 16, *d) for d in [(192, 128), (128, 128)]}
    for i, name in enumerate(["fwd", "bwd"]):
        rate = {d: (fwd_flops, bwd_flops)[i](8, 16, 4096, *d) / res[d][i] for d in res}
        print(f"{name}: (192,128) runs at {rate[(192, 128)] / rate[(128, 128)]:.2f}x "
              f"the (128,128) TF/s")

    print("-- part 2: kernels against the eager oracle, B=2 S=2048 Hq=Hkv=16 causal")
    for d in [(192, 128), (128, 128)]:
        kf, kb = bench(flash, "flash", 2, 2048, 16, *d)
        ef, eb = bench(eager, "eager", 2, 2048, 16, *d, reps=5)
        print(f"({d[0]},{d[1]}): flash fwd+bwd {(kf + kb) * 1e3:.2f} ms, eager "
              f"{(ef + eb) * 1e3:.2f} ms, flash is {(ef + eb) / (kf + kb):.1f}x faster")
        if d == (192, 128):
            assert kf + kb < ef + eb, "wide flash fwd+bwd is not faster than eager"


if __name__ == "__main__":
    main()
