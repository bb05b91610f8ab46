"""Kernel-edge cases on the CPU paths.

Runs every case of tests/kernel_refs.py through the op's CPU path (or, for
the raw extension entry points that have none, a plain-torch fp32
reimplementation) against the fp64 reference. This validates the references
and the case generators without a GPU; tests/test_kernel_edges_gpu.py runs
the same cases on the HIP kernels.
"""

import pytest
import torch

from tests import kernel_refs as kr

BOTH = [False, True]


# ---- RMSNorm -----------------------------------------------------------------


def _rms_cpu(x, w, dy, zero_centered):
    from d9d_amd.ops.rms_norm import _rms_norm_ref_bwd, _rms_norm_ref_fwd

    y, inv = _rms_norm_ref_fwd(x, w, kr.RMS_EPS, zero_centered)
    dx, dw = _rms_norm_ref_bwd(x, w, dy, inv, zero_centered)
    return y, inv, dx, dw


@pytest.mark.parametrize("zero_centered", BOTH)
@pytest.mark.parametrize(
    "shape", kr.RMS_HEAD_SHAPES + kr.RMS_SMALL_SHAPES + kr.RMS_LDS_SHAPES, ids=str
)
def test_rms_norm_edges_cpu(shape, zero_centered):
    kr.check_rms(_rms_cpu, *shape, zero_centered)


def test_rms_norm_4d_cpu():
    from d9d_amd.ops import rms_norm

    x, w, dy = kr.rms_case(24, 64)
    x4 = x.view(2, 3, 4, 64).clone().requires_grad_(True)
    w4 = w.clone().requires_grad_(True)
    y = rms_norm(x4, w4, eps=kr.RMS_EPS)
    y.backward(dy.view(2, 3, 4, 64))
    ry, _, rdx, rdw = kr.rms_ref(x, w, dy, False)
    kr.assert_close(y.view(24, 64), ry, kr.TOL_RMS_Y, "y")
    kr.assert_close(x4.grad.view(24, 64), rdx, kr.TOL_RMS_DX, "dx")
    kr.assert_close(w4.grad, rdw, kr.TOL_RMS_DW, "dw")


# ---- CCE ---------------------------------------------------------------------


def _cce_fwd_cpu(e, c, targets, vocab_start):
    from d9d_amd.ops.cce import _chunk_fwd

    return _chunk_fwd(e.float(), c, targets, vocab_start)


@pytest.mark.parametrize("shape", kr.CCE_FWD_SHAPES, ids=str)
def test_cce_fwd_edges_cpu(shape):
    kr.check_cce_fwd(_cce_fwd_cpu, *shape)


@pytest.mark.parametrize("shape", [(130, 1000, 320), (70, 333, 1024)], ids=str)
def test_cce_fwd_rounded_lse_cpu(shape):
    """The bf16 CPU path takes its lse from bf16-rounded logits, which is
    what the kernel's third output reproduces."""
    from d9d_amd.ops.cce import _chunk_fwd

    kr.check_cce_rounded_lse(lambda e, c, t: _chunk_fwd(e, c, t, 0)[0], *shape)


def test_cce_fwd_vocab_shards_cpu():
    kr.check_cce_vocab_parallel(_cce_fwd_cpu)


def _dlogits_fp32(logits, lse, targets, dl, dlse, vocab_start, eps):
    """Plain-torch fp32 version of the in-place dlogits entry point."""
    z = logits.float()
    p = torch.exp(z - lse.unsqueeze(1))
    local = torch.where(targets == kr.IGNORE, torch.full_like(targets, -1), targets - vocab_start)
    is_tgt = torch.arange(z.shape[1]).unsqueeze(0) == local.unsqueeze(1)
    if eps > 0:
        p = torch.where((p < eps) & ~is_tgt, torch.zeros_like(p), p)
    gp = dl + dlse if dlse is not None else dl
    return (p * gp.unsqueeze(1) - is_tgt.float() * dl.unsqueeze(1)).to(torch.bfloat16)


@pytest.mark.parametrize("eps", kr.CCE_FILTER_EPS)
@pytest.mark.parametrize("vocab_start", [0, 1000])
@pytest.mark.parametrize("with_dlse", BOTH)
@pytest.mark.parametrize("shape", kr.CCE_DLOGITS_SHAPES, ids=str)
def test_cce_dlogits_edges_cpu(shape, with_dlse, vocab_start, eps):
    kr.check_cce_dlogits(_dlogits_fp32, *shape, vocab_start, with_dlse, eps)


def test_cce_end_to_end_cpu_is_unfiltered():
    """The eager path ignores filter_eps (documented): with the default
    "auto" it matches the UNFILTERED fp64 reference, and the filtered
    reference differs from it on this case."""
    from d9d_amd.ops.cce import linear_cross_entropy

    e, c, targets = kr.cce_case(130, 1001, 192)
    e32 = e.float().requires_grad_(True)
    c32 = c.float().requires_grad_(True)
    loss = linear_cross_entropy(e32, c32, targets, reduction="mean")
    loss.backward()
    rloss, rde, rdc = kr.cce_e2e_ref(e, c, targets, 0.0)
    kr.assert_close(loss, rloss, kr.TOL_FP32, "loss")
    kr.assert_close(e32.grad, rde, kr.TOL_FP32, "de")
    kr.assert_close(c32.grad, rdc, kr.TOL_FP32, "dc")
    _, fde, _ = kr.cce_e2e_ref(e, c, targets, 2.0 ** -12)
    assert not torch.equal(fde, rde)


# ---- Router ------------------------------------------------------------------


def _router_cpu(logits, bias, K, renorm, dtop):
    from d9d_amd.ops.router import router_topk

    z = logits.clone().requires_grad_(True)
    top, idx = router_topk(z, bias, K, renorm)
    top.backward(dtop)
    return top.detach(), idx, z.grad


@pytest.mark.parametrize("renorm", BOTH)
@pytest.mark.parametrize("bias_kind", kr.ROUTER_BIAS)
@pytest.mark.parametrize("shape", kr.ROUTER_SHAPES, ids=str)
def test_router_edges_cpu(shape, bias_kind, renorm):
    kr.check_router(_router_cpu, *shape, bias_kind, renorm)


def test_router_reference_tie_rule():
    """The reference itself breaks ties toward the lower index (torch.topk's
    tie order is unspecified, so the CPU path is not asserted here)."""
    logits, K, want = kr.router_tie_case()
    _, idx, keep, _ = kr.router_ref(logits, None, K, True)
    assert torch.equal(idx, want)
    assert not bool(keep.any())  # exact ties are never "decided by a margin"


def test_router_top_k_above_experts_raises():
    from d9d_amd.ops.router import router_topk

    with pytest.raises(ValueError, match="top_k"):
        router_topk(torch.randn(4, 3), None, 4)


# ---- MoE permute / combine ----------------------------------------------------


def _permute_run(device):
    def run(tokens, indices, probs, E, grad_rows):
        from d9d_amd.ops import moe_permute

        t = tokens.to(device).requires_grad_(True)
        perm, pprobs, _, tpe = moe_permute(t, indices.to(device), probs.to(device), E)
        perm.backward(grad_rows.to(device))
        return perm.detach(), pprobs, tpe, t.grad

    return run


def _unpermute_run(device):
    def run(tokens, indices, probs, E, expert_out, grad_out):
        from d9d_amd.ops import moe_permute, moe_unpermute

        _, pprobs, ctx, _ = moe_permute(
            tokens.to(device), indices.to(device), probs.to(device), E
        )
        eo = expert_out.to(device).requires_grad_(True)
        pp = pprobs.detach().clone().requires_grad_(True)
        out = moe_unpermute(eo, pp, ctx)
        out.backward(grad_out.to(device))
        return out.detach(), eo.grad, pp.grad

    return run


MOE_CASES = [(*s, False) for s in kr.MOE_SHAPES] + [(64, 100, 16, 4, True)]


@pytest.mark.parametrize("case", MOE_CASES, ids=str)
def test_moe_permute_edges_cpu(case):
    kr.check_moe_permute(_permute_run("cpu"), *case)


@pytest.mark.parametrize("case", MOE_CASES, ids=str)
def test_moe_unpermute_edges_cpu(case):
    kr.check_moe_unpermute(_unpermute_run("cpu"), *case)


def test_moe_permute_fp32_cpu():
    kr.check_moe_permute(_permute_run("cpu"), 37, 4, 8, 2, dtype=torch.float32)


# ---- RoPE --------------------------------------------------------------------


def _rope_cpu(q, k, cos, sin, gq, gk):
    from d9d_amd.module.block.positional import apply_rotary_emb

    q32 = q.float().requires_grad_(True)
    k32 = k.float().requires_grad_(True)
    qo = apply_rotary_emb(q32, cos, sin)
    ko = apply_rotary_emb(k32, cos, sin)
    ((qo * gq.float()).sum() + (ko * gk.float()).sum()).backward()
    return qo.detach(), ko.detach(), q32.grad, k32.grad


@pytest.mark.parametrize("shape", kr.ROPE_SHAPES, ids=str)
def test_rope_edges_cpu(shape):
    kr.check_rope(_rope_cpu, *shape)


def test_rope_expanded_cos_sin_cpu():
    kr.check_rope(_rope_cpu, 2, 33, 2, 2, 64, 64, expanded=True)


# ---- Attention ---------------------------------------------------------------


def attn_run(device):
    def run(case, use_dlse, backward):
        from d9d_amd.ops.attention import flash_attn_func

        q, k, v = (case[n].to(device).requires_grad_(backward) for n in ("q", "k", "v"))
        sinks = case["sinks"]
        if sinks is not None:
            sinks = sinks.to(device).requires_grad_(backward)
        out, lse = flash_attn_func(
            q, k, v, causal=case["causal"], softmax_scale=case["scale"],
            window_size=(case["window_left"], -1), sinks=sinks, return_lse=True,
            q_offset=case["q_offset"],
        )
        got = dict(out=out.detach(), lse=lse.detach())
        if backward:
            loss = (out.float() * case["dout"].to(device).float()).sum()
            if use_dlse:
                loss = loss + (lse * case["dlse"].to(device)).sum()
            loss.backward()
            got.update(dq=q.grad, dk=k.grad, dv=v.grad,
                       dsinks=sinks.grad if sinks is not None else None)
        return got

    return run


def attn_varlen_run(device):
    def run(case, use_dlse):
        from d9d_amd.ops.attention import flash_attn_varlen_func

        q, k, v = (case[n].to(device).requires_grad_(True) for n in ("q", "k", "v"))
        sinks = case["sinks"]
        if sinks is not None:
            sinks = sinks.to(device).requires_grad_(True)
        out, lse = flash_attn_varlen_func(
            q, k, v, case["cu_q"].to(device), case["cu_k"].to(device),
            causal=case["causal"], softmax_scale=case["scale"],
            window_size=(case["window_left"], -1), sinks=sinks, return_lse=True,
        )
        loss = (out.float() * case["dout"].to(device).float()).sum()
        if use_dlse:
            loss = loss + (lse * case["dlse"].to(device)).sum()
        loss.backward()
        return dict(out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad,
                    dv=v.grad, dsinks=sinks.grad if sinks is not None else None)

    return run


ATTN_HEAD_DIMS = [16, 32, 40, 80, 96, 128]
ATTN_WINDOWS = [0, 5, 16, 63, 64, 200]  # 200 == S: the window covers everything
ATTN_Q_OFFSETS = [(70, 200, 130), (64, 256, 64)]


@pytest.mark.parametrize("D", ATTN_HEAD_DIMS)
def test_attn_head_dims_cpu(D):
    case = kr.attn_case(1, 130, 130, 4, 2, D)
    kr.check_attn_plant(case)
    kr.check_attn(attn_run("cpu"), case)


@pytest.mark.parametrize("sq,skv,off", ATTN_Q_OFFSETS)
def test_attn_q_offset_cpu(sq, skv, off):
    case = kr.attn_case(1, sq, skv, 4, 2, 64, q_offset=off)
    kr.check_attn_plant(case)
    kr.check_attn(attn_run("cpu"), case)


@pytest.mark.parametrize("with_sinks", BOTH)
@pytest.mark.parametrize("window_left", ATTN_WINDOWS)
def test_attn_window_cpu(window_left, with_sinks):
    case = kr.attn_case(1, 200, 200, 4, 2, 64, window_left=window_left, with_sinks=with_sinks)
    kr.check_attn_plant(case)
    kr.check_attn(attn_run("cpu"), case)


def test_attn_noncausal_ragged_cpu():
    case = kr.attn_case(2, 130, 130, 4, 2, 64, causal=False)
    kr.check_attn(attn_run("cpu"), case)


VARLEN_CASES = {
    "window16": dict(lens_q=[1, 37, 128, 129], lens_k=[1, 37, 128, 129], window_left=16),
    "sinks": dict(lens_q=[1, 37, 128, 129], lens_k=[1, 37, 128, 129], with_sinks=True),
    "cross": dict(lens_q=[64, 130], lens_k=[200, 300]),
}


@pytest.mark.parametrize("name", list(VARLEN_CASES))
def test_attn_varlen_cpu(name):
    case = kr.attn_varlen_case(Hq=4, Hkv=2, D=64, **VARLEN_CASES[name])
    kr.check_attn_varlen(attn_varlen_run("cpu"), case)


@pytest.mark.parametrize("with_sinks", BOTH)
def test_attn_dlse_cpu(with_sinks):
    case = kr.attn_case(1, 130, 130, 4, 2, 64, with_sinks=with_sinks)
    kr.check_attn(attn_run("cpu"), case, use_dlse=True)


@pytest.mark.parametrize("with_sinks", BOTH)
def test_attn_varlen_dlse_cpu(with_sinks):
    case = kr.attn_varlen_case([37, 130], [37, 130], 4, 2, 64, with_sinks=with_sinks)
    kr.check_attn_varlen(attn_varlen_run("cpu"), case, use_dlse=True)


# ---- GatedDeltaNet -------------------------------------------------------------


def _gdn_emul_fwd(case):
    return kr.gdn_chunk_emul(case, cast=True)


def gdn_op_run(device):
    """Forward and backward through chunk_gated_delta_rule with bf16 q, k, v
    leaves; packed documents when the case carries `cu`."""

    def run(case, docs=None):
        from d9d_amd.module.block.attention.linear.gated_deltanet import chunk_gated_delta_rule

        q, k, v, beta, g = (
            case[n].to(device).requires_grad_(True) for n in ("q", "k", "v", "beta", "g")
        )
        out = chunk_gated_delta_rule(q, k, v, beta, g, cu_seqlens=case.get("cu"))
        assert out.dtype == torch.bfloat16
        (out.float() * case["dout"].to(device).float()).sum().backward()
        return dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dbeta=beta.grad,
                    dg=g.grad)

    return run


@pytest.mark.parametrize("shape", kr.GDN_FWD_SHAPES, ids=str)
def test_gdn_fwd_emulation_cpu(shape):
    """The yardstick with the kernel's bf16 casts stays at or below half of
    every forward tolerance, on every planted forward case."""
    kr.check_gdn_fwd(_gdn_emul_fwd, *shape, tol_scale=0.5)


@pytest.mark.parametrize("shape", kr.GDN_FWD_SHAPES, ids=str)
def test_gdn_fwd_cpu(shape):
    """The op's torch path gives `out`; the aux outputs and the final state
    have no CPU path and come from the uncast chunk formulation."""
    from d9d_amd.module.block.attention.linear.gated_deltanet import chunk_gated_delta_rule

    def run(case):
        got = kr.gdn_chunk_emul(case, cast=False)
        with torch.no_grad():
            got["out"] = chunk_gated_delta_rule(
                case["q"], case["k"], case["v"], case["beta"], case["g"]
            )
        return got

    kr.check_gdn_fwd(run, *shape, tol_scale=0.5)


def test_gdn_planted_case_exposes_a_truncated_solve():
    """A solve cut after its second-order term is far outside the tolerance
    on the planted case (and the full solve is inside, above)."""
    case = kr.gdn_case(2, 3, 64)
    ref = kr.gdn_step_ref(case)
    broken = kr.gdn_chunk_emul(case, cast=True, solve_order=2)
    assert kr.tol_needed(broken["out"], ref["out"]) > 100 * kr.TOL_GDN_OUT["atol"]
    with pytest.raises(AssertionError, match="out"):
        kr.check_gdn_fwd(lambda c: kr.gdn_chunk_emul(c, cast=True, solve_order=2), 2, 3, 64)


@pytest.mark.parametrize("shape", kr.GDN_BWD_SHAPES, ids=str)
def test_gdn_bwd_emulation_cpu(shape):
    kr.check_gdn_bwd(lambda c: kr.gdn_chunk_emul(c, cast=True, backward=True), *shape,
                     tol_scale=0.5)


@pytest.mark.parametrize("shape", kr.GDN_BWD_SHAPES, ids=str)
def test_gdn_bwd_cpu(shape):
    kr.check_gdn_bwd(gdn_op_run("cpu"), *shape)


def _gdn_emul_varlen(case, docs):
    parts = [kr.gdn_chunk_emul(d, cast=True, backward=True) for d in docs]
    return kr._gdn_cat_docs(parts, ("out",) + kr.GDN_GRADS)


def test_gdn_varlen_bwd_emulation_cpu():
    kr.check_gdn_varlen_bwd(_gdn_emul_varlen, kr.GDN_VARLEN_LENS, 3, tol_scale=0.5)


def test_gdn_varlen_bwd_cpu():
    kr.check_gdn_varlen_bwd(gdn_op_run("cpu"), kr.GDN_VARLEN_LENS, 3)


def test_gdn_bwd_scan_emulation_cpu():
    """drhs = dv / beta and dS0 from the emulation's autograd, at half of
    the tolerances the reverse-scan kernel is held to."""

    def run(case):
        em = kr.gdn_chunk_emul(case, cast=True, backward=True)
        return em["dv32"] / case["beta"].unsqueeze(-1), em["ds0"]

    kr.check_gdn_bwd_scan(run, 2, 3, 100, tol_scale=0.5)


def conv_run(device):
    """The module's conv (the fused kernels on a GPU in bf16, the eager
    pad/conv1d/silu chain in fp32 on the CPU)."""

    def run(x, w, dy):
        from d9d_amd.module.block.attention.linear.gated_deltanet import (
            CausalShortDepthwiseConv1d,
        )

        dtype = torch.bfloat16 if device != "cpu" else torch.float32
        conv = CausalShortDepthwiseConv1d(w.shape[0], w.shape[1], device=device, dtype=dtype)
        with torch.no_grad():
            conv.weight.copy_(w)
        xd = x.to(device=device, dtype=dtype).requires_grad_(True)
        y = conv(xd)
        if device != "cpu":  # the fused kernels ran
            assert type(y.grad_fn).__name__ == "_CausalConvSiluFunctionBackward"
        y.backward(dy.to(device=device, dtype=dtype))
        return y.detach(), xd.grad, conv.weight.grad

    return run


@pytest.mark.parametrize("shape", kr.CONV_SHAPES, ids=str)
def test_conv_silu_edges_cpu(shape):
    kr.check_conv(conv_run("cpu"), *shape)


# ---- Stochastic rounding and AdamW ------------------------------------------------

SR_SEEDS = [7, 123]


@pytest.mark.parametrize("seed", SR_SEEDS + [2 ** 62 + 12345])
@pytest.mark.parametrize("n", kr.SR_COPY_SIZES)
def test_sr_oracle_edges(n, seed):
    """The bit oracle on its own cases: grid values exact, NaN stays NaN,
    everything else a neighbour."""
    kr.check_sr_copy(kr.sr_oracle, n, seed)


@pytest.mark.parametrize("seed", SR_SEEDS)
def test_sr_oracle_is_unbiased(seed):
    """The documented noise is uniform enough: round-up frequency within 6
    sigma of the fraction. (Small seeds only permute the counters, so two of
    them are not two independent samples.)"""
    kr.check_sr_statistics(kr.sr_oracle, seed)


def test_sr_oracle_vector_and_tail_salts_differ():
    """The same element index draws different bits in the vector body and in
    the scalar tail (n = 7: elements 4..6 are tail)."""
    body = kr.sr_noise16(8, 7)[4:7]
    tail = kr.sr_noise16(7, 7)[4:7]
    assert (body != tail).all()


@pytest.mark.parametrize("seed", SR_SEEDS)
def test_sr_cpu_path(seed):
    """_sr_cpu draws other bits than the kernel, so only: floor or the next
    bf16 away from zero, and the same statistic."""
    from d9d_amd.ops.stochastic import _sr_cpu

    src, _ = kr.sr_copy_case(1027)
    kr.check_sr_neighbours(_sr_cpu(src, seed), src)
    kr.check_sr_statistics(_sr_cpu, seed)


def adamw_single_run(device):
    def run(p, g, m, v, lr, weight_decay, step, seed):
        from d9d_amd.ops import adamw_stochastic_bf16_

        p, g, m, v = (t.to(device) for t in (p, g, m, v))
        adamw_stochastic_bf16_(
            p, g, m, v, lr=lr, beta1=kr.ADAMW_BETAS[0], beta2=kr.ADAMW_BETAS[1],
            eps=kr.ADAMW_EPS, weight_decay=weight_decay, step=step, seed=seed,
        )
        return p, m, v

    return run


@pytest.mark.parametrize("hyper", kr.ADAMW_HYPER, ids=lambda h: f"lr{h['lr']}")
@pytest.mark.parametrize("n", kr.ADAMW_SIZES)
def test_adamw_edges_cpu(n, hyper):
    kr.check_adamw(adamw_single_run("cpu"), n, hyper)


def test_adamw_sr_mean_cpu():
    kr.check_adamw_sr_mean(adamw_single_run("cpu"))


def test_adamw_check_sees_dropped_weight_decay_and_nearest_rounding():
    """The checker itself: a step without the decay term, and one that
    rounds to nearest, both fail it."""
    base = adamw_single_run("cpu")

    def no_decay(p, g, m, v, lr, weight_decay, step, seed):
        return base(p, g, m, v, lr, 0.0, step, seed)

    def nearest(p, g, m, v, lr, weight_decay, step, seed):
        rp, rm, rv = kr.adamw_ref(p, g, m, v, lr, weight_decay, step)
        return rp.float().to(torch.bfloat16), rm.float(), rv.float()

    with pytest.raises(AssertionError):
        kr.check_adamw(no_decay, 4097, kr.ADAMW_HYPER[0])
    with pytest.raises(AssertionError):
        kr.check_adamw(nearest, kr.SR_BIG, kr.ADAMW_HYPER[0])
    with pytest.raises(AssertionError):
        kr.check_adamw_sr_mean(nearest)


def test_adamw_multi_cases_are_what_they_say():
    sizes = kr.adamw_multi_big_sizes()
    assert sizes.count(0) == 1 and len(sizes) == 52
    small = kr.ADAMW_MULTI_SMALL
    assert 0 in small["sizes"] and len(set(small["steps"])) > 3
    assert any(n % 8 == 4 for n in small["sizes"])   # partial slot with one 4-vector


def check_stochastic_adamw_class(device):
    """Two steps of optim.StochasticAdamW against per-tensor calls of the
    single-tensor op with the documented seed: a parameter without a grad in
    step 1 (it consumes no idx and its own step lags), an fp32 grad, an empty
    parameter, two groups with different hyperparameters."""
    from d9d_amd.ops import adamw_stochastic_bf16_
    from d9d_amd.optim import StochasticAdamW

    sizes = [(40, 25), (0,), (37,), (4097,), (5,)]
    gen = kr._gen(8400)
    params = [torch.randn(*s, generator=gen).to(torch.bfloat16).to(device) for s in sizes]
    params = [torch.nn.Parameter(p) for p in params]
    groups = [
        dict(params=params[:3], lr=1e-2, weight_decay=0.1),
        dict(params=params[3:], lr=1e-3, weight_decay=0.0, betas=(0.8, 0.9)),
    ]
    opt = StochasticAdamW(groups, seed=5)
    mine = [p.detach().clone().view(-1) for p in params]
    ms = [torch.zeros(p.numel(), device=device) for p in params]
    vs = [torch.zeros(p.numel(), device=device) for p in params]
    steps = [0] * len(params)
    for step_count in (1, 2):
        grads = [torch.randn(*s, generator=gen) for s in sizes]
        for i, p in enumerate(params):
            if i == 2 and step_count == 1:
                p.grad = None
            elif i == 3:                      # an fp32 grad on a bf16 parameter
                if hasattr(p, "grad_dtype"):
                    p.grad_dtype = None
                p.grad = grads[i].to(device)
            else:
                p.grad = grads[i].to(torch.bfloat16).to(device)
        opt.step()
        idx = 0
        for i, p in enumerate(params):
            if p.grad is None:
                continue
            idx += 1
            steps[i] += 1
            group = groups[0] if i < 3 else groups[1]
            b1, b2 = group.get("betas", (0.9, 0.95))
            adamw_stochastic_bf16_(
                mine[i], p.grad.reshape(-1).to(torch.bfloat16), ms[i], vs[i],
                lr=group["lr"], beta1=b1, beta2=b2, eps=1e-8,
                weight_decay=group["weight_decay"], step=steps[i],
                seed=kr.stochastic_adamw_seed(5, step_count, idx),
            )
        for i, p in enumerate(params):
            kr.assert_same_bits(p.detach().view(-1), mine[i], f"step {step_count} param {i}")
            if steps[i]:
                kr.assert_same_bits(opt.state[p]["exp_avg"].view(-1), ms[i], f"exp_avg {i}")
                kr.assert_same_bits(opt.state[p]["exp_avg_sq"].view(-1), vs[i], f"exp_avg_sq {i}")
                assert opt.state[p]["step"] == steps[i]
    assert steps == [2, 2, 1, 2, 2]
    assert not torch.equal(params[0].detach().view(-1).cpu(), torch.zeros(1000).bfloat16())


def test_stochastic_adamw_class_cpu():
    check_stochastic_adamw_class("cpu")


@pytest.mark.parametrize("n", kr.ADD_BF16_SIZES)
def test_add_bf16_into_f32_reference(n):
    kr.check_add_bf16_into_f32(lambda acc, x: acc.add_(x.float()), n)


# ---- SwiGLU ------------------------------------------------------------------------


def silu_run(device):
    def run(a, b, g):
        from d9d_amd.ops import silu_mul

        a_d = a.to(device).requires_grad_(True)
        b_d = b.to(device).requires_grad_(True)
        out = silu_mul(a_d, b_d)
        out.backward(g.to(device))
        return out.detach(), a_d.grad, b_d.grad

    return run


def silu_packed_run(device):
    def run(x, g):
        from d9d_amd.ops.swiglu import silu_mul_packed

        x_d = x.to(device).requires_grad_(True)
        out = silu_mul_packed(x_d)
        out.backward(g.to(device))
        return out.detach(), x_d.grad

    return run


@pytest.mark.parametrize("n", kr.SILU_SIZES)
def test_silu_mul_edges_cpu(n):
    kr.check_silu(silu_run("cpu"), n)


@pytest.mark.parametrize("shape", kr.SILU_PACKED_SHAPES, ids=str)
def test_silu_mul_packed_edges_cpu(shape):
    kr.check_silu_packed(silu_packed_run("cpu"), *shape)
