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
