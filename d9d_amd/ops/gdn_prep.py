"""GatedDeltaNet prologue: what the block does between its short convs / gate
projections and `chunk_gated_delta_rule`.

    qn, kn = l2norm(q), l2norm(k)   expanded from Hkv to H heads, (B, H, S, Dk)
    vt     = v                      (B, H, S, Dv)
    beta   = sigmoid(b_raw)         (B, H, S) fp32
    g      = logsigmoid(a_raw)                              log-sigmoid gate
           = -exp(A_log) * softplus(a_raw + dt_bias)        Mamba gate

GPU, bf16 inputs, head dims 64 / 128: one HIP kernel each way
(csrc/gdn_prep.hip), outputs in the dtypes the chunk kernels read (bf16 rows,
fp32 gates). Anything else, and `D9D_GDN_PREP=0`: the torch chain below, which
is also the specification of the kernels.
"""

import os

import torch
import torch.nn.functional as F

from ._ext import get_ext

_PREP_HEAD_DIMS = (64, 128)


def softplus(x: torch.Tensor) -> torch.Tensor:
    """max(x, 0) + log1p(exp(-|x|)), without F.softplus's linear cut-over."""
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def mamba_decay(a_raw: torch.Tensor, A_log: torch.Tensor, dt_bias: torch.Tensor) -> torch.Tensor:
    """Mamba-style log decay of (..., H) pre-activations, in fp32."""
    return -torch.exp(A_log.float()) * softplus(a_raw.float() + dt_bias.float())


def gdn_prepare_eager(q, k, v, b_raw, a_raw, A_log=None, dt_bias=None):
    """The prologue as a chain of torch ops (any device, any dtype): fp32
    qn, kn, beta, g and vt in v's dtype, as permuted views."""
    H, Hkv = v.shape[2], q.shape[2]
    if H != Hkv:  # GQA expansion
        rep = H // Hkv
        q = q.repeat_interleave(rep, dim=2)
        k = k.repeat_interleave(rep, dim=2)
    # L2-normalize q/k per head (delta-rule convention)
    q = F.normalize(q.float(), dim=-1)
    k = F.normalize(k.float(), dim=-1)
    beta = torch.sigmoid(b_raw.float())  # (B,S,H)
    if A_log is None:
        g = F.logsigmoid(a_raw.float())
    else:
        g = mamba_decay(a_raw, A_log, dt_bias)
    return (
        q.permute(0, 2, 1, 3),
        k.permute(0, 2, 1, 3),
        v.permute(0, 2, 1, 3).to(v.dtype),
        beta.permute(0, 2, 1),
        g.permute(0, 2, 1),
    )


def use_prep_kernels(q, k, v, b_raw, a_raw) -> bool:
    """The HIP prologue serves bf16 device tensors at head dims 64 / 128."""
    return (
        q.is_cuda
        and all(t.dtype == torch.bfloat16 for t in (q, k, v, b_raw, a_raw))
        and q.shape[-1] in _PREP_HEAD_DIMS
        and v.shape[-1] in _PREP_HEAD_DIMS
        and os.environ.get("D9D_GDN_PREP", "1") != "0"
    )


def _gate_params(A_log, dt_bias):
    if A_log is None and dt_bias is None:
        return None, None
    # one without the other goes through as it is: the extension refuses it
    return tuple(
        None if t is None else t.detach().float().contiguous() for t in (A_log, dt_bias)
    )


def prep_fwd_kernel(q, k, v, b_raw, a_raw, A_log, dt_bias):
    return get_ext().gdn_prep_fwd(
        q.contiguous(), k.contiguous(), v.contiguous(),
        b_raw.contiguous(), a_raw.contiguous(), *_gate_params(A_log, dt_bias),
    )


def prep_bwd_kernel(q, k, b_raw, a_raw, A_log, dt_bias, dqn, dkn, dvt, dbeta, dg):
    """The incoming gradients go to the kernel in fp32; (dq, dk, dv, db_raw,
    da_raw) come back bf16, (dA_log, ddt_bias) in the parameters' dtype."""
    grads = get_ext().gdn_prep_bwd(
        q.contiguous(), k.contiguous(), b_raw.contiguous(), a_raw.contiguous(),
        *_gate_params(A_log, dt_bias),
        *(t.float().contiguous() for t in (dqn, dkn, dvt, dbeta, dg)),
    )
    if A_log is not None:
        grads[5] = grads[5].to(A_log.dtype)
        grads[6] = grads[6].to(dt_bias.dtype)
    return tuple(grads)


class _GdnPrepFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, b_raw, a_raw, A_log, dt_bias):
        ctx.save_for_backward(q, k, b_raw, a_raw, A_log, dt_bias)
        return tuple(prep_fwd_kernel(q, k, v, b_raw, a_raw, A_log, dt_bias))

    @staticmethod
    def backward(ctx, dqn, dkn, dvt, dbeta, dg):
        return prep_bwd_kernel(*ctx.saved_tensors, dqn, dkn, dvt, dbeta, dg)


def gdn_prepare(q, k, v, b_raw, a_raw, *, A_log=None, dt_bias=None):
    """q, k (B, S, Hkv, Dk), v (B, S, H, Dv), b_raw, a_raw (B, S, H) ->
    (qn, kn, vt, beta, g), see the module docstring. `A_log` and `dt_bias`
    ((H,), both or neither) select the Mamba gate.

    Autograd rounds a gradient to its tensor's dtype, so the gradients of the
    bf16 qn, kn reach this op's backward in bf16. A caller that has them in
    fp32 and wants them summed over the head group and projected before any
    rounding (the GatedDeltaNet block) calls `prep_bwd_kernel` itself."""
    if use_prep_kernels(q, k, v, b_raw, a_raw):
        return _GdnPrepFunction.apply(q, k, v, b_raw, a_raw, A_log, dt_bias)
    return gdn_prepare_eager(q, k, v, b_raw, a_raw, A_log, dt_bias)
