"""Flash attention op — the framework's single SDPA implementation.

GPU: hand-written CDNA4 flash-attention kernel (csrc/attention.hip) with
online softmax, causal masking, GQA head packing, optional sliding window,
optional learnable attention sinks, and LSE output (needed for context-
parallel ring merging). CPU: eager fp32 oracle with identical semantics
(reference wrapper: d9d/kernel/flash_attn/function.py).

Layout: q (B, S, Hq, Dqk), k (B, S, Hkv, Dqk), v (B, S, Hkv, Dv),
out (B, S, Hq, Dv), lse (B, Hq, S) natural-log-sum-exp of the scores row.
GPU head dims: Dqk and Dv up to 128 each (the narrower side is zero-padded to
the wider), or Dqk up to 192 with Dv up to 128 (the kernels' <192, 128> pair,
MLA's default shape); anything wider raises ValueError before any launch.
"""

import math

import torch

from ._ext import get_ext


def _eager_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    causal: bool,
    softmax_scale: float,
    window_size: tuple[int, int],
    sinks: torch.Tensor | None,
    q_offset: int = 0,
):
    """fp32 eager oracle. Returns (out, lse). `q_offset` is the global
    position of q row 0 (context parallel: local q block vs gathered KV)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    rep = Hq // Hkv

    q32 = q.float().permute(0, 2, 1, 3)  # (B, Hq, S, D)
    k32 = k.float().permute(0, 2, 1, 3)
    v32 = v.float().permute(0, 2, 1, 3)
    if rep > 1:
        k32 = k32.repeat_interleave(rep, dim=1)
        v32 = v32.repeat_interleave(rep, dim=1)

    scores = torch.matmul(q32, k32.transpose(-1, -2)) * softmax_scale  # (B,Hq,S,Skv)
    Skv = scores.shape[-1]
    q_pos = torch.arange(S, device=q.device).unsqueeze(1) + q_offset
    kv_pos = torch.arange(Skv, device=q.device).unsqueeze(0)
    mask = torch.zeros(S, Skv, dtype=torch.bool, device=q.device)
    if causal:
        mask |= kv_pos > q_pos
    left, right = window_size
    if left >= 0:
        mask |= kv_pos < q_pos - left
    if right >= 0 and not causal:
        mask |= kv_pos > q_pos + right
    scores = scores.masked_fill(mask, float("-inf"))

    if sinks is not None:
        # One virtual "sink" column per head: its logit joins the softmax
        # denominator but contributes no value (reference: flash4 sinks).
        sink_col = sinks.float().view(1, Hq, 1, 1).expand(B, Hq, S, 1)
        full = torch.cat([scores, sink_col], dim=-1)
        lse = torch.logsumexp(full, dim=-1)  # (B,Hq,S)
        p = torch.exp(scores - lse.unsqueeze(-1))
    else:
        lse = torch.logsumexp(scores, dim=-1)
        p = torch.exp(scores - lse.unsqueeze(-1))

    out = torch.matmul(p, v32)  # (B,Hq,S,D)
    return out.permute(0, 2, 1, 3).to(q.dtype), lse


#: head dims up to which one padded D serves q, k and v (the kernels' D = D pairs)
_MAX_SQUARE_HEAD_DIM = 128
#: the one wide kernel pair: qk head dim up to 192 with v head dim up to 128
_MAX_WIDE_QK_HEAD_DIM = 192
_MAX_WIDE_V_HEAD_DIM = 128


def head_dim_route(d_qk: int, d_v: int) -> str:
    """How the GPU path serves a (qk, v) head-dim pair.

    "legacy pad": both dims fit the D = D kernels; the narrower side is
    zero-padded to the wider one. "wide": q, k, v go to the kernel as they
    are and it runs the <192, 128> pair. Anything else raises ValueError.
    """
    if max(d_qk, d_v) <= _MAX_SQUARE_HEAD_DIM:
        return "legacy pad"
    if d_qk <= _MAX_WIDE_QK_HEAD_DIM and d_v <= _MAX_WIDE_V_HEAD_DIM:
        return "wide"
    raise ValueError(
        f"flash attention supports qk head_dim <= {_MAX_WIDE_QK_HEAD_DIM} with "
        f"v head_dim <= {_MAX_WIDE_V_HEAD_DIM}; got qk {d_qk}, v {d_v}"
    )


def _pad_narrow_side(q, k, v, route: str):
    """Zero-pad the narrower of qk / v on the "legacy pad" route: zero V
    columns add nothing to PV, zero q/k columns nothing to the dots. F.pad
    keeps it differentiable; the caller slices out[..., :Dv]."""
    Dq, Dv = q.shape[-1], v.shape[-1]
    if route == "wide" or Dq == Dv:
        return q, k, v
    import torch.nn.functional as F

    if Dv < Dq:
        return q, k, F.pad(v, (0, Dq - Dv))
    return F.pad(q, (0, Dv - Dq)), F.pad(k, (0, Dv - Dq)), v


class _FlashAttnFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, sinks, causal, softmax_scale, window_left, q_offset):
        ext = get_ext()
        # the <192, 128> kernels return a third tensor, out's bf16 rounding
        # residual: the backward's delta = rowsum(dout * out) needs it where
        # the softmax is near one-hot
        out, lse, *out_lo = ext.flash_attn_fwd(
            q.contiguous(), k.contiguous(), v.contiguous(), sinks, None, None,
            causal, softmax_scale, window_left, q_offset,
        )
        ctx.save_for_backward(q, k, v, out, lse, *out_lo,
                              *([sinks] if sinks is not None else []))
        ctx.has_out_lo = bool(out_lo)
        ctx.causal = causal
        ctx.softmax_scale = softmax_scale
        ctx.window_left = window_left
        ctx.q_offset = q_offset
        ctx.has_sinks = sinks is not None
        # unused output grads arrive as None, so the common out-only loss
        # pays nothing for the differentiable lse
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    def backward(ctx, dout, dlse):
        q, k, v, out, lse = ctx.saved_tensors[:5]
        out_lo = ctx.saved_tensors[5] if ctx.has_out_lo else None
        if dout is None:
            dout = torch.zeros_like(out)
        ext = get_ext()
        # The sink only enters through the LSE, which the kernel reads back:
        # dq/dk/dv formulas are unchanged. lse is a differentiable output:
        # d(lse)/dS = P, so dS = P*(dP - delta) + P*dlse (the kernel folds
        # dlse into delta).
        dlse = dlse.float().contiguous() if dlse is not None else None
        dq, dk, dv = ext.flash_attn_bwd(
            dout.contiguous(), q.contiguous(), k.contiguous(), v.contiguous(),
            out.contiguous(), lse, None, None,
            ctx.causal, ctx.softmax_scale, ctx.window_left, ctx.q_offset, dlse,
            out_lo,
        )
        dsinks = None
        if ctx.has_sinks:
            sinks = ctx.saved_tensors[-1]
            # p_sink(b,h,t) = exp(sink_h - lse);
            # dsink_h = sum p_sink * (dlse - delta)
            # with delta = rowsum(dout * out) (analytic sink grad, reference
            # d9d/kernel/flash_attn/function.py dsink).
            delta = (out.float() * dout.float()).sum(-1).permute(0, 2, 1)  # (B,Hq,S)
            if dlse is not None:
                delta = delta - dlse
            p_sink = torch.exp(sinks.float().view(1, -1, 1) - lse)
            dsinks = -(p_sink * delta).sum(dim=(0, 2)).to(sinks.dtype)
        return dq, dk, dv, dsinks, None, None, None, None


def flash_attn_func(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    *,
    causal: bool = True,
    softmax_scale: float | None = None,
    window_size: tuple[int, int] = (-1, -1),
    sinks: torch.Tensor | None = None,
    return_lse: bool = False,
    q_offset: int = 0,
):
    """Scaled-dot-product attention. q (B,S,Hq,Dqk); k (B,S,Hkv,Dqk);
    v (B,S,Hkv,Dv); out (B,S,Hq,Dv). On the GPU Dqk and Dv up to 128 each, or
    Dqk up to 192 with Dv up to 128 (see head_dim_route)."""
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    right_ok = window_size[1] < 0 or causal  # right window only via causality
    if q.is_cuda and right_ok:
        # asymmetric head dims: small ones (e.g. MLA at qk 24, v 16) pad the
        # narrower side; past 128 the kernel takes the two dims as they are
        Dv = v.shape[-1]
        q_in, k_in, v_in = _pad_narrow_side(q, k, v, head_dim_route(q.shape[-1], Dv))
        out, lse = _FlashAttnFunction.apply(
            q_in, k_in, v_in, sinks, causal, softmax_scale, window_size[0], q_offset
        )
        if out.shape[-1] != Dv:
            out = out[..., :Dv]
    else:
        out, lse = _eager_attention(
            q, k, v, causal, softmax_scale, window_size, sinks, q_offset
        )
    if return_lse:
        return out, lse
    return out


def _eager_varlen(q, k, v, cu_q, cu_k, causal, softmax_scale, window_size, sinks):
    """Per-sequence eager oracle for packed (total, H, D) inputs."""
    outs, lses = [], []
    for s in range(cu_q.numel() - 1):
        q_s = q[cu_q[s] : cu_q[s + 1]].unsqueeze(0)
        k_s = k[cu_k[s] : cu_k[s + 1]].unsqueeze(0)
        v_s = v[cu_k[s] : cu_k[s + 1]].unsqueeze(0)
        # causal aligns the END of q with the END of kv
        off = (cu_k[s + 1] - cu_k[s]) - (cu_q[s + 1] - cu_q[s])
        o, l = _eager_attention(
            q_s, k_s, v_s, causal, softmax_scale, window_size, sinks, int(off)
        )
        outs.append(o.squeeze(0))
        lses.append(l.squeeze(0))
    return torch.cat(outs, dim=0), torch.cat(lses, dim=1)


class _FlashAttnVarlenFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, sinks, causal, softmax_scale, window_left):
        ext = get_ext()
        out, lse, *out_lo = ext.flash_attn_fwd(  # out_lo: see _FlashAttnFunction
            q.contiguous(), k.contiguous(), v.contiguous(), sinks, cu_q, cu_k,
            causal, softmax_scale, window_left, 0,
        )
        to_save = [q, k, v, out, lse, cu_q, cu_k, *out_lo]
        ctx.has_out_lo = bool(out_lo)
        if sinks is not None:
            to_save.append(sinks)
        ctx.save_for_backward(*to_save)
        ctx.causal = causal
        ctx.softmax_scale = softmax_scale
        ctx.window_left = window_left
        ctx.has_sinks = sinks is not None
        # unused output grads arrive as None, so the common out-only loss
        # pays nothing for the differentiable lse
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    def backward(ctx, dout, dlse):
        q, k, v, out, lse, cu_q, cu_k = ctx.saved_tensors[:7]
        out_lo = ctx.saved_tensors[7] if ctx.has_out_lo else None
        if dout is None:
            dout = torch.zeros_like(out)
        ext = get_ext()
        dlse = dlse.float().contiguous() if dlse is not None else None
        dq, dk, dv = ext.flash_attn_bwd(
            dout.contiguous(), q.contiguous(), k.contiguous(), v.contiguous(),
            out.contiguous(), lse, cu_q, cu_k,
            ctx.causal, ctx.softmax_scale, ctx.window_left, 0, dlse, out_lo,
        )
        dsinks = None
        if ctx.has_sinks:
            sinks = ctx.saved_tensors[-1]
            delta = (out.float() * dout.float()).sum(-1).permute(1, 0)  # (Hq,total)
            if dlse is not None:
                delta = delta - dlse
            p_sink = torch.exp(sinks.float().view(-1, 1) - lse)
            dsinks = -(p_sink * delta).sum(dim=1).to(sinks.dtype)
        return dq, dk, dv, None, None, dsinks, None, None, None


def flash_attn_varlen_func(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    cu_seqlens_q: torch.Tensor,
    cu_seqlens_k: torch.Tensor | None = None,
    *,
    causal: bool = True,
    softmax_scale: float | None = None,
    window_size: tuple[int, int] = (-1, -1),
    sinks: torch.Tensor | None = None,
    return_lse: bool = False,
):
    """Packed-sequence attention. q (total_q, Hq, Dqk); k (total_k, Hkv, Dqk);
    v (total_k, Hkv, Dv); cu_seqlens (nseq+1,) int32. out is (total_q, Hq, Dv),
    lse (Hq, total_q). Causal masking aligns the end of each sequence's q with
    the end of its kv (flash-attn convention). Head dims as flash_attn_func.
    Reference: d9d/kernel/flash_attn/function.py varlen path."""
    if cu_seqlens_k is None:
        cu_seqlens_k = cu_seqlens_q
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    right_ok = window_size[1] < 0 or causal
    if q.is_cuda and right_ok:
        Dv = v.shape[-1]
        q_in, k_in, v_in = _pad_narrow_side(q, k, v, head_dim_route(q.shape[-1], Dv))
        out, lse = _FlashAttnVarlenFunction.apply(
            q_in, k_in, v_in, cu_seqlens_q, cu_seqlens_k, sinks, causal,
            softmax_scale, window_size[0],
        )
        if out.shape[-1] != Dv:
            out = out[..., :Dv]
    else:
        out, lse = _eager_varlen(
            q, k, v, cu_seqlens_q.cpu(), cu_seqlens_k.cpu(), causal,
            softmax_scale, window_size, sinks,
        )
    if return_lse:
        return out, lse
    return out
