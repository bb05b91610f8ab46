"""GPU parity tests for flash attention at head dims 193..256 (the <256, 256>
kernels) against the fp32 eager oracle on fp32 leaves of the same bf16 inputs.

Tolerances are the family's (tests/test_flash_wide_gpu.py): out 3e-2, lse 1e-2,
gradients 5e-2 + 5%. They carry over: at scale 1/sqrt(256) the scores keep unit
variance, P rows sum to one so the out error does not grow with Dv, and dP's
sqrt(2) growth moves gradient magnitude and error together.
"""

import copy
import math

import pytest
import torch

from d9d_amd.ops.attention import (
    _eager_attention,
    _eager_varlen,
    flash_attn_func,
    flash_attn_varlen_func,
)
from tests.test_flash_wide_gpu import (
    GRAD_TOL,
    LSE_TOL,
    OUT_TOL,
    _assert_all_close,
    _check_against_oracle,
    _cu,
    _f32_leaves,
    _qkv,
    _rel_err,
)


@pytest.mark.gpu
@pytest.mark.parametrize(
    "B,S,Hq,Hkv,Dqk,Dv,causal,scale",
    [
        (1, 1, 2, 2, 256, 256, True, None),     # single row
        (2, 33, 4, 2, 256, 256, True, None),    # one row past the 32-row q tile, GQA 2
        (1, 65, 4, 4, 256, 256, False, None),   # one row past the 64-row kv tiles
        (2, 129, 8, 2, 256, 256, True, None),   # one row past the forward's 128 q rows
        (1, 300, 4, 1, 256, 256, True, None),   # several tiles, MQA
        (1, 130, 2, 2, 224, 200, True, None),   # host padding on both sides
        # peaked softmax: a wrong k-step or fragment map moves the argmax; needs
        # the forward's residual plane for delta
        (2, 129, 8, 2, 256, 256, True, 0.5),
    ],
)
def test_256_fwd_bwd_parity(B, S, Hq, Hkv, Dqk, Dv, causal, scale):
    q, k, v = _qkv(B, S, S, Hq, Hkv, Dqk, Dv)
    _check_against_oracle(q, k, v, causal=causal, scale=scale)


@pytest.mark.gpu
@pytest.mark.parametrize("live", [(0, 128), (128, 256)])
def test_256_column_block_only(live):
    """q, k, v and dO are zero outside columns live[0]..live[1] (scale 0.5):
    the dead columns' gradients are exactly zero and the live ones are not.
    The backward splits the head dim between waves at column 128."""
    lo, hi = live
    keep = torch.zeros(256, dtype=torch.bool, device="cuda")
    keep[lo:hi] = True
    q, k, v = ((t * keep).requires_grad_(True)
               for t in _qkv(1, 129, 129, 4, 2, 256, 256, grad=False))
    out, lse = flash_attn_func(q, k, v, causal=True, softmax_scale=0.5, return_lse=True)
    g = torch.randn_like(out) * keep
    out.backward(g)
    q32, k32, v32 = _f32_leaves(q, k, v)
    ref, ref_lse = _eager_attention(q32, k32, v32, True, 0.5, (-1, -1), None)
    ref.backward(g.float())

    def dead_columns_are_zero():
        for t in (q, k, v):
            assert t.grad[..., lo:hi].abs().max() > 0
            assert (t.grad[..., ~keep] == 0).all()

    _assert_all_close([
        ("out", out.float(), ref, OUT_TOL),
        ("lse", lse, ref_lse, LSE_TOL),
        ("dq", q.grad.float(), q32.grad, GRAD_TOL),
        ("dk", k.grad.float(), k32.grad, GRAD_TOL),
        ("dv", v.grad.float(), v32.grad, GRAD_TOL),
    ], dead_columns_are_zero)


@pytest.mark.gpu
@pytest.mark.parametrize("feature", ["window", "sinks", "lse", "q_offset"])
def test_256_features(feature):
    if feature == "window":
        _check_against_oracle(*_qkv(2, 200, 200, 4, 2, 256, 256), window=(40, -1))
    elif feature == "sinks":
        sinks = torch.randn(8, dtype=torch.float32, device="cuda", requires_grad=True)
        _check_against_oracle(*_qkv(2, 129, 129, 8, 2, 256, 256), sinks=sinks)
    elif feature == "lse":
        _check_against_oracle(*_qkv(2, 129, 129, 4, 2, 256, 256), lse_weight=1.0)
    else:
        q, k, v = _qkv(2, 192, 192, 4, 2, 256, 256, grad=False)
        full, full_lse = flash_attn_func(q, k, v, causal=True, return_lse=True)
        part, part_lse = flash_attn_func(
            q[:, 128:], k, v, causal=True, q_offset=128, return_lse=True
        )
        ref, ref_lse = _eager_attention(
            q[:, 128:].float(), k.float(), v.float(), True, 256 ** -0.5, (-1, -1),
            None, q_offset=128,
        )
        for want, want_lse in [(full[:, 128:].float(), full_lse[:, :, 128:]), (ref, ref_lse)]:
            torch.testing.assert_close(part.float(), want, **OUT_TOL)
            torch.testing.assert_close(part_lse, want_lse, **LSE_TOL)


@pytest.mark.gpu
def test_256_varlen_documents():
    cu = _cu([1, 33, 127, 130])
    total = int(cu[-1])
    q, k, v = (t.squeeze(0).requires_grad_(True)
               for t in _qkv(1, total, total, 4, 2, 256, 256, grad=False))
    out, lse = flash_attn_varlen_func(q, k, v, cu.cuda(), causal=True, return_lse=True)
    g = torch.randn_like(out)
    out.backward(g)
    q32, k32, v32 = _f32_leaves(q, k, v)
    ref, ref_lse = _eager_varlen(q32, k32, v32, cu, cu, True, 256 ** -0.5, (-1, -1), None)
    ref.backward(g.float())
    _assert_all_close([
        ("out", out.float(), ref, OUT_TOL),
        ("lse", lse, ref_lse, LSE_TOL),
        ("dq", q.grad.float(), q32.grad, GRAD_TOL),
        ("dk", k.grad.float(), k32.grad, GRAD_TOL),
        ("dv", v.grad.float(), v32.grad, GRAD_TOL),
    ])


@pytest.mark.gpu
def test_256_varlen_cross_lengths_forward():
    """cu_seqlens_q != cu_seqlens_k: causal aligns the sequence ends."""
    cu_q, cu_k = _cu([64, 130]), _cu([200, 300])
    mk = lambda n: torch.randn(n, 4, 256, dtype=torch.bfloat16, device="cuda")  # noqa: E731
    q, k, v = mk(int(cu_q[-1])), mk(int(cu_k[-1])), mk(int(cu_k[-1]))
    out, lse = flash_attn_varlen_func(
        q, k, v, cu_q.cuda(), cu_k.cuda(), causal=True, return_lse=True
    )
    ref, ref_lse = _eager_varlen(
        q.float(), k.float(), v.float(), cu_q, cu_k, True, 256 ** -0.5, (-1, -1), None
    )
    torch.testing.assert_close(out.float(), ref, **OUT_TOL)
    torch.testing.assert_close(lse, ref_lse, **LSE_TOL)


@pytest.mark.gpu
def test_256_merged_lse_backward():
    """The ring contract of docs/kernels.md: flash_attn_bwd once per kv chunk
    with the lse and out merged over both chunks (not from its own forward).
    The summed dq and the per-chunk dk, dv match the oracle on the whole kv."""
    from d9d_amd.ops._ext import get_ext

    q, k, v = _qkv(1, 130, 130, 2, 2, 256, 256, grad=False)
    q32, k32, v32 = _f32_leaves(q, k, v)
    scale = 256 ** -0.5
    ref, ref_lse = _eager_attention(q32, k32, v32, False, scale, (-1, -1), None)
    g = torch.randn_like(q)
    ref.backward(g.float())
    out, lse = ref.detach().bfloat16(), ref_lse.detach().contiguous()
    dq, dks, dvs = 0, [], []
    for sl in (slice(0, 70), slice(70, 130)):
        dq_c, dk_c, dv_c = get_ext().flash_attn_bwd(
            g, q, k[:, sl].contiguous(), v[:, sl].contiguous(), out, lse,
            None, None, False, scale, -1, 0, None, None,
        )
        dq = dq + dq_c.float()
        dks.append(dk_c.float())
        dvs.append(dv_c.float())
    _assert_all_close([
        ("dq", dq, q32.grad, GRAD_TOL),
        ("dk", torch.cat(dks, dim=1), k32.grad, GRAD_TOL),
        ("dv", torch.cat(dvs, dim=1), v32.grad, GRAD_TOL),
    ])


# ---- module: GroupedQueryAttention at head dim 256, partial rotary, gate ----


def _gqa_run(gqa, x, cos_sin, w, cu):
    """(output, {param: grad}) as fp32 CPU tensors for loss = <out, w>."""
    gqa.zero_grad(set_to_none=True)
    out = gqa(x, cos_sin, cu_seqlens=cu)
    (out.float() * w.to(out.device)).sum().backward()
    grads = {n: p.grad.detach().float().cpu() for n, p in gqa.named_parameters()}
    return out.detach().float().cpu(), grads


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dense", "packed"])
def test_gqa_head_dim_256_kernel_error_within_2x_of_eager(mode, monkeypatch):
    """Reference: the same module and weights in fp32 on the CPU. Error =
    max-abs difference over max-abs of the reference, for the output and every
    parameter gradient. The kernel path may be at most 2x the error of the same
    GPU module with the flash op patched to the eager oracle (the bound of
    profiles/flash_wide.md)."""
    import d9d_amd.module.block.attention.grouped_query as mod
    import d9d_amd.ops as ops
    from d9d_amd.module.block.positional import RotaryEmbeddingProvider

    torch.manual_seed(5)
    S = 130
    gqa = mod.GroupedQueryAttention(256, 2, 1, head_dim=256, rope_dim=64,
                                    use_output_gate=True, use_qk_norm=True)
    gqa.reset_parameters()
    gqa = gqa.bfloat16()
    ref_gqa = copy.deepcopy(gqa).float()
    gqa = gqa.cuda()
    x, w = torch.randn(1, S, 256).bfloat16(), torch.randn(1, S, 256)
    packed = mode == "packed"
    cu = torch.tensor([0, 33, 130], dtype=torch.int32) if packed else None
    pos = torch.cat([torch.arange(33), torch.arange(97)]) if packed else torch.arange(S)
    cos_sin = RotaryEmbeddingProvider(rope_dim=64)(pos.unsqueeze(0))
    cos_sin_gpu = tuple(t.cuda() for t in cos_sin)
    cu_gpu = cu.cuda() if packed else None

    ref_out, ref_grads = _gqa_run(ref_gqa, x.float(), cos_sin, w, cu)
    out_k, grads_k = _gqa_run(gqa, x.cuda(), cos_sin_gpu, w, cu_gpu)

    def eager_dense(q, k, v, *, causal, window_size, sinks, q_offset):
        assert q.shape[-1] == 256 and v.shape[-1] == 256
        return _eager_attention(q, k, v, causal, 1 / 16, window_size, sinks, q_offset)[0]

    def eager_varlen(q, k, v, cu_q, *, causal, window_size, sinks):
        c = cu_q.cpu()
        return _eager_varlen(q, k, v, c, c, causal, 1 / 16, window_size, sinks)[0]

    monkeypatch.setattr(mod, "flash_attn_func", eager_dense)
    monkeypatch.setattr(ops, "flash_attn_varlen_func", eager_varlen)
    out_e, grads_e = _gqa_run(gqa, x.cuda(), cos_sin_gpu, w, cu_gpu)

    rows = [("output", _rel_err(out_k, ref_out), _rel_err(out_e, ref_out))]
    for n in ref_grads:
        rows.append((f"grad {n}", _rel_err(grads_k[n], ref_grads[n]),
                     _rel_err(grads_e[n], ref_grads[n])))
    for name, ek, ee in rows:
        print(f"gqa256 {mode} {name}: kernel {ek:.3e} eager {ee:.3e}")
    for name, ek, ee in rows:
        assert math.isfinite(ek) and ek <= 2 * ee, (mode, name, ek, ee)
