"""GPU parity tests for flash attention at MLA head dims (qk up to 192, v up
to 128: the <192, 128> kernel pair) against the fp32 eager oracle.

Tolerances are those of tests/test_attention_gpu.py for this kernel family at
these sequence lengths (S <= 512): out 3e-2, lse 1e-2, gradients 5e-2. They
carry over because scores keep unit variance at scale 1/sqrt(192) and dP still
sums over 128 columns.
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

OUT_TOL = dict(rtol=3e-2, atol=3e-2)
LSE_TOL = dict(rtol=1e-2, atol=1e-2)
GRAD_TOL = dict(rtol=5e-2, atol=5e-2)


def _qkv(B, Sq, Skv, Hq, Hkv, Dqk, Dv, grad=True):
    mk = lambda *shape: torch.randn(  # noqa: E731
        *shape, dtype=torch.bfloat16, device="cuda"
    ).requires_grad_(grad)
    return mk(B, Sq, Hq, Dqk), mk(B, Skv, Hkv, Dqk), mk(B, Skv, Hkv, Dv)


def _f32_leaves(*ts):
    return [t.detach().float().requires_grad_(True) for t in ts]


def _check_against_oracle(q, k, v, *, causal=True, scale=None,
                          window=(-1, -1), sinks=None, lse_weight=0.0,
                          first=None):
    """Forward + backward of the kernel against the fp32 oracle on the same
    bf16 inputs; loss = <out, g> + lse_weight * lse.sum(). `first()` holds a
    case's own assertions and runs before the tolerance checks."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    out, lse = flash_attn_func(
        q, k, v, causal=causal, softmax_scale=scale, window_size=window,
        sinks=sinks, return_lse=True,
    )
    assert out.shape == (*q.shape[:-1], v.shape[-1])
    g = torch.randn_like(out)
    loss = (out.float() * g.float()).sum()
    if lse_weight:
        loss = loss + lse_weight * lse.sum()
    loss.backward()

    q32, k32, v32 = _f32_leaves(q, k, v)
    s32 = sinks.detach().clone().requires_grad_(True) if sinks is not None else None
    ref, ref_lse = _eager_attention(q32, k32, v32, causal, scale, window, s32)
    ref_loss = (ref * g.float()).sum()
    if lse_weight:
        ref_loss = ref_loss + lse_weight * ref_lse.sum()
    ref_loss.backward()

    checks = [
        ("out", out.float(), ref, OUT_TOL),
        ("lse", lse, ref_lse, LSE_TOL),
        ("dq", q.grad.float(), q32.grad, GRAD_TOL),
        ("dk", k.grad.float(), k32.grad, GRAD_TOL),
        ("dv", v.grad.float(), v32.grad, GRAD_TOL),
    ]
    if sinks is not None:
        checks.append(("dsinks", sinks.grad, s32.grad, GRAD_TOL))
    _assert_all_close(checks, first)
    return out, lse


def _assert_all_close(checks, first=None):
    """Print every figure (shown with pytest -s), then assert each."""
    for name, got, want, tol in checks:
        err = (got - want).abs()
        over = (err > tol["atol"] + tol["rtol"] * want.abs()).sum().item()
        print(f"  {name}: max abs err {err.max().item():.4g} "
              f"(tol {tol['atol']:g}), {over} of {err.numel()} over")
    if first is not None:
        first()
    for name, got, want, tol in checks:
        torch.testing.assert_close(got, want, **tol, msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize(
    "B,S,Hq,Hkv,Dqk,Dv,causal",
    [
        (1, 1, 2, 2, 192, 128, True),     # single row
        (2, 33, 4, 2, 192, 128, True),    # one row past a 32-row q tile, GQA 2
        (1, 65, 4, 4, 192, 128, False),   # one row past the 64-row kv tile
        (2, 129, 8, 2, 192, 128, True),   # one row past the 128-row tiles, GQA 4
        (1, 300, 4, 1, 192, 128, True),   # several tiles, MQA
        (1, 130, 2, 2, 160, 96, True),    # host padding on both sides
        (1, 130, 2, 2, 136, 128, False),  # ... on the qk side
        (1, 96, 2, 2, 192, 64, True),     # ... on the v side
    ],
)
def test_wide_fwd_bwd_parity(B, S, Hq, Hkv, Dqk, Dv, causal):
    q, k, v = _qkv(B, S, S, Hq, Hkv, Dqk, Dv)
    _check_against_oracle(q, k, v, causal=causal)


@pytest.mark.gpu
def test_wide_peaked_softmax():
    """scale 0.5: attention is near one-hot, so a wrong k-step or fragment map
    moves the argmax and misses by O(1).

    This is the case that needs the forward's residual plane: with delta =
    rowsum(dO * O) taken from the bf16 `out` alone, one-hot rows carry delta's
    rounding error into dS un-averaged, and dq / dk miss 5e-2 + 5% at 83 of
    396288 and 29 of 99072 elements (max abs err 0.106 / 0.118; the <128, 128>
    kernels at this shape and scale: 65 of 264192 and 29 of 66048). With
    O = out + residual no element is over.
    """
    q, k, v = _qkv(2, 129, 129, 8, 2, 192, 128)
    _check_against_oracle(q, k, v, causal=True, scale=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("live", [(128, 192), (0, 128)])
def test_wide_column_block_only(live):
    """q and k are zero outside columns live[0]..live[1]: a kernel that drops
    that block of the qk dim gives uniform attention; the gradients of the
    dead columns are exactly zero."""
    lo, hi = live
    q, k, v = _qkv(1, 129, 129, 4, 2, 192, 128, grad=False)
    keep = torch.zeros(192, dtype=torch.bool, device="cuda")
    keep[lo:hi] = True
    q = (q * keep).requires_grad_(True)
    k = (k * keep).requires_grad_(True)
    v.requires_grad_(True)

    def dead_columns_are_zero():
        assert q.grad[..., lo:hi].abs().max() > 0
        assert (q.grad[..., ~keep] == 0).all()
        assert (k.grad[..., ~keep] == 0).all()

    _check_against_oracle(q, k, v, causal=True, scale=0.5,
                          first=dead_columns_are_zero)


@pytest.mark.gpu
def test_wide_host_padding_is_exact():
    import torch.nn.functional as F

    q, k, v = _qkv(1, 130, 130, 2, 2, 160, 96, grad=False)
    scale = 160 ** -0.5
    out, lse = flash_attn_func(q, k, v, softmax_scale=scale, return_lse=True)
    out_p, lse_p = flash_attn_func(
        F.pad(q, (0, 32)), F.pad(k, (0, 32)), F.pad(v, (0, 32)),
        softmax_scale=scale, return_lse=True,
    )
    assert out.shape[-1] == 96 and out_p.shape[-1] == 128
    assert torch.equal(out, out_p[..., :96])
    assert torch.equal(lse, lse_p)


@pytest.mark.gpu
def test_wide_sliding_window():
    q, k, v = _qkv(2, 200, 200, 4, 2, 192, 128)
    _check_against_oracle(q, k, v, causal=True, window=(40, -1))


@pytest.mark.gpu
def test_wide_sinks_and_dsinks():
    q, k, v = _qkv(2, 129, 129, 8, 2, 192, 128)
    sinks = torch.randn(8, dtype=torch.float32, device="cuda", requires_grad=True)
    _check_against_oracle(q, k, v, causal=True, sinks=sinks)


@pytest.mark.gpu
def test_wide_differentiable_lse():
    """loss = out.sum() + lse.sum(): dlse is folded into delta."""
    q, k, v = _qkv(2, 129, 129, 4, 2, 192, 128)
    _check_against_oracle(q, k, v, causal=True, lse_weight=1.0)


@pytest.mark.gpu
def test_wide_q_offset_matches_slice_of_full_call():
    q, k, v = _qkv(2, 192, 192, 4, 2, 192, 128, grad=False)
    full, full_lse = flash_attn_func(q, k, v, causal=True, return_lse=True)
    part, part_lse = flash_attn_func(
        q[:, 128:], k, v, causal=True, q_offset=128, return_lse=True
    )
    assert part.shape == (2, 64, 4, 128)
    torch.testing.assert_close(part.float(), full[:, 128:].float(), **OUT_TOL)
    torch.testing.assert_close(part_lse, full_lse[:, :, 128:], **LSE_TOL)
    ref, ref_lse = _eager_attention(
        q[:, 128:].float(), k.float(), v.float(), True, 192 ** -0.5, (-1, -1),
        None, q_offset=128,
    )
    torch.testing.assert_close(part.float(), ref, **OUT_TOL)
    torch.testing.assert_close(part_lse, ref_lse, **LSE_TOL)


def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)


@pytest.mark.gpu
def test_wide_varlen_documents():
    cu = _cu([1, 33, 127, 130])
    total, Hq, Hkv = int(cu[-1]), 4, 2
    q, k, v = (t.squeeze(0) for t in _qkv(1, total, total, Hq, Hkv, 192, 128, grad=False))
    for t in (q, k, v):
        t.requires_grad_(True)
    out, lse = flash_attn_varlen_func(q, k, v, cu.cuda(), causal=True, return_lse=True)
    assert out.shape == (total, Hq, 128)
    g = torch.randn_like(out)
    out.backward(g)

    q32, k32, v32 = _f32_leaves(q, k, v)
    ref, ref_lse = _eager_varlen(q32, k32, v32, cu, cu, True, 192 ** -0.5, (-1, -1), None)
    ref.backward(g.float())
    _assert_all_close([
        ("out", out.float(), ref, OUT_TOL),
        ("lse", lse, ref_lse, LSE_TOL),
        ("dq", q.grad.float(), q32.grad, GRAD_TOL),
        ("dk", k.grad.float(), k32.grad, GRAD_TOL),
        ("dv", v.grad.float(), v32.grad, GRAD_TOL),
    ])


@pytest.mark.gpu
def test_wide_varlen_cross_lengths_forward():
    """cu_seqlens_q != cu_seqlens_k: causal aligns the sequence ends."""
    cu_q, cu_k = _cu([64, 130]), _cu([200, 300])
    mk = lambda n, h, d: torch.randn(  # noqa: E731
        n, h, d, dtype=torch.bfloat16, device="cuda"
    )
    q, k, v = mk(int(cu_q[-1]), 4, 192), mk(int(cu_k[-1]), 4, 192), mk(int(cu_k[-1]), 4, 128)
    out, lse = flash_attn_varlen_func(
        q, k, v, cu_q.cuda(), cu_k.cuda(), causal=True, return_lse=True
    )
    ref, ref_lse = _eager_varlen(
        q.float(), k.float(), v.float(), cu_q, cu_k, True, 192 ** -0.5, (-1, -1), None
    )
    torch.testing.assert_close(out.float(), ref, **OUT_TOL)
    torch.testing.assert_close(lse, ref_lse, **LSE_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("Dqk,Dv", [(192, 192), (256, 128), (64, 192)])
def test_unsupported_head_dims_raise(Dqk, Dv):
    q, k, v = _qkv(1, 16, 16, 2, 2, Dqk, Dv, grad=False)
    with pytest.raises(ValueError, match="192"):
        flash_attn_func(q, k, v)
    with pytest.raises(ValueError, match="192"):
        flash_attn_varlen_func(
            q[0], k[0], v[0], torch.tensor([0, 16], dtype=torch.int32, device="cuda")
        )


# ---- module: MultiHeadLatentAttention at its default head dims (192 / 128) ----

_MLA_LENS = [33, 97]  # cu_seqlens [0, 33, 130]


def _mla_run(mla, x, cos_sin, w, cu_seqlens=None):
    """(output, {param: grad}) as fp32 CPU tensors for loss = <out, w>."""
    mla.zero_grad(set_to_none=True)
    out = mla(x, cos_sin, cu_seqlens=cu_seqlens)
    (out.float() * w.to(out.device)).sum().backward()
    grads = {n: p.grad.detach().float().cpu() for n, p in mla.named_parameters()}
    return out.detach().float().cpu(), grads


def _rel_err(a, ref):
    return ((a - ref).abs().max() / ref.abs().max()).item()


@pytest.fixture(scope="module")
def mla_setup():
    """The bf16 GPU module, its fp32 CPU copy (same weights), inputs, and the
    fp32 CPU reference results for the dense and the packed run."""
    from d9d_amd.module.block.attention import MultiHeadLatentAttention
    from d9d_amd.module.block.positional import RotaryEmbeddingProvider

    torch.manual_seed(5)
    S = sum(_MLA_LENS)
    mla = MultiHeadLatentAttention(256, 2, kv_lora_rank=64, q_lora_rank=48)
    mla.reset_parameters()
    mla = mla.bfloat16()
    ref_mla = copy.deepcopy(mla).float()
    mla = mla.cuda()
    prov = RotaryEmbeddingProvider(rope_dim=64)
    x = torch.randn(1, S, 256).bfloat16()
    w = torch.randn(1, S, 256)
    pos_dense = torch.arange(S).unsqueeze(0)
    pos_packed = torch.cat([torch.arange(n) for n in _MLA_LENS]).unsqueeze(0)

    ref_dense = _mla_run(ref_mla, x.float(), prov(pos_dense), w)
    # the packed reference: the two documents run separately
    ref_mla.zero_grad(set_to_none=True)
    outs, lo = [], 0
    for n in _MLA_LENS:
        o = ref_mla(x[:, lo : lo + n].float(), prov(torch.arange(n).unsqueeze(0)))
        (o * w[:, lo : lo + n]).sum().backward()  # grads accumulate over the documents
        outs.append(o.detach())
        lo += n
    ref_packed = (
        torch.cat(outs, dim=1),
        {n: p.grad.detach().clone() for n, p in ref_mla.named_parameters()},
    )
    to_gpu = lambda cs: tuple(t.cuda() for t in cs)  # noqa: E731
    return dict(
        mla=mla, x=x.cuda(), w=w,
        dense=(to_gpu(prov(pos_dense)), None, ref_dense),
        packed=(to_gpu(prov(pos_packed)),
                torch.tensor([0, 33, 130], dtype=torch.int32, device="cuda"), ref_packed),
    )


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["dense", "packed"])
def test_mla_default_dims_kernel_error_within_2x_of_eager(mode, mla_setup, monkeypatch):
    """Reference: the same module and weights in fp32 on the CPU (for the packed
    run, on the two documents separately). Error = max-abs difference over
    max-abs of the reference, for the output and every parameter gradient. The
    kernel path and the same GPU module with the flash op patched to the eager
    oracle are both bf16 pipelines that differ only in the attention's internal
    rounding (P rounded to bf16 before PV), so the kernel path may be at most
    2x the eager path's error."""
    import d9d_amd.module.block.attention.multi_head_latent as mod
    import d9d_amd.ops as ops

    mla, x, w = mla_setup["mla"], mla_setup["x"], mla_setup["w"]
    cos_sin, cu, (ref_out, ref_grads) = mla_setup[mode]

    out_k, grads_k = _mla_run(mla, x, cos_sin, w, cu)

    def eager_dense(q, k, v, *, causal, softmax_scale):
        assert q.shape[-1] == 192 and v.shape[-1] == 128
        return _eager_attention(q, k, v, causal, softmax_scale, (-1, -1), None)[0]

    def eager_varlen(q, k, v, cu_q, *, causal, softmax_scale):
        c = cu_q.cpu()
        return _eager_varlen(q, k, v, c, c, causal, softmax_scale, (-1, -1), None)[0]

    monkeypatch.setattr(mod, "flash_attn_func", eager_dense)
    monkeypatch.setattr(ops, "flash_attn_varlen_func", eager_varlen)
    out_e, grads_e = _mla_run(mla, x, cos_sin, w, cu)

    rows = [("output", _rel_err(out_k, ref_out), _rel_err(out_e, ref_out))]
    for n in ref_grads:
        rows.append((f"grad {n}", _rel_err(grads_k[n], ref_grads[n]),
                     _rel_err(grads_e[n], ref_grads[n])))
    for name, ek, ee in rows:
        print(f"mla {mode} {name}: kernel {ek:.3e} eager {ee:.3e}")
    for name, ek, ee in rows:
        assert math.isfinite(ek) and ek <= 2 * ee, (mode, name, ek, ee)
