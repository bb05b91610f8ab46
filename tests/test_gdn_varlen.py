"""Packed-document (cu_seqlens) GatedDeltaNet: with `cu_seqlens` given,
output rows cu[i]:cu[i+1] equal what the same code produces when fed
document i alone — zero recurrent state and no conv taps across a document
start, no gradient across a boundary.

References are always the existing dense code run one document at a time
and concatenated. Tolerances are the ones tests/test_blocks_extra.py uses
for the same quantities and the same input distribution.
"""

import os

import pytest
import torch
import torch.nn.functional as F

from d9d_amd.dataset.packing import pack_documents
from d9d_amd.module.block.attention.linear.gated_deltanet import (
    CausalShortDepthwiseConv1d,
    GatedDeltaNet,
    _chunk_gated_delta_rule_torch,
    _chunk_gdn_backward,
    chunk_gated_delta_rule,
    step_gated_delta_rule,
)

LENS = [1, 64, 63, 65, 0, 130, 7]  # T = 330: short, exact, tail, empty, multi-chunk
LENS_WIDE = [5, 64, 70, 33] * 4    # 16 documents


def _cu(lens, device="cpu"):
    cu = torch.zeros(len(lens) + 1, dtype=torch.int32)
    cu[1:] = torch.tensor(lens, dtype=torch.int32).cumsum(0)
    return cu.to(device)


def _spans(lens):
    cu = _cu(lens).tolist()
    return list(zip(cu[:-1], cu[1:]))


def _gdn_inputs(H, T, Dk, Dv, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed)
    q = F.normalize(torch.randn(1, H, T, Dk, generator=g), dim=-1)
    k = F.normalize(torch.randn(1, H, T, Dk, generator=g), dim=-1)
    v = torch.randn(1, H, T, Dv, generator=g) * 0.5
    beta = torch.rand(1, H, T, generator=g)
    dl = -torch.rand(1, H, T, generator=g) * 0.2
    return tuple(t.to(device) for t in (q, k, v, beta, dl))


def _per_doc(fn, lens, *tensors):
    """fn on each non-empty document's rows (dim 2), concatenated."""
    outs = [fn(*(t[:, :, s:e] for t in tensors)) for s, e in _spans(lens) if e > s]
    return torch.cat(outs, dim=2)


# ----------------------------------------------------------------- CPU tests


def test_chunk_torch_varlen_matches_step_oracle():
    q, k, v, beta, g = _gdn_inputs(2, sum(LENS), 32, 48)
    out = _chunk_gated_delta_rule_torch(q, k, v, beta, g, 64, _cu(LENS))
    ref = _per_doc(step_gated_delta_rule, LENS, q, k, v, beta, g)
    assert out.shape == v.shape
    torch.testing.assert_close(out, ref, rtol=1e-3, atol=1e-3)


def test_derived_backward_varlen_matches_autograd():
    q, k, v, beta, g = (
        t.requires_grad_(True) for t in _gdn_inputs(2, sum(LENS), 32, 48, seed=1)
    )
    out = _per_doc(_chunk_gated_delta_rule_torch, LENS, q, k, v, beta, g)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
    ref = torch.autograd.grad(out, (q, k, v, beta, g), dout)
    mine = _chunk_gdn_backward(
        q.detach(), k.detach(), v.detach(), beta.detach(), g.detach(), dout,
        64, _cu(LENS),
    )
    for name, a, m in zip("qkvbg", ref, mine):
        torch.testing.assert_close(
            a, m, rtol=2e-4, atol=2e-4, msg=lambda s, n=name: f"d{n}: {s}"
        )


def test_conv_eager_varlen_matches_per_document():
    lens = [1, 2, 3, 4, 9, 0, 5]  # documents shorter than K are the hard case
    T, C, K = sum(lens), 12, 4
    torch.manual_seed(3)
    conv = CausalShortDepthwiseConv1d(C, K)
    conv.reset_parameters()
    x = torch.randn(1, T, C, requires_grad=True)
    dy = torch.randn(1, T, C)

    out = conv(x, _cu(lens))
    gx, gw = torch.autograd.grad(out, (x, conv.weight), dy)

    ref = torch.cat([conv(x[:, s:e]) for s, e in _spans(lens) if e > s], dim=1)
    rx, rw = torch.autograd.grad(ref, (x, conv.weight), dy)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gx, rx, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gw, rw, rtol=1e-5, atol=1e-5)


def _small_module():
    torch.manual_seed(4)
    m = GatedDeltaNet(32, num_heads=4, num_kv_heads=2, head_k_dim=8, head_v_dim=8)
    m.reset_parameters()
    # O(1) activations, so the absolute tolerance below means something
    with torch.no_grad():
        for lin in (m.q_proj, m.k_proj, m.v_proj, m.beta_proj, m.out_gate, m.o_proj):
            torch.nn.init.normal_(lin.weight, std=0.2)
    return m


def _check_module_agreement(m, x, cu, rtol, atol):
    spans = list(zip(cu.tolist()[:-1], cu.tolist()[1:]))
    with torch.no_grad():
        packed = m(x, cu_seqlens=cu)
        alone = torch.cat([m(x[:, s:e]) for s, e in spans if e > s], dim=1)
        dense = m(x)
    torch.testing.assert_close(packed.float(), alone.float(), rtol=rtol, atol=atol)
    # the argument is not ignored: every document after the first changes
    first = True
    for s, e in spans:
        if e == s:
            continue
        if first:
            first = False
            continue
        diff = (packed[:, s:e].float() - dense[:, s:e].float()).abs().max()
        assert diff > 1e-2 * packed[:, s:e].float().abs().max(), (s, e, diff)


def test_module_varlen_matches_per_document():
    m = _small_module()
    lens = [5, 70, 3, 0, 66]
    x = torch.randn(1, sum(lens), 32)
    _check_module_agreement(m, x, _cu(lens), 1e-4, 1e-4)


def _check_isolation(m, x, cu):
    """Backward of document 2's output touches document 2's input only."""
    x = x.detach().requires_grad_(True)
    out = m(x, cu_seqlens=cu)
    s, e = int(cu[2]), int(cu[3])
    assert e > s
    out[:, s:e].float().sum().backward()
    g = x.grad.float()
    assert torch.count_nonzero(g[:, :s]) == 0
    assert torch.count_nonzero(g[:, e:]) == 0
    assert torch.count_nonzero(g[:, s:e]) > 0
    assert torch.isfinite(g).all()


def test_module_varlen_gradient_isolation():
    m = _small_module()
    lens = [5, 70, 3, 0, 66]
    _check_isolation(m, torch.randn(1, sum(lens), 32), _cu(lens))


def test_module_varlen_with_packer():
    torch.manual_seed(5)
    docs = [torch.randint(0, 50, (n,)) for n in (7, 20, 4, 30)]
    pack = next(iter(pack_documents(docs, 64)))
    cu = pack["cu_seqlens"]
    assert cu.dtype == torch.int32 and cu.numel() > 2
    emb = torch.nn.Embedding(50, 32)
    x = emb(pack["input_ids"]).detach().unsqueeze(0)
    _check_module_agreement(_small_module(), x, cu, 1e-4, 1e-4)


def test_functional_rejects_bad_packing():
    q, k, v, beta, g = _gdn_inputs(2, 20, 8, 8)
    two = tuple(torch.cat([t, t], dim=0) for t in (q, k, v, beta, g))
    with pytest.raises(ValueError):
        chunk_gated_delta_rule(*two, cu_seqlens=_cu([8, 12]))
    with pytest.raises(ValueError):
        chunk_gated_delta_rule(q, k, v, beta, g, cu_seqlens=_cu([8, 13]))
    with pytest.raises(ValueError):
        chunk_gated_delta_rule(q, k, v, beta, g, cu_seqlens=_cu([8, 11]))


# ----------------------------------------------------------------- GPU tests

GPU_CASES = [(LENS, 3), (LENS_WIDE, 13)]  # Dv-split / full-width instantiation


def _gpu_bf16_inputs(lens, H, seed):
    q, k, v, beta, g = _gdn_inputs(H, sum(lens), 64, 64, "cuda", seed)
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), beta, g


@pytest.mark.gpu
@pytest.mark.parametrize("lens,H", GPU_CASES)
def test_gdn_chunk_fwd_varlen_kernel_gpu(lens, H):
    from d9d_amd.ops._ext import get_ext

    ext = get_ext()
    q, k, v, beta, g = _gpu_bf16_inputs(lens, H, 6)
    cu = _cu(lens, "cuda")
    out, fs, r, s0 = ext.gdn_chunk_fwd_varlen(q, k, v, beta, g, cu, True, True, False)

    nchunks = [(n + 63) // 64 for n in lens]
    assert out.shape == v.shape and r.shape == (1, H, sum(lens), 64)
    assert fs.shape == (len(lens), H, 64, 64)
    assert s0.shape == (1, H, sum(nchunks), 64, 64)

    oracle = _per_doc(
        step_gated_delta_rule, lens, q.float(), k.float(), v.float(), beta, g
    )
    torch.testing.assert_close(out.float(), oracle.float(), rtol=3e-2, atol=3e-2)

    # every document starts from a zero state
    off = 0
    for n in nchunks:
        if n:
            assert torch.count_nonzero(s0[:, :, off]) == 0
        off += n
    for i, n in enumerate(lens):
        if n == 0:
            assert torch.count_nonzero(fs[i]) == 0

    split = len(lens) * H * 2 <= 384  # the kernels' Dv-split rule on nseq*H
    assert split == (lens is LENS)    # the two cases cover both instantiations
    if split:
        # varlen and a dense one-document call pick the same (Dv-split)
        # instantiation: same arithmetic in the same order, so bit-equal
        for i, (s, e) in enumerate(_spans(lens)):
            if e == s:
                continue
            d_out, d_fs = ext.gdn_chunk_fwd(
                q[:, :, s:e], k[:, :, s:e], v[:, :, s:e],
                beta[:, :, s:e], g[:, :, s:e], True, False, False,
            )
            assert torch.equal(out[:, :, s:e], d_out), i
            assert torch.equal(fs[i], d_fs[0]), i


@pytest.mark.gpu
@pytest.mark.parametrize("lens,H", GPU_CASES)
def test_gdn_varlen_backward_kernel_scan_gpu(lens, H):
    q, k, v, beta, g = (t.float() for t in _gpu_bf16_inputs(lens, H, 7))
    do = torch.randn(
        v.shape, generator=torch.Generator().manual_seed(8)
    ).cuda()

    prev = os.environ.get("D9D_GDN_BWD_SCAN")
    os.environ["D9D_GDN_BWD_SCAN"] = "0"
    try:
        ref = [
            torch.cat(parts, dim=2)
            for parts in zip(*(
                _chunk_gdn_backward(
                    q[:, :, s:e], k[:, :, s:e], v[:, :, s:e],
                    beta[:, :, s:e], g[:, :, s:e], do[:, :, s:e],
                )
                for s, e in _spans(lens) if e > s
            ))
        ]
        os.environ["D9D_GDN_BWD_SCAN"] = "1"
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v, beta, g)]
        out = chunk_gated_delta_rule(*leaves, cu_seqlens=_cu(lens, "cuda"))
        mine = torch.autograd.grad(out, leaves, do)
    finally:
        if prev is None:
            os.environ.pop("D9D_GDN_BWD_SCAN", None)
        else:
            os.environ["D9D_GDN_BWD_SCAN"] = prev
    for name, a, b in zip("qkvbg", ref, mine):
        torch.testing.assert_close(
            a.float(), b.float(), rtol=2e-2, atol=2e-2,
            msg=lambda s, n=name: f"d{n}: {s}",
        )


@pytest.mark.gpu
def test_causal_conv_silu_varlen_kernel_gpu():
    from d9d_amd.ops._ext import get_ext

    ext = get_ext()
    lens = [1, 2, 3, 4, 37, 0, 5]
    T, C, K = sum(lens), 48, 4
    torch.manual_seed(9)
    x = torch.randn(1, T, C, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(C, K, device="cuda", dtype=torch.bfloat16)
    dy = torch.randn(1, T, C, device="cuda", dtype=torch.bfloat16)
    cu = _cu(lens, "cuda")
    spans = [(s, e) for s, e in _spans(lens) if e > s]

    out = ext.causal_conv_silu_varlen_fwd(x, w, cu)
    dx, dw = ext.causal_conv_silu_varlen_bwd(x, w, dy, cu)

    # per-document dense kernel calls: same taps in the same order
    d_out = torch.cat([ext.causal_conv_silu_fwd(x[:, s:e], w) for s, e in spans], 1)
    d_bwd = [ext.causal_conv_silu_bwd(x[:, s:e], w, dy[:, s:e]) for s, e in spans]
    assert torch.equal(out, d_out)
    assert torch.equal(dx, torch.cat([b[0] for b in d_bwd], 1))
    d_dw = sum(b[1].float() for b in d_bwd)
    torch.testing.assert_close(dw.float(), d_dw, rtol=3e-2, atol=2e-1)

    # eager fp32 chain, one document at a time
    x32 = x.float().requires_grad_(True)
    w32 = w.float().requires_grad_(True)
    ref = torch.cat([
        F.silu(F.conv1d(
            F.pad(x32[:, s:e].transpose(1, 2), (K - 1, 0)),
            w32.unsqueeze(1), groups=C,
        ).transpose(1, 2))
        for s, e in spans
    ], dim=1)
    ref.backward(dy.float())
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(dx.float(), x32.grad, rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(dw.float(), w32.grad, rtol=3e-2, atol=2e-1)


@pytest.mark.gpu
def test_gdn_module_varlen_kernel_path_gpu():
    torch.manual_seed(11)
    m = GatedDeltaNet(128, num_heads=2, head_k_dim=64, head_v_dim=64).cuda().bfloat16()
    m.reset_parameters()
    lens = [40, 64, 100]
    cu = _cu(lens, "cuda")
    x = torch.randn(1, sum(lens), 128, device="cuda", dtype=torch.bfloat16)
    _check_module_agreement(m, x, cu.cpu(), 3e-2, 3e-2)
    _check_isolation(m, x, cu)
    for n, p in m.named_parameters():
        assert p.grad is None or torch.isfinite(p.grad.float()).all(), n
    assert m.q_conv.weight.grad is not None


@pytest.mark.gpu
def test_varlen_kernels_reject_bad_cu_seqlens_on_host_gpu():
    """Only the host check runs: each call must raise before any launch."""
    from d9d_amd.ops._ext import get_ext

    ext = get_ext()
    lens = [10, 20, 6]
    T = sum(lens)
    q, k, v, beta, g = _gpu_bf16_inputs(lens, 2, 12)
    x = torch.randn(1, T, 16, device="cuda", dtype=torch.bfloat16)
    w = torch.randn(16, 4, device="cuda", dtype=torch.bfloat16)

    too_long = _cu(lens, "cuda")
    too_long[-1] = T + 1
    decreasing = torch.tensor([0, 20, 10, T], dtype=torch.int32, device="cuda")
    for bad in (too_long, decreasing):
        with pytest.raises(RuntimeError, match="cu_seqlens"):
            ext.gdn_chunk_fwd_varlen(q, k, v, beta, g, bad, False, False, False)
        with pytest.raises(RuntimeError, match="cu_seqlens"):
            ext.gdn_chunk_bwd_scan_varlen(q, k, v, beta, g, bad)
        with pytest.raises(RuntimeError, match="cu_seqlens"):
            ext.causal_conv_silu_varlen_fwd(x, w, bad)
        with pytest.raises(RuntimeError, match="cu_seqlens"):
            ext.causal_conv_silu_varlen_bwd(x, w, x, bad)
    with pytest.raises(RuntimeError, match="int32"):
        ext.gdn_chunk_fwd_varlen(
            q, k, v, beta, g, _cu(lens, "cuda").long(), False, False, False
        )
