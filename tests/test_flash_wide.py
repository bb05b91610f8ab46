"""CPU tests for the wide head-dim support: the op's head-dim routing and
MultiHeadLatentAttention's packed-document (cu_seqlens) path."""

import pytest
import torch

from d9d_amd.ops.attention import head_dim_route


@pytest.mark.parametrize(
    "dims,route",
    [
        ((24, 16), "legacy pad"),
        ((128, 64), "legacy pad"),
        ((64, 128), "legacy pad"),
        ((128, 128), "legacy pad"),
        ((192, 128), "wide"),
        ((136, 96), "wide"),
        ((129, 1), "wide"),
    ],
)
def test_head_dim_route(dims, route):
    assert head_dim_route(*dims) == route


@pytest.mark.parametrize("dims", [(192, 192), (256, 128), (64, 192), (193, 128), (192, 129)])
def test_head_dim_route_rejects_unsupported(dims):
    with pytest.raises(ValueError, match="192.*128"):
        head_dim_route(*dims)


def test_cpu_oracle_takes_any_head_dims():
    """The limits are the GPU kernels'; the eager CPU path has none."""
    from d9d_amd.ops import flash_attn_func

    q = torch.randn(1, 5, 2, 200)
    out = flash_attn_func(q, torch.randn(1, 5, 2, 200), torch.randn(1, 5, 2, 136))
    assert out.shape == (1, 5, 2, 136)


@pytest.mark.parametrize("dims", [(16, 8, 16), (40, 8, 24)])  # qk 24 / v 16; qk 48 / v 24
def test_mla_packed_documents_match_per_doc(dims):
    """cu_seqlens path == running each document separately."""
    from d9d_amd.module.block.attention import MultiHeadLatentAttention
    from d9d_amd.module.block.positional import RotaryEmbeddingProvider

    nope, rope, vdim = dims
    torch.manual_seed(9)
    mla = MultiHeadLatentAttention(
        64, 4, qk_nope_head_dim=nope, qk_rope_head_dim=rope, v_head_dim=vdim,
        kv_lora_rank=32, q_lora_rank=24,
    )
    mla.reset_parameters()
    prov = RotaryEmbeddingProvider(rope_dim=rope)
    lens = [5, 9, 3]
    cu = torch.tensor([0, 5, 14, 17], dtype=torch.int32)
    xs = [torch.randn(1, n, 64) for n in lens]
    packed = torch.cat(xs, dim=1).requires_grad_(True)

    # rotary positions restart per document
    pos = torch.cat([torch.arange(n) for n in lens]).unsqueeze(0)
    out_packed = mla(packed, prov(pos), cu_seqlens=cu)
    outs = [mla(x, prov(torch.arange(x.shape[1]).unsqueeze(0))) for x in xs]
    torch.testing.assert_close(out_packed, torch.cat(outs, dim=1), rtol=1e-5, atol=1e-6)

    # a later document's input does not reach an earlier document's output
    out_packed[:, :5].sum().backward()
    assert packed.grad[:, :5].abs().max() > 0
    assert (packed.grad[:, 5:] == 0).all()

    with pytest.raises(AssertionError, match="batch dim 1"):
        mla(torch.randn(2, 17, 64), prov(pos), cu_seqlens=cu)
