"""Ring attention on the HIP kernels (MI355X): d9d_amd/parallel/context.py
calls flash_attn_fwd / flash_attn_bwd directly, and the backward under a
contract no other caller uses: `lse` is the LSE merged over all chunks and
`out` the final merged output, so P = exp(S - lse) has row sums well below 1
and delta = rowsum(dout * out_final); off-diagonal blocks run non-causal with
Sq == Skv. The cases (kernel_refs.ring_case) put dominant keys into every
chunk a rank attends to; tests/test_kernel_edges.py holds the same cases, the
plant conditions and the mutants on the CPU.

The ring runs as W threads of this process (kernel_refs.virtual_ring): only
the rank queries and the P2P exchange are replaced. Every test here runs with
the eager branch of _block_fwd / _block_bwd made to raise.

Branch -> test:
  _block_fwd / _block_bwd kernel branch per (rank, chunk), diagonal causal and
    off-diagonal non-causal, S_local 65 / 128 / 130 (forward tile 128 x 64,
    backward 128 kv x 64 q), foreign lse and out .......... test_ring_blocks[*-64]
  the same at the <128, 128> instantiation ................ test_ring_blocks[*-128]
  D = 80: maybe_pad_d to 96 and the unfused cast at the
    end of flash_attn_bwd .................................. test_ring_blocks[*-80]
  _RingAttention forward + backward on the kernels: skip
    rule, online merge, fp32 dK/dV rotation, W = 2, 3, 4,
    exact 64 tile, single-row chunks, B = 2 at D = 128 .... test_virtual_ring
  non-causal ring, every rank x every chunk ................ test_virtual_ring_noncausal
  same bits from the forward twice, gradients (fp32
    atomics) within the tolerance of each other ............ test_ring_block_repeatable
  host argument checks of both entry points ................ test_flash_entry_points_reject_bad_arguments

Tolerances are the project's (TOL_ATTN_OUT, TOL_ATTN_LSE, TOL_ATTN_GRAD,
TOL_ATTN_DQ). What the kernels needed on an MI355X (kernel_refs.tol_needed:
rtol = atol = x), largest over the cases of each test:
                     out      lse      dq      dk      dv
  test_ring_blocks   3.1e-3   2.0e-7   0.045   0.036   0.0068   (max |ref| 4.5, 24, 10, 5.9, 7.0)
  test_virtual_ring  4.9e-3   2.0e-7   0.058   0.029   0.015    (max |ref| 4.5, 23, 12, 3.8, 9.2)
test_virtual_ring includes the non-causal case. The eager branch on the CPU,
fed the same bf16 tensors, needs 0.058 for dq on ring_case(4, 64, ...) as
well: that figure is the bf16 rounding of the W per-block dq partials, not the
kernel. All of them are inside the project's tolerances, so none is widened.
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from d9d_amd.ops._ext import get_ext

    return get_ext()


@pytest.fixture(autouse=True)
def no_eager_branch(monkeypatch):
    """The eager branch of _block_fwd / _block_bwd raises: a test that passes
    here ran the kernels."""
    from d9d_amd.ops import attention
    from d9d_amd.parallel import context

    real = context._use_kernel

    def kernel_or_raise(q):
        if not real(q):
            raise AssertionError("a ring block went to the eager branch")
        return True

    def refuse(*args, **kwargs):
        raise AssertionError("a ring block went to eager attention")

    monkeypatch.setattr(context, "_use_kernel", kernel_or_raise)
    monkeypatch.setattr(attention, "_eager_attention", refuse)


_CASES = {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = kr.ring_case(*shape)
    return _CASES[shape]


@pytest.mark.parametrize("shape", kr.RING_BLOCK_SHAPES, ids=lambda s: f"S{s[1]}-{s[5]}")
def test_ring_blocks(shape):
    """Every (rank, chunk) block of a W = 3 ring on the kernels, fed the fp64
    full-sequence lse (as fp32) and out (as bf16)."""
    from d9d_amd.parallel import context

    case = _case(shape)
    for r, j in kr.ring_blocks(case):
        kr.check_ring_block(context._block_fwd, context._block_bwd, case, r, j, DEV)


@pytest.mark.parametrize("shape", kr.RING_SHAPES, ids=lambda s: f"W{s[0]}-S{s[1]}-B{s[2]}-{s[5]}")
def test_virtual_ring(shape, monkeypatch):
    kr.check_ring(lambda case: kr.virtual_ring(monkeypatch, case, DEV), _case(shape))


def test_virtual_ring_noncausal(monkeypatch):
    case = kr.ring_noncausal_case(*kr.RING_NONCAUSAL)
    kr.check_ring(lambda c: kr.virtual_ring(monkeypatch, c, DEV), case)


def test_ring_block_repeatable():
    """The forward has no atomics: the same bits twice. dq, dk and dv are
    accumulated with fp32 atomics in an order that varies, so two runs agree
    within the tolerance only."""
    from d9d_amd.parallel import context

    case = _case(kr.RING_BLOCK_SHAPES[2])
    for r, j in ((2, 0), (2, 2)):
        x = kr.ring_block_inputs(case, r, j, DEV)
        fwd = lambda: context._block_fwd(x["q"], x["k"], x["v"], x["causal_block"], x["scale"])
        bwd = lambda: context._block_bwd(x["q"], x["k"], x["v"], x["out"], x["dout"],
                                         x["lse"], x["causal_block"], x["scale"])
        for a, b, n in zip(fwd(), fwd(), ("out", "lse")):
            kr.assert_bitwise(a, b, f"block ({r},{j}) {n} twice")
        tols = (kr.TOL_ATTN_DQ, kr.TOL_ATTN_GRAD, kr.TOL_ATTN_GRAD)
        for a, b, n, tol in zip(bwd(), bwd(), ("dq", "dk", "dv"), tols):
            kr.assert_close(a, b.double(), tol, f"block ({r},{j}) {n} twice")


def test_flash_entry_points_reject_bad_arguments():
    """Operands of the wrong device, dtype, rank or shape, an lse that is not
    the contiguous fp32 (B, Hq, Sq) the kernel indexes, and cu_seqlens that
    do not describe the packed tensors raise before anything is launched."""
    ext = _ext()
    B, S, Hq, Hkv, D = 1, 8, 4, 2, 64
    bf = dict(device=DEV, dtype=torch.bfloat16)
    q = torch.randn(B, S, Hq, D, **bf)
    k = torch.randn(B, S, Hkv, D, **bf)
    v = torch.randn(B, S, Hkv, D, **bf)
    sinks = torch.zeros(Hq, device=DEV)
    scale = D ** -0.5
    cu = torch.tensor([0, 3, 8], dtype=torch.int32, device=DEV)

    def fwd(q=q, k=k, v=v, sinks=None, cu_q=None, cu_k=None):
        return ext.flash_attn_fwd(q, k, v, sinks, cu_q, cu_k, True, scale, -1, 0)

    def fwd_varlen(cu_q, cu_k, q=q[0], k=k[0], v=v[0]):
        return fwd(q, k, v, None, cu_q, cu_k)

    def cu_of(*vals):
        return torch.tensor(vals, dtype=torch.int32, device=DEV)

    bad_cu = [
        (cu.view(1, 3), cu),                    # not 1-D
        (cu, cu.view(3, 1)),
        (cu_of(1, 3, 8), cu),                   # does not start at 0
        (cu_of(0, 5, 3, 8), cu_of(0, 3, 5, 8)),  # decreases
        (cu, cu_of(0, 8)),                      # lengths differ
        (cu_of(0, 3, 7), cu),                   # last entry is not the total
        (cu, cu_of(0, 3, 9)),
        (cu.float(), cu),                       # not integers
        (cu, None),
    ]
    bad_fwd = [
        lambda: fwd(q=q.cpu()),
        lambda: fwd(k=k.cpu()),
        lambda: fwd(q=q.float()),
        lambda: fwd(k=k.float()),
        lambda: fwd(v=v.half()),
        lambda: fwd(q=q[0]),                                    # rank 3 without cu_seqlens
        lambda: fwd(k=k[0]),
        lambda: fwd(v=v[None]),
        lambda: fwd(cu_q=cu, cu_k=cu),                          # rank 4 with cu_seqlens
        lambda: fwd(k=k[:, :, :1].expand(B, S, 3, D), v=v[:, :, :1].expand(B, S, 3, D)),
        lambda: fwd(k=k[..., :32]),                             # k narrower than q
        lambda: fwd(v=v[:, :7]),                                # v shorter than k
        lambda: fwd(v=v[:, :, :1]),                             # v with fewer heads
        lambda: fwd(k=k.expand(2, S, Hkv, D), v=v.expand(2, S, Hkv, D)),
        lambda: fwd(sinks=sinks[:3]),
        lambda: fwd(sinks=sinks.cpu()),
    ] + [lambda a=a, b=b: fwd_varlen(a, b) for a, b in bad_cu]
    for i, call in enumerate(bad_fwd):
        with pytest.raises(RuntimeError, match="flash_attn_fwd"):
            call()
            pytest.fail(f"flash_attn_fwd: bad call {i} was accepted")

    out, lse = fwd()[:2]
    dout = torch.randn_like(out)

    def bwd(dout=dout, q=q, k=k, v=v, out=out, lse=lse, cu_q=None, cu_k=None, dlse=None,
            out_lo=None):
        return ext.flash_attn_bwd(dout, q, k, v, out, lse, cu_q, cu_k, True, scale, -1, 0,
                                  dlse, out_lo)

    out_v, lse_v = fwd_varlen(cu, cu)[:2]
    assert lse_v.shape == (Hq, S)

    def bwd_varlen(cu_q, cu_k, lse=lse_v):
        return bwd(dout[0], q[0], k[0], v[0], out_v, lse, cu_q, cu_k)

    lse_strided = lse.transpose(1, 2).contiguous().transpose(1, 2)
    assert lse_strided.shape == lse.shape and not lse_strided.is_contiguous()
    bad_bwd = [
        lambda: bwd(dout=dout.cpu()),
        lambda: bwd(out=out.cpu()),
        lambda: bwd(q=q.cpu()),
        lambda: bwd(dout=dout.float()),
        lambda: bwd(out=out.float()),
        lambda: bwd(q=q.float()),
        lambda: bwd(k=k.float()),
        lambda: bwd(v=v.float()),
        lambda: bwd(dout=dout[0]),                              # wrong ranks
        lambda: bwd(out=out[0]),
        lambda: bwd(q=q[0]),
        lambda: bwd(k=k[None]),
        lambda: bwd(cu_q=cu, cu_k=cu),
        lambda: bwd(k=k[:, :, :1].expand(B, S, 3, D), v=v[:, :, :1].expand(B, S, 3, D)),
        lambda: bwd(k=k[..., :32]),
        lambda: bwd(v=v[:, :7]),
        lambda: bwd(out=out[..., :32]),                         # not v's head dim
        lambda: bwd(dout=dout[..., :32]),
        lambda: bwd(out=out[:, :7]),                            # not q's rows
        lambda: bwd(dout=dout[:, :, :2]),                       # not q's heads
        lambda: bwd(lse=lse.double()),
        lambda: bwd(lse=lse.bfloat16()),
        lambda: bwd(lse=lse.cpu()),
        lambda: bwd(lse=lse_strided),
        lambda: bwd(lse=lse[0]),
        lambda: bwd(lse=lse.transpose(1, 2).contiguous()),      # (B, Sq, Hq)
        lambda: bwd(lse=lse[:, :, :7].contiguous()),
        lambda: bwd(lse=lse[:, :2].contiguous()),
        lambda: bwd(dlse=lse[:, :, :7].contiguous()),
        lambda: bwd(dlse=lse.cpu()),
        lambda: bwd(out_lo=out[:, :7]),
        lambda: bwd(out_lo=out.float()),
        lambda: bwd_varlen(cu, cu, lse=lse_v.t().contiguous()),  # (total, Hq)
        lambda: bwd_varlen(cu, cu, lse=lse_v[None]),
    ] + [lambda a=a, b=b: bwd_varlen(a, b) for a, b in bad_cu]
    for i, call in enumerate(bad_bwd):
        with pytest.raises(RuntimeError, match="flash_attn_bwd"):
            call()
            pytest.fail(f"flash_attn_bwd: bad call {i} was accepted")

    # what the callers pass stays legal: int64 cu_seqlens on either device,
    # bf16 sinks, strided q/k/v/out/dout
    kr.assert_bitwise(fwd_varlen(cu.long().cpu(), cu)[0], out_v, "int64 host cu_seqlens")
    kr.assert_bitwise(fwd(sinks=sinks.bfloat16())[1], fwd(sinks=sinks)[1], "bf16 sinks")
    q_strided = q.transpose(1, 2).contiguous().transpose(1, 2)
    kr.assert_bitwise(fwd(q=q_strided)[0], out, "strided q")
    for g in bwd(q=q_strided) + bwd_varlen(cu, cu):
        assert bool(torch.isfinite(g.float()).all())
