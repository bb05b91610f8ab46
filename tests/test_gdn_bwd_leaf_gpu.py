"""gdn_chunk_bwd_leaf (csrc/gdn.hip): the per-chunk leaf gradients of the
GatedDeltaNet backward against `_gdn_leaf_grads_torch`, the torch stage the
kernel replaces, evaluated in fp64 on the CPU on the very tensors the kernel
reads (bf16 q, k, v, dout; fp32 r, s0 of gdn_chunk_fwd and drhs, ds0 of
gdn_chunk_bwd_scan).

Tolerance per output, |got - ref| <= atol + rtol |ref|:
    rtol = 2 * need,  atol = 2 * need + 2^-16 * max |ref|
`need` is what the fp32 torch stage on the GPU needs against the same fp64
evaluation (kr.tol_needed, largest over LEAF_SHAPES); the factor 2 is
kernel_refs' allowance for accumulation order, the last term one unit of the
kernel's bf16 hi/lo operand split at the output's largest magnitude.
"""

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda"
# one chunk (S0 = 0 and dS1 = 0: in-chunk terms only); two chunks (a real S0
# in chunk 1, a real dS1 in chunk 0); a middle chunk that has both
LEAF_SHAPES = [(1, 2, 64), (2, 3, 128), (1, 2, 192)]
# tol_needed against the fp64 stage, largest over LEAF_SHAPES (max |ref|: dq 5.5,
# dk 9.4, dv 3.9, dbeta 21, dg 3.0):
#   fp32 torch stage : dq 4.294e-6  dk 5.001e-6  dv 2.862e-8  dbeta 8.148e-6  dg 8.737e-6
#   kernel           : dq 2.761e-5  dk 3.286e-5  dv 2.862e-8  dbeta 5.093e-5  dg 3.556e-5
#   kernel, max abs error as a share of atol: 0.3 (dbeta) to 0.7 (dg)
LEAF_NEED = dict(dq=4.294e-6, dk=5.001e-6, dv=2.862e-8, dbeta=8.148e-6, dg=8.737e-6)


def _ext():
    from d9d_amd.ops._ext import get_ext

    return get_ext()


def _tol(name, ref):
    need = 2.0 * LEAF_NEED[name]
    return dict(rtol=need, atol=need + 2.0 ** -16 * float(ref.abs().max()))


def _leaf_args(case):
    """The ten tensors the op hands the leaf kernel, made the way it makes
    them; packed documents when the case carries `cu`."""
    ext = _ext()
    q, k, v, dout, beta, g = (case[n].to(DEV) for n in ("q", "k", "v", "dout", "beta", "g"))
    if "cu" in case:
        r, s0 = ext.gdn_chunk_fwd_varlen(q, k, v, beta, g, case["cu"], False, True, True)
        drhs, ds0 = ext.gdn_chunk_bwd_scan_varlen(q, k, dout, beta, g, case["cu"])
    else:
        r, s0 = ext.gdn_chunk_fwd(q, k, v, beta, g, False, True, True)
        drhs, ds0 = ext.gdn_chunk_bwd_scan(q, k, dout, beta, g)
    return q, k, v, dout, beta, g, r, drhs, s0, ds0


def _leaf_ref(args, last_chunks, dtype=torch.float64, device="cpu"):
    """`_gdn_leaf_grads_torch` on the kernel's inputs; dS1 = ds0 one chunk
    ahead, zero at `last_chunks`."""
    from d9d_amd.module.block.attention.linear.gated_deltanet import _gdn_leaf_grads_torch

    q, k, v, dout, beta, g, r, drhs, s0, ds0 = (
        t.detach().to(device=device, dtype=dtype) for t in args
    )
    B, H, S, _ = q.shape
    ds1 = torch.cat([ds0[:, :, 1:], torch.zeros_like(ds0[:, :, :1])], 2)
    ds1[:, :, last_chunks] = 0.0
    qc, kc, vc, doc, bc, gc, rc, drc = (
        t.view(B, H, S // 64, 64, *t.shape[3:]) for t in (q, k, v, dout, beta, g, r, drhs)
    )
    outs = _gdn_leaf_grads_torch(qc, kc, vc, doc, bc, gc.cumsum(-1), rc, drc, s0, ds1)
    return {n: t.reshape(B, H, S, *t.shape[4:]) for n, t in zip(kr.GDN_GRADS, outs)}


def _check(got, ref, what):
    got = dict(zip(kr.GDN_GRADS, got))
    for n in kr.GDN_GRADS:
        assert got[n].dtype == torch.float32 and got[n].shape == ref[n].shape
        print(f"{what} {n}: need {kr.tol_needed(got[n], ref[n]):.3g}, "
              f"max |ref| {float(ref[n].abs().max()):.3g}")
    for n in kr.GDN_GRADS:
        kr.assert_close(got[n], ref[n], _tol(n, ref[n]), f"{what} {n}")
    return got


@pytest.mark.parametrize("shape", LEAF_SHAPES, ids=str)
def test_gdn_bwd_leaf_parity(shape):
    """All five outputs of the dense entry point; rows with beta = 0 and
    g = -6 are in every chunk."""
    case = kr.gdn_case(*shape, zero_beta=True)
    assert float(case["beta"].min()) == 0.0 and float(case["g"].min()) == -6.0
    args = _leaf_args(case)
    _check(_ext().gdn_chunk_bwd_leaf(*args), _leaf_ref(args, [-1]), str(shape))


def test_gdn_bwd_leaf_document_boundaries():
    """Packed documents of 64, 128 and 64 rows: chunks 0, 2 and 3 end a
    document and take dS1 = 0. The dense entry point on the same buffers lets
    chunk 1's ds0 into chunk 0, so its dk there must differ by more than
    the tolerance."""
    case, _ = kr.gdn_varlen_case([64, 128, 64], 2)
    args = _leaf_args(case)
    ref = _leaf_ref(args, [0, 2, 3])
    got = _check(_ext().gdn_chunk_bwd_leaf_varlen(*args, case["cu"]), ref, "varlen")
    dense_dk = _ext().gdn_chunk_bwd_leaf(*args)[1]
    leak = (dense_dk[:, :, :64] - got["dk"][:, :, :64]).abs().max()
    assert float(leak) > _tol("dk", ref["dk"])["atol"], float(leak)


def test_gdn_bwd_leaf_flag(monkeypatch):
    """D9D_GDN_BWD_LEAF=0 (torch stage) and =1 (kernel) through the op, on
    fp32 leaves so no gradient is rounded to bf16 on the way out: they agree
    within the parity tolerance and both meet the fp64 recurrence."""
    from d9d_amd.module.block.attention.linear.gated_deltanet import chunk_gated_delta_rule

    case = kr.gdn_case(2, 3, 128)
    step = kr.gdn_step_ref(case, backward=True)
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("D9D_GDN_BWD_LEAF", flag)
        leaves = [case[n].to(DEV).float().requires_grad_(True) for n in ("q", "k", "v", "beta", "g")]
        out = chunk_gated_delta_rule(*leaves)
        (out.float() * case["dout"].to(DEV).float()).sum().backward()
        res[flag] = dict(zip(kr.GDN_GRADS, (t.grad for t in leaves)))
        for n in kr.GDN_GRADS:
            kr.assert_close(res[flag][n], step[n], kr.TOL_GDN_GRAD[n], f"flag {flag} {n}")
    for n in kr.GDN_GRADS:
        ref = res["0"][n].cpu().double()
        kr.assert_close(res["1"][n], ref, _tol(n, ref), f"kernel vs torch stage {n}")


def test_gdn_bwd_leaf_rejects_bad_arguments():
    """Wrong dtype, S % 64 != 0, a non-contiguous r, an s0 with the wrong
    chunk count and unaligned document boundaries raise before any launch."""
    ext = _ext()
    args = list(_leaf_args(kr.gdn_case(1, 2, 128)))
    q, r, s0 = args[0], args[6], args[8]

    def swapped(i, t):
        return args[:i] + [t] + args[i + 1:]

    r_strided = torch.cat([r, r], -1)[..., ::2]
    assert r_strided.shape == r.shape and not r_strided.is_contiguous()
    bad_calls = [
        lambda: ext.gdn_chunk_bwd_leaf(*swapped(0, q.float())),
        lambda: ext.gdn_chunk_bwd_leaf(*swapped(6, r.double())),
        lambda: ext.gdn_chunk_bwd_leaf(*swapped(6, r_strided)),
        lambda: ext.gdn_chunk_bwd_leaf(*swapped(8, torch.cat([s0, s0[:, :, :1]], 2))),
        lambda: ext.gdn_chunk_bwd_leaf(*(t[:, :, :100] if t.dim() < 5 else t for t in args)),
        lambda: ext.gdn_chunk_bwd_leaf_varlen(
            *args, torch.tensor([0, 32, 128], dtype=torch.int32)),
    ]
    for i, bad in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="gdn_chunk_bwd_leaf"):
            bad()
            pytest.fail(f"bad call {i} was accepted")
