"""gdn_chunk_bwd_leaf_wide (csrc/gdn.hip): the per-chunk leaf gradients of the
GatedDeltaNet backward at Dk = Dv = 128 against `_gdn_leaf_grads_torch`
evaluated in fp64 on the CPU on the very tensors the kernel reads.

Tolerance per output, the rule of test_gdn_bwd_leaf_gpu.py:
    rtol = 2 * need,  atol = 2 * need + 2^-16 * max |ref|
`need` is what the fp32 torch stage on the GPU needs against the same fp64
evaluation (kr.tol_needed), largest over LEAF_SHAPES at D = 128.
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests.test_gdn_bwd_leaf_gpu import _leaf_args, _leaf_ref
from tests.test_gdn_wide_gpu import wide  # noqa: F401  autouse: GDN_D = 128 and the wide tolerances

pytestmark = pytest.mark.gpu

DEV = "cuda"
LEAF_SHAPES = [(1, 2, 64), (2, 3, 128), (1, 2, 192)]
# tol_needed against the fp64 stage, largest over LEAF_SHAPES (max |ref|: dq 5.0,
# dk 10, dv 4.5, dbeta 37, dg 3.2):
#   fp32 torch stage : dq 4.372e-6  dk 4.193e-6  dv 1.927e-8  dbeta 1.589e-5  dg 1.890e-5
#   kernel           : dq 3.683e-5  dk 3.052e-5  dv 1.927e-8  dbeta 3.818e-5  dg 5.862e-5
#   kernel, max abs error as a share of each shape's atol: dq 0.41-0.54,
#   dk 0.33-0.42, dv < 0.001, dbeta 0.17-0.31, dg 0.47-0.79 (S = 192)
LEAF_NEED = dict(dq=4.372e-6, dk=4.193e-6, dv=1.927e-8, dbeta=1.589e-5, dg=1.890e-5)
LEAF_NAMES = {False: "gdn_chunk_bwd_leaf_wide", True: "gdn_chunk_bwd_leaf_wide_varlen"}


def _leaf(args, cu=None):
    from d9d_amd.ops._ext import get_ext

    fn = getattr(get_ext(), LEAF_NAMES[cu is not None])
    return fn(*args) if cu is None else fn(*args, cu)


def _tol(name, ref):
    need = 2.0 * LEAF_NEED[name]
    return dict(rtol=need, atol=need + 2.0 ** -16 * float(ref.abs().max()))


def _check(got, ref, what):
    got = dict(zip(kr.GDN_GRADS, got))
    for n in kr.GDN_GRADS:
        assert got[n].dtype == torch.float32 and got[n].shape == ref[n].shape
        print(f"{what} {n}: need {kr.tol_needed(got[n], ref[n]):.3g}, max |ref| "
              f"{float(ref[n].abs().max()):.3g}, atol {_tol(n, ref[n])['atol']:.3g}")
    for n in kr.GDN_GRADS:
        kr.assert_close(got[n], ref[n], _tol(n, ref[n]), f"{what} {n}")
    return got


@pytest.mark.parametrize("shape", LEAF_SHAPES, ids=str)
def test_gdn_wide_leaf_parity(shape):
    """One chunk (S0 = 0, dS1 = 0), two chunks (a real S0 in one, a real dS1
    in the other), a middle chunk with both; beta = 0 rows in every chunk."""
    args = _leaf_args(kr.gdn_case(*shape, zero_beta=True))
    assert args[0].shape[-1] == 128
    _check(_leaf(args), _leaf_ref(args, [-1]), str(shape))


def test_gdn_wide_leaf_document_boundaries():
    """Documents of 64, 128 and 64 rows: chunks 0, 2 and 3 take dS1 = 0. The
    dense entry point lets chunk 1's ds0 into chunk 0's dk."""
    case, _ = kr.gdn_varlen_case([64, 128, 64], 2)
    args = _leaf_args(case)
    ref = _leaf_ref(args, [0, 2, 3])
    got = _check(_leaf(args, case["cu"]), ref, "varlen")
    leak = (_leaf(args)[1][:, :, :64] - got["dk"][:, :, :64]).abs().max()
    assert float(leak) > _tol("dk", ref["dk"])["atol"], float(leak)


def _op_grads(case):
    from d9d_amd.module.block.attention.linear.gated_deltanet import chunk_gated_delta_rule

    leaves = [case[n].to(DEV).float().requires_grad_(True) for n in ("q", "k", "v", "beta", "g")]
    out = chunk_gated_delta_rule(*leaves, cu_seqlens=case.get("cu"))
    (out.float() * case["dout"].to(DEV).float()).sum().backward()
    return dict(zip(kr.GDN_GRADS, (t.grad for t in leaves)))


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
def test_gdn_wide_leaf_dispatch_and_flag(monkeypatch, packed):
    """The op at head dim 128 never reaches the torch leaf stage, meets the
    fp64 recurrence, and agrees with D9D_GDN_BWD_LEAF=0 (the torch stage)."""
    from d9d_amd.module.block.attention.linear import gated_deltanet

    if packed:
        case, docs = kr.gdn_varlen_case([64, 128, 64], 2)
        step = kr._gdn_cat_docs([kr.gdn_step_ref(d, backward=True) for d in docs], kr.GDN_GRADS)
    else:
        case = kr.gdn_case(2, 3, 128)
        step = kr.gdn_step_ref(case, backward=True)

    def refuse(*args, **kwargs):
        raise AssertionError("head dim 128 went to the torch leaf stage")

    with monkeypatch.context() as m:
        m.setattr(gated_deltanet, "_gdn_leaf_grads_torch", refuse)
        kernel = _op_grads(case)
    for n in kr.GDN_GRADS:
        kr.assert_close(kernel[n], step[n], kr.TOL_GDN_GRAD[n], f"kernel path {n}")
    monkeypatch.setenv("D9D_GDN_BWD_LEAF", "0")
    torch_stage = _op_grads(case)
    for n in kr.GDN_GRADS:
        ref = torch_stage[n].cpu().double()
        kr.assert_close(kernel[n], ref, _tol(n, ref), f"kernel vs torch stage {n}")


def test_gdn_wide_leaf_rejects_bad_arguments():
    """Head dim 64, S % 64 != 0, a non-contiguous r, an s0 with one chunk too
    many and unaligned document boundaries raise before any launch."""
    args = list(_leaf_args(kr.gdn_case(1, 2, 128)))
    r, s0 = args[6], args[8]
    r_strided = torch.cat([r, r], -1)[..., ::2]
    assert r_strided.shape == r.shape and not r_strided.is_contiguous()
    bad_calls = [
        lambda: _leaf([t[..., :64].contiguous() for t in args[:4]] + args[4:]),
        lambda: _leaf([t[:, :, :100] if t.dim() < 5 else t for t in args]),
        lambda: _leaf(args[:6] + [r_strided] + args[7:]),
        lambda: _leaf(args[:8] + [torch.cat([s0, s0[:, :, :1]], 2)] + args[9:]),
        lambda: _leaf(args, torch.tensor([0, 32, 128], dtype=torch.int32)),
    ]
    for i, bad in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match=LEAF_NAMES[i == 4]):
            bad()
            pytest.fail(f"bad call {i} was accepted")
