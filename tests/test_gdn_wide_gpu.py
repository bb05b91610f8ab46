"""GatedDeltaNet chunk kernels at Dk = Dv = 128 (csrc/gdn.hip, the `wide`
forward and reverse-scan kernels) against the fp64 per-timestep recurrence,
on the planted cases of tests/kernel_refs.py with GDN_D = 128.

Tolerances, kernel_refs' rule: out and fs keep the project's 3e-2; every
other quantity gets twice what gdn_chunk_emul(cast=True) needs against
gdn_step_ref on the CPU (kr.tol_needed), the largest over the cases below:
    r     5.261e-4 (max |r| 1.75)     s0    1.784e-3 (max |s0| 0.24)
          on FWD_SHAPES (out needs 1.47e-2, fs 1.82e-3 there)
    dq    1.900e-2 (max |dq| 5.2)     dk    2.086e-2 (max |dk| 12)
    dv    1.587e-2 (max |dv| 4.8)     dbeta 6.415e-2 (max |dbeta| 105)
    dg    1.132e-1 (max |dg| 3.2)
          on BWD_SHAPES and GDN_VARLEN_LENS with 2 heads (dg: the 65-row document)
    drhs  1.724e-2 (max |drhs| 4.7)   dS0   2.421e-3 (max |dS0| 1.4)
          on SCAN_SHAPES with zero_beta=False
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests.test_kernel_edges import gdn_op_run

pytestmark = pytest.mark.gpu

DEV = "cuda"
# B*H = 6 takes four Dv slices of 32 (n_wg * 4 <= 256), B*H = 65 two of 64
FWD_SHAPES = [(2, 3, s) for s in (1, 63, 64, 65, 130, 192)] + [(1, 65, 128)]
SCAN_SHAPES = [(2, 3, 100), (2, 3, 128), (1, 65, 128)]
# S = 128: forward, aux and reverse scan on the kernels; S = 130: forward on
# the kernel, the scans on torch (a tail chunk)
BWD_SHAPES = [(2, 3, 128), (2, 3, 130)]


def _both(x):
    return dict(rtol=x, atol=x)


@pytest.fixture(autouse=True)
def wide(monkeypatch):
    monkeypatch.setattr(kr, "GDN_D", 128)
    monkeypatch.setattr(kr, "TOL_GDN_R", _both(1.053e-3))
    monkeypatch.setattr(kr, "TOL_GDN_S0", _both(3.567e-3))
    monkeypatch.setattr(kr, "TOL_GDN_GRAD", dict(
        dq=_both(3.80e-2), dk=_both(4.171e-2), dv=_both(3.173e-2),
        dbeta=_both(1.283e-1), dg=_both(2.264e-1)))
    monkeypatch.setattr(kr, "TOL_GDN_DRHS", _both(3.448e-2))
    monkeypatch.setattr(kr, "TOL_GDN_DS0", _both(4.842e-3))


def _ext():
    from d9d_amd.ops._ext import get_ext

    return get_ext()


def _dev(case, names):
    return [case[n].to(DEV) for n in names]


@pytest.mark.parametrize("shape", FWD_SHAPES, ids=str)
def test_gdn_wide_fwd(shape):
    """out, final state, r and s0 of gdn_chunk_fwd at both Dv widths."""

    def run(case):
        out, fs, r, s0 = _ext().gdn_chunk_fwd(
            *_dev(case, ("q", "k", "v", "beta", "g")), True, True, False)
        assert out.dtype == torch.bfloat16 and fs.shape[-2:] == s0.shape[-2:] == (128, 128)
        return dict(out=out, fs=fs, r=r, s0=s0)

    kr.check_gdn_fwd(run, *shape)


@pytest.mark.parametrize("shape", SCAN_SHAPES, ids=str)
def test_gdn_wide_bwd_scan(shape):
    """drhs = dv / beta and dS0 of gdn_chunk_bwd_scan: a tail chunk, whole
    chunks, and the two-slice instantiation."""
    kr.check_gdn_bwd_scan(
        lambda case: _ext().gdn_chunk_bwd_scan(*_dev(case, ("q", "k", "dout", "beta", "g"))),
        *shape)


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=str)
def test_gdn_wide_op_bwd(shape):
    kr.check_gdn_bwd(gdn_op_run(DEV), *shape)


def test_gdn_wide_varlen_bwd():
    """Packed documents of 1, 64, 63, 65, 0, 130 and 7 rows through the
    varlen kernels; each document against the recurrence on it alone."""
    kr.check_gdn_varlen_bwd(gdn_op_run(DEV), kr.GDN_VARLEN_LENS, 2)


def _no_torch_path(monkeypatch):
    from d9d_amd.module.block.attention.linear import gated_deltanet

    def refuse(*args, **kwargs):
        raise AssertionError("head dim 128 went to the torch path")

    monkeypatch.setattr(gated_deltanet, "_chunk_gated_delta_rule_torch", refuse)
    return gated_deltanet


def test_gdn_wide_op_takes_the_kernel(monkeypatch):
    gdn = _no_torch_path(monkeypatch)
    case = kr.gdn_case(1, 2, 128)
    with torch.no_grad():
        out = gdn.chunk_gated_delta_rule(*_dev(case, ("q", "k", "v", "beta", "g")))
    assert out.shape == (1, 2, 128, 128) and bool(torch.isfinite(out.float()).all())


def test_gdn_wide_module_matches_cpu(monkeypatch):
    """GatedDeltaNet at head dim 128, bf16 on the GPU (kernels) against the
    same weights in fp32 on the CPU. Half-unit-gain weights: activations of
    O(0.1..1), dx up to ~5. dx is a bf16 gradient summed over six
    projections, held to the project's figure for such sums, TOL_ATTN_DQ."""
    from d9d_amd.module.block.attention.linear.gated_deltanet import GatedDeltaNet

    torch.manual_seed(11)
    ref_m = GatedDeltaNet(256, num_heads=2, head_k_dim=128, head_v_dim=128)
    ref_m.reset_parameters()
    with torch.no_grad():
        for lin in (ref_m.q_proj, ref_m.k_proj, ref_m.v_proj, ref_m.beta_proj,
                    ref_m.out_gate, ref_m.o_proj):
            torch.nn.init.normal_(lin.weight, std=0.5 * lin.in_features ** -0.5)
            lin.weight.copy_(lin.weight.bfloat16().float())
    x = torch.randn(2, 128, 256).bfloat16().float()
    dout = torch.randn(2, 128, 256).bfloat16().float()
    xr = x.clone().requires_grad_(True)
    ref = ref_m(xr)
    (ref * dout).sum().backward()

    _no_torch_path(monkeypatch)
    m = GatedDeltaNet(256, num_heads=2, head_k_dim=128, head_v_dim=128)
    m.load_state_dict(ref_m.state_dict())
    m = m.to(DEV).bfloat16()
    xg = x.to(DEV).bfloat16().requires_grad_(True)
    out = m(xg)
    (out.float() * dout.to(DEV)).sum().backward()
    print(f"out need {kr.tol_needed(out, ref):.3g}, dx need {kr.tol_needed(xg.grad, xr.grad):.3g}")
    kr.assert_close(out, ref, kr.TOL_ATTN_OUT, "out")
    kr.assert_close(xg.grad, xr.grad, kr.TOL_ATTN_DQ, "dx")


def test_gdn_wide_rejects_other_head_dims():
    ext = _ext()
    q = torch.zeros(1, 2, 64, 96, device=DEV, dtype=torch.bfloat16)
    gates = torch.zeros(1, 2, 64, device=DEV)
    cu = torch.tensor([0, 64], dtype=torch.int32)
    calls = dict(
        gdn_chunk_fwd=lambda: ext.gdn_chunk_fwd(q, q, q, gates, gates, False, False, False),
        gdn_chunk_fwd_varlen=lambda: ext.gdn_chunk_fwd_varlen(
            q, q, q, gates, gates, cu, False, False, False),
        gdn_chunk_bwd_scan=lambda: ext.gdn_chunk_bwd_scan(q, q, q, gates, gates),
        gdn_chunk_bwd_scan_varlen=lambda: ext.gdn_chunk_bwd_scan_varlen(q, q, q, gates, gates, cu),
    )
    for who, call in calls.items():
        with pytest.raises(RuntimeError, match=who):
            call()
    # the leaf kernel stays D = 64 only
    q = torch.zeros(1, 2, 64, 128, device=DEV, dtype=torch.bfloat16)
    r = torch.zeros(1, 2, 64, 128, device=DEV)
    s0 = torch.zeros(1, 2, 1, 128, 128, device=DEV)
    with pytest.raises(RuntimeError, match="gdn_chunk_bwd_leaf"):
        ext.gdn_chunk_bwd_leaf(q, q, q, q, gates, gates, r, r, s0, s0)
