"""gdn_prep_fwd / gdn_prep_bwd (csrc/gdn_prep.hip) against the prologue's
formulas in fp64 on the CPU, evaluated on the very bf16 tensors the kernels
read; the backward reference is autograd through that fp64 forward with the
fp32 incoming gradients.

Tolerance per output, the rule of test_gdn_bwd_leaf_gpu.py:
    rtol = 2 * need,  atol = 2 * need + 2^-16 * max |ref|
and one bf16 ulp (2^-8, relative) more for the bf16 outputs. `need` is what
the fp32 torch chain (`gdn_prepare_eager` on fp32 copies of the inputs, on the
GPU) needs against the same fp64 evaluation (kr.tol_needed), the largest over
SHAPES x DIMS x GATES:
    fp32 torch chain : qn 3.389e-8  kn 3.431e-8  vt 0  beta 4.120e-8  g 1.226e-7
                       dq 1.016e-7  dk 6.612e-8  dv 0  db_raw 1.767e-7  da_raw 1.596e-7
                       dA_log 4.314e-7  ddt_bias 2.615e-7
    kernels          : qn 1.112e-3  kn 7.785e-4  vt 0  beta 4.120e-8  g 1.226e-7
                       dq 2.887e-3  dk 1.284e-3  dv 2.811e-3  db_raw 1.219e-3  da_raw 3.357e-3
                       dA_log 2.091e-7  ddt_bias 7.452e-7
    (max |ref|: qn 0.53, kn 0.49, vt 4.5, beta 1.0, g 433, dq 6.0, dk 1.1, dv 4.6,
    db_raw 0.76, da_raw 24, dA_log 400, ddt_bias 86; the kernels' figures for the
    bf16 outputs are their one rounding, at most 2^-9 = 1.95e-3 of |ref| on top of
    the fp32 error, under the added ulp)
"""

import functools

import pytest
import torch

from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (B, S, H, Hkv): the 64-token tile's tail on both sides of 64, two tiles and
# a tail, rep 1 / 2 / 3, an odd H through the LDS transpose
SHAPES = [(2, 1, 2, 2), (1, 63, 4, 2), (2, 65, 3, 1), (1, 130, 5, 5)]
DIMS = [(64, 64), (128, 128), (64, 128)]
GATES = ["logsigmoid", "mamba"]
FWD = ("qn", "kn", "vt", "beta", "g")
BWD = ("dq", "dk", "dv", "db_raw", "da_raw", "dA_log", "ddt_bias")
BF16_OUT = ("qn", "kn", "vt", "dq", "dk", "dv", "db_raw", "da_raw")
NEED = dict(qn=3.389e-8, kn=3.431e-8, vt=0.0, beta=4.120e-8, g=1.226e-7,
            dq=1.016e-7, dk=6.612e-8, dv=0.0, db_raw=1.767e-7, da_raw=1.596e-7,
            dA_log=4.314e-7, ddt_bias=2.615e-7)


def _ext():
    from d9d_amd.ops._ext import get_ext

    return get_ext()


def formulas(q, k, v, b_raw, a_raw, A_log=None, dt_bias=None):
    """The prologue in the dtype of its arguments."""
    rep = v.shape[2] // q.shape[2]

    def unit(x):
        x = x.repeat_interleave(rep, dim=2)
        return (x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)).permute(0, 2, 1, 3)

    def softplus(x):
        return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))

    g = -softplus(-a_raw) if A_log is None else -torch.exp(A_log) * softplus(a_raw + dt_bias)
    return (unit(q), unit(k), v.permute(0, 2, 1, 3),
            torch.sigmoid(b_raw).permute(0, 2, 1), g.permute(0, 2, 1))


@functools.lru_cache(maxsize=None)
def case(shape, dims, gate):
    """bf16 inputs, fp32 gate parameters and incoming gradients, and the fp64
    reference of all twelve results. Planted: q row (0, 0, 0) all zero and q row
    (-1, -1, -1) of norm ~1e-20 (both under the clamp; their incoming
    gradients are scaled by 1e-12, as the clamp multiplies them by 1e12); the
    dqn rows of one q row parallel to its unit vector (the projection cancels
    to ~0); a_raw = +30 and -30."""
    (B, S, H, Hkv), (Dk, Dv) = shape, dims
    rep = H // Hkv
    gen = torch.Generator().manual_seed(B * 1000 + S + Dk)

    def rnd(*size):
        return torch.randn(*size, generator=gen)

    q, k, v = rnd(B, S, Hkv, Dk), rnd(B, S, Hkv, Dk), rnd(B, S, H, Dv)
    b_raw, a_raw = 2.0 * rnd(B, S, H), 2.0 * rnd(B, S, H)
    q[0, 0, 0] = 0.0
    q[-1, -1, -1] = 1e-20 * Dk ** -0.5
    a_raw[0, 0, 0], a_raw[-1, -1, -1] = 30.0, -30.0
    ins = [t.bfloat16() for t in (q, k, v, b_raw, a_raw)]
    if gate == "mamba":
        ins += [torch.log(16.0 * torch.rand(H, generator=gen)), rnd(H) - 3.0]
    douts = [rnd(B, H, S, Dk), rnd(B, H, S, Dk), rnd(B, H, S, Dv), rnd(B, H, S), rnd(B, H, S)]
    douts[0][0, :rep, 0] *= 1e-12
    douts[0][-1, -rep:, -1] *= 1e-12
    pb, ps = (B - 1, 0) if B > 1 else (0, 1)  # the parallel row: (pb, ps, qk head 0)
    unit = ins[0][pb, ps, 0].double()
    unit = (unit / unit.norm()).float()
    douts[0][pb, :rep, ps] = torch.arange(1, rep + 1).view(rep, 1) * unit

    leaves = [t.double().requires_grad_(True) for t in ins]
    outs = formulas(*leaves)
    grads = torch.autograd.grad(outs, leaves, [d.double() for d in douts])
    ref = dict(zip(FWD + BWD, [o.detach() for o in outs] + list(grads)))
    assert float(ref["dq"][pb, ps, 0].abs().max()) < 1e-6 * float(ref["dq"].abs().max())
    return ins, douts, ref


def run_kernels(ins, douts):
    q, k, v, b_raw, a_raw, *gate = (t.to(DEV) for t in ins)
    gate = gate or [None, None]
    got = _ext().gdn_prep_fwd(q, k, v, b_raw, a_raw, *gate)
    got += _ext().gdn_prep_bwd(q, k, b_raw, a_raw, *gate, *(d.to(DEV) for d in douts))
    return dict(zip(FWD + BWD, got))


def tol(name, ref):
    need = 2.0 * NEED[name]
    ulp = 2.0 ** -8 if name in BF16_OUT else 0.0
    return dict(rtol=need + ulp, atol=need + 2.0 ** -16 * float(ref.abs().max()))


@pytest.mark.parametrize("gate", GATES)
@pytest.mark.parametrize("dims", DIMS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gdn_prep_parity(shape, dims, gate):
    ins, douts, ref = case(shape, dims, gate)
    got = run_kernels(ins, douts)
    for n in ref:
        want = torch.bfloat16 if n in BF16_OUT else torch.float32
        assert got[n].dtype == want and got[n].is_contiguous(), n
        print(f"{n}: need {kr.tol_needed(got[n], ref[n]):.3g}, max |ref| "
              f"{float(ref[n].abs().max()):.3g}, atol {tol(n, ref[n])['atol']:.3g}")
    if gate == "logsigmoid":
        assert got["dA_log"] is None and got["ddt_bias"] is None
    assert torch.equal(got["vt"].cpu(), ins[2].permute(0, 2, 1, 3))
    for n in ref:
        kr.assert_close(got[n], ref[n], tol(n, ref[n]), n)


def test_gdn_prep_bwd_repeats_bit_for_bit():
    """Three token tiles fold into dA_log and ddt_bias in a fixed order: same bits."""
    ins, douts, _ = case(SHAPES[3], DIMS[1], "mamba")
    first, second = run_kernels(ins, douts), run_kernels(ins, douts)
    for n in BWD:
        assert torch.equal(first[n], second[n]), n


def _block_run(m, x, dout, cu):
    m.zero_grad()
    x = x.clone().requires_grad_(True)
    out = m(x, cu_seqlens=cu)
    (out.float() * dout).sum().backward()
    return dict(out=out, x=x.grad, **{n: p.grad for n, p in m.named_parameters()})


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("gate", GATES)
def test_block_fused_prologue_matches_the_torch_chain(monkeypatch, gate, packed):
    """The block with D9D_GDN_PREP=1 (F.normalize may not be reached) against
    =0, output and every gradient, at the bf16 tolerances of the block's other
    GPU tests (test_gdn_wide_gpu.py): TOL_ATTN_OUT for the output, and for the
    gradients TOL_ATTN_DQ, whose atol of 0.1 is stated there for a dx of up to
    ~5, 2% of the largest element. A parameter gradient is a sum over all B * S
    tokens and larger in that proportion (up to ~75 here), so every gradient
    gets rtol 5e-2 and atol = 2% of its own largest element."""
    from d9d_amd.module.block.attention.linear import GatedDeltaNet

    torch.manual_seed(5)
    m = GatedDeltaNet(256, num_heads=4, num_kv_heads=2, head_k_dim=128, head_v_dim=128,
                      decay_gate=gate)
    m.reset_parameters()
    with torch.no_grad():  # half-unit-gain weights: activations of O(0.1..1)
        for lin in (m.q_proj, m.k_proj, m.v_proj, m.beta_proj, m.out_gate, m.o_proj):
            torch.nn.init.normal_(lin.weight, std=0.5 * lin.in_features ** -0.5)
    m = m.to(DEV).bfloat16()
    shape, cu = ((1, 256, 256), torch.tensor([0, 64, 192, 256], dtype=torch.int32)) \
        if packed else ((2, 128, 256), None)
    x = torch.randn(shape, device=DEV).bfloat16()
    dout = torch.randn(shape, device=DEV)

    monkeypatch.setenv("D9D_GDN_PREP", "0")
    chain = _block_run(m, x, dout, cu)
    monkeypatch.setenv("D9D_GDN_PREP", "1")

    def refuse(*args, **kwargs):
        raise AssertionError("the fused prologue went to F.normalize")

    monkeypatch.setattr(torch.nn.functional, "normalize", refuse)
    fused = _block_run(m, x, dout, cu)
    assert set(fused) == set(chain) and all(g is not None for g in fused.values())
    chain = {n: t.detach().cpu().double() for n, t in chain.items()}
    for n in fused:
        print(f"{n}: max abs err {float((fused[n].detach().cpu() - chain[n]).abs().max()):.3g}, "
              f"max |chain| {float(chain[n].abs().max()):.3g}")
    kr.assert_close(fused.pop("out"), chain["out"], kr.TOL_ATTN_OUT, "out")
    for n in fused:
        scale = kr.TOL_ATTN_DQ["atol"] / 5.0 * float(chain[n].abs().max())
        kr.assert_close(fused[n], chain[n], dict(kr.TOL_ATTN_DQ, atol=scale), n)


def test_gdn_prep_rejects_bad_arguments():
    """Wrong dtype, non-contiguous q, H % Hkv != 0, head dim 96 and one gate
    parameter without the other raise before any launch."""
    ins, douts, _ = case(SHAPES[1], DIMS[0], "mamba")
    q, k, v, b_raw, a_raw, A_log, dt_bias = (t.to(DEV) for t in ins)
    q_strided = torch.cat([q, q], -1)[..., ::2]
    assert q_strided.shape == q.shape and not q_strided.is_contiguous()

    def wide(t):  # head dim 64 -> 96
        return torch.cat([t, t[..., :32]], -1).contiguous()

    bad_calls = [
        (q.float(), k, v, b_raw, a_raw, A_log, dt_bias),
        (q_strided, k, v, b_raw, a_raw, A_log, dt_bias),
        (q, k, v[:, :, :3].contiguous(), b_raw[..., :3].contiguous(),
         a_raw[..., :3].contiguous(), A_log[:3].contiguous(), dt_bias[:3].contiguous()),
        (wide(q), wide(k), v, b_raw, a_raw, A_log, dt_bias),
        (q, k, v, b_raw, a_raw, A_log, None),
    ]
    grads = [d.to(DEV) for d in douts]
    for i, bad in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="gdn_prep_fwd"):
            _ext().gdn_prep_fwd(*bad)
            pytest.fail(f"bad forward call {i} was accepted")
    with pytest.raises(RuntimeError, match="gdn_prep_bwd"):
        _ext().gdn_prep_bwd(q, k, b_raw, a_raw, A_log, dt_bias, grads[0].bfloat16(), *grads[1:])
