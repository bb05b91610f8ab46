"""GatedDeltaNet prologue on the CPU: `gdn_prepare`'s torch chain is the glue
the block had inline, the Mamba decay gate meets its formula, and the block
runs with it."""

import math

import pytest
import torch
import torch.nn.functional as F

from d9d_amd.module.block.attention.linear import (
    GatedDeltaNet,
    MambaDecayGate,
    chunk_gated_delta_rule,
    gated_deltanet,
    step_gated_delta_rule,
)
from d9d_amd.ops import gdn_prepare, silu_mul


def _block(gate="logsigmoid", **kw):
    torch.manual_seed(3)
    m = GatedDeltaNet(32, num_heads=4, num_kv_heads=2, head_k_dim=8, head_v_dim=8,
                      decay_gate=gate, **kw)
    m.reset_parameters()
    return m


def _inline_glue_forward(m, x):
    """GatedDeltaNet.forward as it stood before `gdn_prepare`."""
    B, S, _ = x.shape
    H, Hkv = m.num_heads, m.num_kv_heads
    q = m.q_conv(m.q_proj(x)).view(B, S, Hkv, m.head_k_dim)
    k = m.k_conv(m.k_proj(x)).view(B, S, Hkv, m.head_k_dim)
    v = m.v_conv(m.v_proj(x)).view(B, S, H, m.head_v_dim)
    q = q.repeat_interleave(H // Hkv, dim=2)
    k = k.repeat_interleave(H // Hkv, dim=2)
    q = F.normalize(q.float(), dim=-1)
    k = F.normalize(k.float(), dim=-1)
    beta = torch.sigmoid(m.beta_proj(x).float())
    decay = m.decay_gate(x)
    glue = (q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3).to(v.dtype),
            beta.permute(0, 2, 1), decay.permute(0, 2, 1))
    out = m.out_norm(chunk_gated_delta_rule(*glue).permute(0, 2, 1, 3))
    gate = m.out_gate(x).view(B, S, H, m.head_v_dim)
    out = silu_mul(gate.contiguous(), out.contiguous().to(gate.dtype))
    return (q, k, v, glue), m.o_proj(out.reshape(B, S, H * m.head_v_dim))


def test_eager_prologue_is_the_inline_glue_bit_for_bit():
    m = _block()
    with torch.no_grad():
        m.decay_gate.proj.bias.normal_()  # the log-sigmoid gate's bias counts
    x = torch.randn(2, 70, 32)
    B, S = x.shape[:2]
    (_, _, v, glue), want = _inline_glue_forward(m, x)
    got = gdn_prepare(
        m.q_conv(m.q_proj(x)).view(B, S, 2, 8), m.k_conv(m.k_proj(x)).view(B, S, 2, 8), v,
        m.beta_proj(x), m.decay_gate.proj(x),
    )
    for name, a, b in zip(("qn", "kn", "vt", "beta", "g"), got, glue):
        assert a.dtype == torch.float32 and torch.equal(a, b), name
    assert torch.equal(m(x), want)


def test_mamba_gate_meets_the_fp64_formula():
    torch.manual_seed(0)
    gate = MambaDecayGate(16, 3)
    gate.reset_parameters()
    with torch.no_grad():
        gate.proj.weight.normal_(std=5.0)  # pre-activations past +-20: both softplus tails
    x = torch.randn(2, 5, 16)
    out = gate(x)
    dout = torch.randn_like(out)
    grads = torch.autograd.grad(out, [gate.proj.weight, gate.A_log, gate.dt_bias], dout)

    w, A, dt = (p.detach().double().requires_grad_(True)
                for p in (gate.proj.weight, gate.A_log, gate.dt_bias))
    z = x.double() @ w.T + dt
    assert float(z.detach().min()) < -20 and float(z.detach().max()) > 20
    ref = -torch.exp(A) * (z.clamp_min(0) + torch.log1p(torch.exp(-z.abs())))
    ref_grads = torch.autograd.grad(ref, [w, A, dt], dout.double())
    assert out.dtype == torch.float32 and bool((out <= 0).all())
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-6)
    for got, want in zip(grads, ref_grads):
        torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-5)


def test_mamba_gate_init_ranges():
    torch.manual_seed(1)
    gate = MambaDecayGate(8, 4096, normalizer=16.0, dt_min=1e-3, dt_max=0.1,
                          dt_init_floor=2e-3, dtype=torch.bfloat16)
    gate.reset_parameters()
    assert gate.proj.bias is None and gate.proj.weight.dtype == torch.bfloat16
    assert gate.A_log.dtype == gate.dt_bias.dtype == torch.float32
    A = gate.A_log.detach().exp()
    assert 0.0 < float(A.min()) < 0.1 and 15.9 < float(A.max()) <= 16.0
    dt = F.softplus(gate.dt_bias.detach())  # dt_bias is dt's inverse softplus
    assert 2e-3 * (1 - 1e-4) <= float(dt.min()) and float(dt.max()) <= 0.1 * (1 + 1e-4)
    # log-uniform on [1e-3, 0.1]: the floor at 2e-3 catches log(2) / log(100) of the draws
    floored = float((dt < 2e-3 * (1 + 1e-4)).float().mean())
    assert abs(floored - math.log(2) / math.log(100)) < 0.03


def test_block_with_mamba_gate_matches_the_step_recurrence(monkeypatch):
    m = _block("mamba")
    x = torch.randn(2, 70, 32, requires_grad=True)
    dout = torch.randn(2, 70, 32)
    grads = torch.autograd.grad(m(x), [x, *m.parameters()], dout)
    monkeypatch.setattr(
        gated_deltanet, "chunk_gated_delta_rule",
        lambda q, k, v, beta, g, cu_seqlens=None: step_gated_delta_rule(q, k, v, beta, g),
    )
    ref_grads = torch.autograd.grad(m(x), [x, *m.parameters()], dout)
    names = ["x", *(n for n, _ in m.named_parameters())]
    assert "decay_gate.A_log" in names and "decay_gate.dt_bias" in names
    for n, got, want in zip(names, grads, ref_grads):
        torch.testing.assert_close(got, want, rtol=1e-3, atol=1e-4, msg=lambda s: f"{n}: {s}")


def test_gate_choice_and_tp_refusal():
    from d9d_amd.parallel.tensor import parallelize_tp_gdn

    with pytest.raises(ValueError, match="decay_gate"):
        GatedDeltaNet(32, decay_gate="sigmoid")
    assert "decay_gate.A_log" not in dict(_block().named_parameters())
    with pytest.raises(NotImplementedError, match="Mamba"):
        parallelize_tp_gdn(_block("mamba"), None)
