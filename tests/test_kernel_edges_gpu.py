"""Kernel-edge cases on the HIP kernels (MI355X).

Every dispatch branch of the host wrappers in d9d_amd/csrc (template
instantiations, tails, grid-stride loops) against the fp64 references of
tests/kernel_refs.py, on the cases tests/test_kernel_edges.py validates on the
CPU. The inputs are generated on the CPU, so both suites see the same bits.

Branch -> test:
  rms head-norm kernel, dw_part reduce, row loop ....... test_rms_norm_head_kernel
  rms small-N VPL 1/2/4/8, odd N, N == 64*VPL, loop .... test_rms_norm_small_n_kernel
  rms LDS kernel tails and both grid caps .............. test_rms_norm_lds_kernel
  cce_fwd KT=64, T < 64, T == 1, V < 128, padded tile .. test_cce_fwd_edges
  cce_fwd vocab_start != 0 ............................. test_cce_fwd_vocab_shards
  cce_fwd lse of the bf16-rounded logits ............... test_cce_fwd_rounded_lse
  cce_dlogits_ filter, tails, odd V, shard, both loops . test_cce_dlogits_edges
  cce default filter end to end ........................ test_cce_end_to_end_default_filter
  router E/K edges, decisive bias, margin rule ......... test_router_edges
  router exact ties .................................... test_router_ties_pick_lower_index
  router K > E, non-fp32 logits ........................ test_router_top_k_above_experts_raises,
                                                         test_router_bf16_logits_fall_back
  moe H tails, H < 8, H > 512, K == 1, empty experts ... test_moe_permute_edges,
                                                         test_moe_unpermute_edges, test_moe_*_direct
  moe dtype dispatch and argument checks ............... test_moe_permute_fp32_takes_index_path,
                                                         test_moe_entry_points_reject_bad_arguments
  rope grid loop, rope_dim 4/32, D % 8, rope_dim < D ... test_rope_edges
  rope expanded cos/sin in the backward ................ test_rope_expanded_cos_sin
  attention D templates and padded D, fwd + bwd ........ test_attn_head_dims
  attention q_offset, Sq != Skv, fwd + bwd ............. test_attn_q_offset
  attention windows, window + sinks .................... test_attn_window
  attention varlen window / sinks / cross lengths ...... test_attn_varlen
  attention non-causal ragged bwd ...................... test_attn_noncausal_ragged
  attention dlse ....................................... test_attn_dlse, test_attn_varlen_dlse,
                                                         test_attn_lse_only_loss
  gdn fwd DVT=32 / DVT=64, S < 64, tails, chunk carry,
    planted solve; out, final_state, r, s0 ............. test_gdn_fwd_edges
  gdn fwd return-list order per flag triple ............ test_gdn_fwd_return_order
  gdn bwd scan kernels DVT=32 / DVT=64 through the op .. test_gdn_bwd_edges[(2,3,128)/(1,193,128)]
  gdn bwd pad != 0 torch-scan branch on the GPU ........ test_gdn_bwd_edges[(2,3,130)]
  gdn varlen fwd + bwd, per-document reference ......... test_gdn_varlen_bwd
  gdn_chunk_bwd_scan tail rows (direct call, S = 100) .. test_gdn_bwd_scan_tail
  conv K 1..4, S < K, grid loop ........................ test_conv_silu_edges
  SR copy seed contract, tail salt, both loops twice ... test_sr_copy_bitwise
  adamw single kernel, tails, second grid iteration .... test_adamw_edges, test_adamw_sr_mean
  adamw multi per-tensor step/seed, empty tensor ....... test_adamw_multi_steps_and_seeds
  adamw multi pipelined loop, walk across tensors ...... test_adamw_multi_pipelined_loop
  adamw multi split at the LDS limit ................... test_adamw_multi_many_tensors
  StochasticAdamW seed formula, grad None, fp32 grad ... test_stochastic_adamw_class
  add_bf16_into_f32_ tail and grid loop ................ test_add_bf16_into_f32
  silu_mul tails, grid loop, extreme gates ............. test_silu_mul_edges
  silu_mul_packed grid loop, last columns, I % 8 ....... test_silu_mul_packed_edges,
                                                         test_silu_mul_packed_needs_multiple_of_8
  gdn / conv / silu / adamw-multi argument checks ...... test_*_reject_bad_arguments
"""

import pytest
import torch

from tests import kernel_refs as kr
from tests.test_kernel_edges import (
    ATTN_HEAD_DIMS,
    ATTN_Q_OFFSETS,
    ATTN_WINDOWS,
    BOTH,
    MOE_CASES,
    VARLEN_CASES,
    _permute_run,
    _unpermute_run,
    adamw_single_run,
    attn_run,
    attn_varlen_run,
    check_stochastic_adamw_class,
    conv_run,
    gdn_op_run,
    silu_packed_run,
    silu_run,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ext():
    from d9d_amd.ops._ext import get_ext

    return get_ext()


# ---- RMSNorm -----------------------------------------------------------------


def _rms_gpu(x, w, dy, zero_centered):
    ext = _ext()
    x, w, dy = x.to(DEV), w.to(DEV), dy.to(DEV)
    y, inv = ext.rms_norm_fwd(x, w, kr.RMS_EPS, zero_centered)
    dx, dw = ext.rms_norm_bwd(x, w, dy, inv, zero_centered)
    assert dw.dtype == torch.float32
    return y, inv, dx, dw


@pytest.mark.parametrize("zero_centered", BOTH)
@pytest.mark.parametrize("shape", kr.RMS_HEAD_SHAPES, ids=str)
def test_rms_norm_head_kernel(shape, zero_centered):
    """N <= 128 and N % 8 == 0: the q/k-norm kernel, its row loop and the
    dw_part reduction ((65541, 64) is more than 4096 blocks x 16 rows)."""
    kr.check_rms(_rms_gpu, *shape, zero_centered)


@pytest.mark.parametrize("zero_centered", BOTH)
@pytest.mark.parametrize("shape", kr.RMS_SMALL_SHAPES, ids=str)
def test_rms_norm_small_n_kernel(shape, zero_centered):
    """One wave per row at VPL 1, 2, 4, 8, odd row pitch, N == 64*VPL, and
    the grid-stride loop ((8200, 60))."""
    kr.check_rms(_rms_gpu, *shape, zero_centered)


@pytest.mark.parametrize("zero_centered", BOTH)
@pytest.mark.parametrize("shape", kr.RMS_LDS_SHAPES, ids=str)
def test_rms_norm_lds_kernel(shape, zero_centered):
    """N > 512: scalar tails and both row loops ((2100, 520))."""
    kr.check_rms(_rms_gpu, *shape, zero_centered)


def test_rms_norm_4d():
    from d9d_amd.ops import rms_norm

    x, w, dy = kr.rms_case(24, 64)
    x4 = x.view(2, 3, 4, 64).to(DEV).requires_grad_(True)
    w4 = w.to(DEV).requires_grad_(True)
    y = rms_norm(x4, w4, eps=kr.RMS_EPS)
    y.backward(dy.view(2, 3, 4, 64).to(DEV))
    ry, _, rdx, rdw = kr.rms_ref(x, w, dy, False)
    kr.assert_close(y.view(24, 64), ry, kr.TOL_RMS_Y, "y")
    kr.assert_close(x4.grad.view(24, 64), rdx, kr.TOL_RMS_DX, "dx")
    kr.assert_close(w4.grad, rdw, kr.TOL_RMS_DW, "dw")


# ---- CCE ---------------------------------------------------------------------


def _cce_fwd_gpu(e, c, targets, vocab_start):
    from d9d_amd.ops.cce import _can_use_kernel, _kernel_forward

    e, c = e.to(DEV), c.to(DEV)
    assert _can_use_kernel(e, c)
    return _kernel_forward(e, c, targets.to(DEV), vocab_start)


@pytest.mark.parametrize("shape", kr.CCE_FWD_SHAPES, ids=str)
def test_cce_fwd_edges(shape):
    """KT=64 (K % 128 != 0) and KT=128, K = 1024, T < 64, T == 1, V < 128,
    the dominant logit and the target in the padded last vocab tile."""
    kr.check_cce_fwd(_cce_fwd_gpu, *shape)


@pytest.mark.parametrize("shape", [(130, 1000, 320), (70, 333, 1024)], ids=str)
def test_cce_fwd_rounded_lse(shape):
    """The third output of cce_fwd: the lse of the bf16-rounded logits."""
    from d9d_amd.ops.cce import _kernel_forward

    def run(e, c, targets):
        return _kernel_forward(e.to(DEV), c.to(DEV), targets.to(DEV), 0, True)[2]

    kr.check_cce_rounded_lse(run, *shape)


def test_cce_fwd_vocab_shards():
    """vocab_start != 0: three shards merged like the vocab-parallel path."""
    kr.check_cce_vocab_parallel(_cce_fwd_gpu)


def _dlogits_gpu(logits, lse, targets, dl, dlse, vocab_start, eps):
    buf = logits.to(DEV)
    out = _ext().cce_dlogits_(
        buf, lse.to(DEV), targets.to(DEV), dl.to(DEV),
        dlse.to(DEV) if dlse is not None else None, vocab_start, kr.IGNORE, eps,
    )
    assert out.data_ptr() == buf.data_ptr()  # in place
    return out


@pytest.mark.parametrize("eps", kr.CCE_FILTER_EPS)
@pytest.mark.parametrize("vocab_start", [0, 1000])
@pytest.mark.parametrize("with_dlse", BOTH)
@pytest.mark.parametrize("shape", kr.CCE_DLOGITS_SHAPES, ids=str)
def test_cce_dlogits_edges(shape, with_dlse, vocab_start, eps):
    """filter_eps > 0, V % 8 != 0 and odd V, vocab_start != 0, the row loop
    ((4200, 40)) and the column loop (V = 128*2048 + 13)."""
    kr.check_cce_dlogits(_dlogits_gpu, *shape, vocab_start, with_dlse, eps)


def test_cce_end_to_end_default_filter():
    """linear_cross_entropy with the training default filter_eps="auto",
    reduction="mean" and ignored targets against the filtered fp64 reference.

    The mean loss is multiplied by the valid-token count n before backward,
    so each token's gradient has scale 1 instead of 1/n: at 1/n every element
    of de and dc is below the absolute tolerance and zeros would pass."""
    from d9d_amd.ops.cce import linear_cross_entropy

    e, c, targets = kr.cce_case(130, 1001, 192)
    n = int((targets != kr.IGNORE).sum())
    assert n < targets.numel()
    e_d = e.to(DEV).requires_grad_(True)
    c_d = c.to(DEV).requires_grad_(True)
    loss = linear_cross_entropy(e_d, c_d, targets.to(DEV), reduction="mean")
    (loss * n).backward()
    rloss, rde, rdc = kr.cce_e2e_ref(e, c, targets, 2.0 ** -12)
    _, _, udc = kr.cce_e2e_ref(e, c, targets, 0.0)
    rde, rdc, udc = rde * n, rdc * n, udc * n
    kr.assert_close(loss, rloss, kr.TOL_CCE_LSE, "loss")
    kr.assert_close(e_d.grad, rde, kr.TOL_CCE_DE_UNIT, "de")
    kr.assert_close(c_d.grad, rdc, kr.TOL_CCE_DC_UNIT, "dc")
    # the filter ran: over all of dc it moves the gradient by 0.63 (L2), twice
    # the bf16 rounding noise (0.34 for bf16 eager), so dc is nearer to the
    # filtered reference than to the unfiltered one. In de the filter's 0.035
    # is below the noise (0.07) and cannot be told apart.
    dc64 = c_d.grad.cpu().double()
    to_filtered, to_unfiltered = float((dc64 - rdc).norm()), float((dc64 - udc).norm())
    assert to_filtered < to_unfiltered, (to_filtered, to_unfiltered)


# ---- Router ------------------------------------------------------------------


def _router_gpu(logits, bias, K, renorm, dtop):
    from d9d_amd.ops.router import router_topk

    z = logits.to(DEV).requires_grad_(True)
    top, idx = router_topk(z, bias.to(DEV) if bias is not None else None, K, renorm)
    assert type(top.grad_fn).__name__ == "_RouterTopKFunctionBackward"  # the kernel ran
    top.backward(dtop.to(DEV))
    return top.detach(), idx, z.grad


@pytest.mark.parametrize("renorm", BOTH)
@pytest.mark.parametrize("bias_kind", kr.ROUTER_BIAS)
@pytest.mark.parametrize("shape", kr.ROUTER_SHAPES, ids=str)
def test_router_edges(shape, bias_kind, renorm):
    """E < 64, E in {64, 65}, E = 1024, K in {1, 16, E}, a bias that decides
    the selection; exact indices on every row decided by a margin."""
    kr.check_router(_router_gpu, *shape, bias_kind, renorm)


@pytest.mark.parametrize("renorm", BOTH)
def test_router_ties_pick_lower_index(renorm):
    from d9d_amd.ops.router import router_topk

    logits, K, want = kr.router_tie_case()
    _, idx = router_topk(logits.to(DEV), None, K, renorm)
    kr.assert_bitwise(idx, want, "tie order")


def test_router_top_k_above_experts_raises():
    from d9d_amd.ops.router import router_topk

    logits = torch.randn(4, 3, device=DEV)
    with pytest.raises(ValueError, match="top_k"):
        router_topk(logits, None, 4)
    with pytest.raises(RuntimeError, match="top_k"):
        _ext().router_topk_fwd(logits, None, 4, True)


def test_router_bf16_logits_fall_back():
    from d9d_amd.ops.router import _torch_router, router_topk

    logits, _, _, _ = kr.router_case(33, 16, 4, "none")
    z = logits.to(DEV).bfloat16()
    top, idx = router_topk(z, None, 4, True)
    rtop, ridx = _torch_router(z, None, 4, True)
    assert top.dtype == torch.bfloat16
    assert torch.equal(idx, ridx) and torch.equal(top, rtop)
    with pytest.raises(RuntimeError, match="fp32"):
        _ext().router_topk_fwd(z, None, 4, True)


# ---- MoE permute / combine ----------------------------------------------------


@pytest.mark.parametrize("case", MOE_CASES, ids=str)
def test_moe_permute_edges(case):
    """H % 8 != 0, H < 8, H > 512, K == 1, empty experts, one expert taking
    every token: rows, probs, counts and order bitwise; d tokens through
    moe_csr_combine without probs."""
    kr.check_moe_permute(_permute_run(DEV), *case)


@pytest.mark.parametrize("case", MOE_CASES, ids=str)
def test_moe_unpermute_edges(case):
    """Row-distinct expert_out, non-uniform probs, random upstream grad."""
    kr.check_moe_unpermute(_unpermute_run(DEV), *case)


def test_moe_permute_fp32_takes_index_path():
    kr.check_moe_permute(_permute_run(DEV), 37, 4, 8, 2, dtype=torch.float32)


def _moe_raw_case():
    case = kr.moe_case(50, 1037, 128, 8)
    order, row_to_token, _ = kr.moe_permute_ref(case["indices"], 128)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())
    return case, order, row_to_token, inv


def test_moe_gather_rows_direct():
    case, order, row_to_token, _ = _moe_raw_case()
    ext = _ext()
    src = case["tokens"].to(DEV)
    got = ext.moe_gather_rows(src, row_to_token.to(DEV), None)
    kr.assert_bitwise(got, case["tokens"][row_to_token], "gather")
    scale = case["probs"].reshape(-1)[order]
    src2 = case["grad_out"]
    got = ext.moe_gather_rows(src2.to(DEV), row_to_token.to(DEV), scale.to(DEV))
    ref = src2.double()[row_to_token] * scale.double().unsqueeze(1)
    kr.assert_close(got, ref, kr.TOL_COMBINE, "scaled gather")


@pytest.mark.parametrize("with_probs", BOTH)
def test_moe_csr_combine_direct(with_probs):
    case, order, row_to_token, inv = _moe_raw_case()
    T, K = case["indices"].shape
    eo = case["expert_out"]
    pp = case["probs"].reshape(-1)[order]
    got = _ext().moe_csr_combine(
        eo.to(DEV), pp.to(DEV) if with_probs else None, inv.to(DEV), T, K
    )
    weighted = eo.double() * (pp.double().unsqueeze(1) if with_probs else 1.0)
    ref = torch.zeros(T, eo.shape[1], dtype=torch.float64).index_add_(0, row_to_token, weighted)
    kr.assert_close(got, ref, kr.TOL_COMBINE, "combine")


def test_moe_row_dot_direct():
    case, _, row_to_token, _ = _moe_raw_case()
    got = _ext().moe_row_dot(
        case["grad_out"].to(DEV), case["expert_out"].to(DEV), row_to_token.to(DEV)
    )
    ref = (case["grad_out"].double()[row_to_token] * case["expert_out"].double()).sum(-1)
    assert got.dtype == torch.float32
    kr.assert_close(got, ref, kr.TOL_FP32, "row dot")


def test_moe_entry_points_reject_bad_arguments():
    """Wrong dtype, device or strides raise instead of being reinterpreted."""
    ext = _ext()
    case, order, row_to_token, inv = _moe_raw_case()
    T, K = case["indices"].shape
    eo, go = case["expert_out"].to(DEV), case["grad_out"].to(DEV)
    r2t, inv_d = row_to_token.to(DEV), inv.to(DEV)
    pp = case["probs"].reshape(-1)[order].to(DEV)
    strided = torch.stack([inv_d, inv_d], 1)[:, 0]
    assert not strided.is_contiguous()
    bad_calls = [
        lambda: ext.moe_gather_rows(go.float(), r2t, None),
        lambda: ext.moe_gather_rows(go, r2t.int(), None),
        lambda: ext.moe_gather_rows(go, r2t, pp.bfloat16()),
        lambda: ext.moe_gather_rows(go, row_to_token, None),
        lambda: ext.moe_csr_combine(eo.float(), None, inv_d, T, K),
        lambda: ext.moe_csr_combine(eo, pp.double(), inv_d, T, K),
        lambda: ext.moe_csr_combine(eo, None, strided, T, K),
        lambda: ext.moe_csr_combine(eo, None, inv_d.int(), T, K),
        lambda: ext.moe_csr_combine(eo, None, inv_d, T, K + 1),
        lambda: ext.moe_row_dot(go.float(), eo, r2t),
        lambda: ext.moe_row_dot(go, eo.float(), r2t),
        lambda: ext.moe_row_dot(go, eo, r2t.int()),
        lambda: ext.moe_row_dot(go[:, :8], eo, r2t),
        lambda: ext.moe_row_dot(go, eo, row_to_token),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="moe_"):
            call()
            pytest.fail(f"bad call {i} was accepted")


# ---- RoPE --------------------------------------------------------------------


def _table_to_dev(t):
    # .to() would densify a batch-broadcast table: move one copy and expand
    if t.stride(0) == 0:
        return t[:1].to(DEV).expand(*t.shape)
    return t.to(DEV)


def _rope_gpu(q, k, cos, sin, gq, gk):
    from d9d_amd.ops.rope import rope_qk, rope_qk_available

    q_d = q.to(DEV).requires_grad_(True)
    k_d = k.to(DEV).requires_grad_(True)
    assert rope_qk_available(q_d, cos.shape[-1])
    qo, ko = rope_qk(q_d, k_d, _table_to_dev(cos), _table_to_dev(sin))
    ((qo.float() * gq.to(DEV).float()).sum() + (ko.float() * gk.to(DEV).float()).sum()).backward()
    return qo.detach(), ko.detach(), q_d.grad, k_d.grad


@pytest.mark.parametrize("shape", kr.ROPE_SHAPES, ids=str)
def test_rope_edges(shape):
    """rope_dim in {4, 32, 64}, D % 8 != 0, rope_dim < D in both directions,
    and 524 544 work items (one block past the 2048 x 256 grid cap)."""
    kr.check_rope(_rope_gpu, *shape)


def test_rope_expanded_cos_sin():
    """A batch-broadcast cos/sin works forward AND backward."""
    _, _, cos, _, _, _ = kr.rope_case(2, 33, 2, 2, 64, 64, expanded=True)
    assert not _table_to_dev(cos).is_contiguous()
    kr.check_rope(_rope_gpu, 2, 33, 2, 2, 64, 64, expanded=True)


# ---- Attention ---------------------------------------------------------------


@pytest.mark.parametrize("D", ATTN_HEAD_DIMS)
def test_attn_head_dims(D):
    """Every template (32, 64, 96, 128) and padded head dims (16, 40, 80) in
    both directions, more than one q and kv tile."""
    kr.check_attn(attn_run(DEV), kr.attn_case(1, 130, 130, 4, 2, D))


@pytest.mark.parametrize("sq,skv,off", ATTN_Q_OFFSETS)
def test_attn_q_offset(sq, skv, off):
    """Sq != Skv with q_offset, forward and backward, against the reference."""
    kr.check_attn(attn_run(DEV), kr.attn_case(1, sq, skv, 4, 2, 64, q_offset=off))


@pytest.mark.parametrize("with_sinks", BOTH)
@pytest.mark.parametrize("window_left", ATTN_WINDOWS)
def test_attn_window(window_left, with_sinks):
    """Windows of 0, below a tile, not a multiple of 16, a tile, and >= S;
    alone and with sinks."""
    case = kr.attn_case(1, 200, 200, 4, 2, 64, window_left=window_left, with_sinks=with_sinks)
    kr.check_attn(attn_run(DEV), case)


def test_attn_noncausal_ragged():
    kr.check_attn(attn_run(DEV), kr.attn_case(2, 130, 130, 4, 2, 64, causal=False))


@pytest.mark.parametrize("name", list(VARLEN_CASES))
def test_attn_varlen(name):
    """Varlen with a window, with sinks, and with len_q < len_k (backward)."""
    case = kr.attn_varlen_case(Hq=4, Hkv=2, D=64, **VARLEN_CASES[name])
    kr.check_attn_varlen(attn_varlen_run(DEV), case)


@pytest.mark.parametrize("with_sinks", BOTH)
def test_attn_dlse(with_sinks):
    """A loss through lse reaches dq, dk and dsinks."""
    case = kr.attn_case(1, 130, 130, 4, 2, 64, with_sinks=with_sinks)
    kr.check_attn(attn_run(DEV), case, use_dlse=True)


@pytest.mark.parametrize("with_sinks", BOTH)
def test_attn_varlen_dlse(with_sinks):
    case = kr.attn_varlen_case([37, 130], [37, 130], 4, 2, 64, with_sinks=with_sinks)
    kr.check_attn_varlen(attn_varlen_run(DEV), case, use_dlse=True)


def test_attn_lse_only_loss():
    """No grad reaches `out`: the backward still runs and is the lse term."""
    from d9d_amd.ops.attention import flash_attn_func

    case = kr.attn_case(1, 70, 70, 4, 2, 64)
    q, k, v = (case[n].to(DEV).requires_grad_(True) for n in ("q", "k", "v"))
    _, lse = flash_attn_func(q, k, v, softmax_scale=case["scale"], return_lse=True)
    (lse * case["dlse"].to(DEV)).sum().backward()
    q64, k64, v64 = (case[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    _, rlse = kr.attn_fwd64(q64, k64, v64, True, case["scale"], -1, None, 0)
    (rlse * case["dlse"].double()).sum().backward()
    kr.assert_close(q.grad, q64.grad, kr.TOL_ATTN_DQ, "dq")
    kr.assert_close(k.grad, k64.grad, kr.TOL_ATTN_GRAD, "dk")
    assert float(v.grad.abs().max()) == 0.0


# ---- GatedDeltaNet -------------------------------------------------------------


def _gdn_dev(case, names=("q", "k", "v", "beta", "g")):
    return [case[n].to(DEV) for n in names]


def _gdn_fwd_gpu(case):
    out, fs, r, s0 = _ext().gdn_chunk_fwd(*_gdn_dev(case), True, True, False)
    assert out.dtype == torch.bfloat16 and fs.dtype == r.dtype == s0.dtype == torch.float32
    return dict(out=out, fs=fs, r=r, s0=s0)


@pytest.mark.parametrize("shape", kr.GDN_FWD_SHAPES, ids=str)
def test_gdn_fwd_edges(shape):
    """Both Dv instantiations (B*H = 6 -> DVT 32, B*H = 193 -> DVT 64),
    S = 1, S < 64, S = 64, one tail row, a tail after two chunks, three full
    chunks; runs of a repeated key (a solve that is far from the identity),
    state wipes, beta = 0 rows and a poisoned row behind every tail. All four
    outputs against the fp64 recurrence."""
    kr.check_gdn_fwd(_gdn_fwd_gpu, *shape)


def test_gdn_fwd_return_order():
    """[out unless skip_out] + [final_state if return_state] + [r, s0 if
    return_aux], each equal to what the full call returns."""
    case = kr.gdn_case(2, 3, 65)
    args = _gdn_dev(case)
    full = _gdn_fwd_gpu(case)
    for return_state, return_aux, skip_out in kr.GDN_FLAG_TRIPLES:
        got = _ext().gdn_chunk_fwd(*args, return_state, return_aux, skip_out)
        want = ([] if skip_out else ["out"]) + (["fs"] if return_state else []) + (
            ["r", "s0"] if return_aux else []
        )
        assert len(got) == len(want), (return_state, return_aux, skip_out)
        for name, t in zip(want, got):
            kr.assert_same_bits(t, full[name], f"{name} of {(return_state, return_aux, skip_out)}")


@pytest.mark.parametrize("shape", kr.GDN_BWD_SHAPES, ids=str)
def test_gdn_bwd_edges(shape):
    """chunk_gated_delta_rule forward + backward against autograd on the
    fp64 recurrence: the scan kernels at both Dv widths (S = 128) and the
    torch-scan branch a tail selects on the GPU (S = 130)."""
    kr.check_gdn_bwd(gdn_op_run(DEV), *shape)


def test_gdn_varlen_bwd():
    """Packed documents of 1, 64, 63, 65, 0, 130 and 7 rows through the
    varlen kernels; each document against the recurrence on it alone."""
    kr.check_gdn_varlen_bwd(gdn_op_run(DEV), kr.GDN_VARLEN_LENS, 3)


def test_gdn_bwd_scan_tail():
    """gdn_chunk_bwd_scan at S = 100: the op never sends it a tail, a direct
    call does. drhs = dv / beta and dS0 = the boundary state's gradient."""

    def run(case):
        drhs, ds0 = _ext().gdn_chunk_bwd_scan(*_gdn_dev(case, ("q", "k", "dout", "beta", "g")))
        return drhs, ds0

    kr.check_gdn_bwd_scan(run, 2, 3, 100)


@pytest.mark.parametrize("shape", kr.CONV_SHAPES, ids=str)
def test_conv_silu_edges(shape):
    """K = 1..4 with S below, at and above K, and the grid-stride loop
    ((2, 1030, 1024, 4) is 2 109 440 elements for 8192 x 256 threads)."""
    kr.check_conv(conv_run(DEV), *shape)


def test_gdn_entry_points_reject_bad_arguments():
    """The dense chunk entry points and the conv backward refuse what the
    kernels would reinterpret. Every bad tensor is at least as large as the
    good one."""
    ext = _ext()
    case = kr.gdn_case(1, 2, 70)
    q, k, v, beta, g = _gdn_dev(case)
    dout = case["dout"].to(DEV)
    longer = torch.cat([k, k[:, :, :1]], 2)
    beta_longer = torch.cat([beta, beta[:, :, :1]], 2)
    for name, fn, third in (("gdn_chunk_fwd", lambda *a: ext.gdn_chunk_fwd(*a, False, False, False), v),
                            ("gdn_chunk_bwd_scan", ext.gdn_chunk_bwd_scan, dout)):
        bad_calls = [
            lambda: fn(q, k.float(), third, beta, g),
            lambda: fn(q, k, third.float(), beta, g),
            lambda: fn(q.float(), k, third, beta, g),
            lambda: fn(q, longer, third, beta, g),
            lambda: fn(q, k, longer, beta, g),
            lambda: fn(q, case["k"], third, beta, g),
            lambda: fn(q, k, third.cpu(), beta, g),
            lambda: fn(q, k, third, case["beta"], g),
            lambda: fn(q, k, third, beta, case["g"]),
            lambda: fn(q, k, third, beta_longer, g),
            lambda: fn(q, k, third, beta, beta_longer),
            lambda: fn(q, k, third, beta.unsqueeze(-1), g),
            lambda: fn(q[0], k[0], third[0], beta[0], g[0]),
        ]
        for i, call in enumerate(bad_calls):
            with pytest.raises(RuntimeError, match=name):
                call()
                pytest.fail(f"{name}: bad call {i} was accepted")
    x, w, dy = (t.to(DEV) for t in kr.conv_case(2, 37, 48, 4))
    bad_calls = [
        lambda: ext.causal_conv_silu_bwd(x.float(), w, dy),
        lambda: ext.causal_conv_silu_bwd(x, w.float(), dy),
        lambda: ext.causal_conv_silu_bwd(x, w, dy.float()),
        lambda: ext.causal_conv_silu_bwd(x, w, dy.cpu()),
        lambda: ext.causal_conv_silu_bwd(x, w.cpu(), dy),
        lambda: ext.causal_conv_silu_bwd(x, w, torch.cat([dy, dy], 1)),
        lambda: ext.causal_conv_silu_bwd(x, torch.cat([w, w], 0), dy),
        lambda: ext.causal_conv_silu_bwd(x, torch.cat([w, w], 1), dy),
        lambda: ext.causal_conv_silu_bwd(x[0], w, dy[0]),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="causal_conv_silu_bwd"):
            call()
            pytest.fail(f"conv: bad call {i} was accepted")


# ---- Stochastic rounding and AdamW ------------------------------------------------


def _sr_copy_gpu(src, seed):
    dst = torch.empty(src.shape, dtype=torch.bfloat16, device=DEV)
    _ext().copy_fp32_to_bf16_stochastic_(dst, src.to(DEV), seed)
    return dst


@pytest.mark.parametrize("seed", [7, 2 ** 62 + 12345])
@pytest.mark.parametrize("n", kr.SR_COPY_SIZES)
def test_sr_copy_bitwise(n, seed):
    """The seed contract, bit for bit: vector body, scalar tail (n % 4), a
    second trip through both loops (n = 2 097 303), +-0, +-inf, NaN, grid
    values and the five low-half fractions on both signs. The oracle's
    statistics are asserted in the CPU suite and hold here by equality."""
    kr.check_sr_copy(_sr_copy_gpu, n, seed)


@pytest.mark.parametrize("hyper", kr.ADAMW_HYPER, ids=lambda h: f"lr{h['lr']}")
@pytest.mark.parametrize("n", kr.ADAMW_SIZES)
def test_adamw_edges(n, hyper):
    """Every element within one bf16 ulp of the fp64 step, no bias over the
    tensor, moments at fp32 accuracy; n = 2 097 303 takes both loops twice."""
    kr.check_adamw(adamw_single_run(DEV), n, hyper)


def test_adamw_sr_mean():
    kr.check_adamw_sr_mean(adamw_single_run(DEV))


ADAMW_ARGS = (1e-3, 0.9, 0.95, 1e-8, 0.01)


def _adamw_multi_vs_single(sizes, steps, seeds):
    """The documented contract: one multi-tensor launch equals per-tensor
    single-kernel calls, bit for bit, in p, exp_avg and exp_avg_sq."""
    ext = _ext()
    ps, gs, ms, vs = kr.adamw_multi_case(sizes)
    gs = [t.to(DEV) for t in gs]
    one = [[t.to(DEV) for t in lst] for lst in (ps, ms, vs)]
    many = [[t.to(DEV) for t in lst] for lst in (ps, ms, vs)]
    for i in range(len(sizes)):
        ext.adamw_stochastic_bf16_(
            one[0][i], gs[i], one[1][i], one[2][i], *ADAMW_ARGS, steps[i], seeds[i]
        )
    ext.adamw_stochastic_bf16_multi_(many[0], gs, many[1], many[2], *ADAMW_ARGS, steps, seeds)
    changed = 0
    for i in range(len(sizes)):
        for a, b, view, what in zip(one, many, (torch.int16, torch.int32, torch.int32),
                                    ("p", "exp_avg", "exp_avg_sq")):
            same = torch.equal(a[i].view(view), b[i].view(view))
            assert same, f"{what} of tensor {i} ({sizes[i]} elements) differs"
        changed += int((one[0][i].cpu() != ps[i]).sum())
    assert changed > 0.3 * sum(sizes)   # the step did something


def test_adamw_multi_steps_and_seeds():
    """A different step (bias correction) and seed per tensor, an empty
    tensor in the middle, a partial slot that still holds a 4-vector."""
    small = kr.ADAMW_MULTI_SMALL
    _adamw_multi_vs_single(small["sizes"], small["steps"], small["seeds"])


def test_adamw_multi_pipelined_loop():
    """More slots than threads: the software-pipelined loop runs, and a
    thread's second slot lies several tensors after its first."""
    sizes = kr.adamw_multi_big_sizes()
    steps = [1 + i % 7 for i in range(len(sizes))]
    seeds = [1000 + 37 * i for i in range(len(sizes))]
    _adamw_multi_vs_single(sizes, steps, seeds)


def test_adamw_multi_many_tensors():
    """1 200 tensors need more lookup-table space than one launch has LDS:
    the wrapper splits the list."""
    n = 1200
    _adamw_multi_vs_single([8] * n, [1 + i % 5 for i in range(n)], [1 + 7919 * i for i in range(n)])


def test_stochastic_adamw_class():
    check_stochastic_adamw_class(DEV)


def test_adamw_multi_rejects_bad_arguments():
    ext = _ext()
    sizes = [64, 24]
    ps, gs, ms, vs = ([t.to(DEV) for t in lst] for lst in kr.adamw_multi_case(sizes))
    steps, seeds = [1, 2], [3, 4]
    extra = torch.zeros(64, device=DEV)

    def call(ps=ps, gs=gs, ms=ms, vs=vs, steps=steps, seeds=seeds):
        return lambda: ext.adamw_stochastic_bf16_multi_(ps, gs, ms, vs, *ADAMW_ARGS, steps, seeds)

    def swap(lst, t):
        return [t] + lst[1:]

    strided = torch.zeros(64, 2, device=DEV)
    bad_calls = [
        call(gs=gs + [extra.bfloat16()]),
        call(ms=ms + [extra]),
        call(vs=vs + [extra]),
        call(steps=steps + [1]),
        call(seeds=seeds + [1]),
        call(ps=swap(ps, extra)),                               # fp32 parameter
        call(gs=swap(gs, extra)),                               # fp32 grad
        call(ms=swap(ms, extra.double())),
        call(vs=swap(vs, extra.double())),
        call(gs=swap(gs, strided.bfloat16()[:, 0])),
        call(ms=swap(ms, strided[:, 0])),
        call(ps=swap(ps, strided.bfloat16()[:, 0])),
        call(gs=swap(gs, torch.zeros(65, dtype=torch.bfloat16, device=DEV))),
        call(vs=swap(vs, torch.zeros(65, device=DEV))),
        call(gs=swap(gs, gs[0].cpu())),
        call(ms=swap(ms, ms[0].cpu())),
    ]
    for i, bad in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="adamw multi"):
            bad()
            pytest.fail(f"bad call {i} was accepted")


@pytest.mark.parametrize("n", kr.ADD_BF16_SIZES)
def test_add_bf16_into_f32(n):
    """One IEEE add per element: the 8-wide body, the scalar tail and, at
    33 554 475 elements, a second grid-stride iteration."""

    def run(acc, x):
        acc = acc.to(DEV)
        _ext().add_bf16_into_f32_(acc, x.to(DEV))
        return acc

    kr.check_add_bf16_into_f32(run, n)


# ---- SwiGLU ------------------------------------------------------------------------


@pytest.mark.parametrize("n", kr.SILU_SIZES)
def test_silu_mul_edges(n):
    """n % 8 tails, more than 2048 x 256 vectors (a second grid-stride
    iteration in both loops), gates where exp2 overflows or underflows and
    where silu' changes sign."""
    kr.check_silu(silu_run(DEV), n)


@pytest.mark.parametrize("shape", kr.SILU_PACKED_SHAPES, ids=str)
def test_silu_mul_packed_edges(shape):
    """One vector per row, I not a power of two, and 528 900 vectors (past
    the grid); the largest values in the last column of each half."""
    kr.check_silu_packed(silu_packed_run(DEV), *shape)


def test_silu_mul_packed_needs_multiple_of_8():
    ext = _ext()
    x = torch.zeros(4, 2 * 12, dtype=torch.bfloat16, device=DEV)
    g = torch.zeros(4, 12, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="I % 8"):
        ext.silu_mul_packed_fwd(x)
    with pytest.raises(RuntimeError, match="I % 8"):
        ext.silu_mul_packed_bwd(x, g)


def test_silu_entry_points_reject_bad_arguments():
    ext = _ext()
    a, b, g = (t.to(DEV) for t in kr.silu_case(64))
    wide = torch.zeros(64, 2, dtype=torch.bfloat16, device=DEV)
    bad_calls = [
        lambda: ext.silu_mul_bwd(a, b.float(), g),
        lambda: ext.silu_mul_bwd(a, b, g.float()),
        lambda: ext.silu_mul_bwd(a, b.cpu(), g),
        lambda: ext.silu_mul_bwd(a, b, g.cpu()),
        lambda: ext.silu_mul_bwd(a, wide[:, 0], g),
        lambda: ext.silu_mul_bwd(a, b, wide[:, 0]),
        lambda: ext.silu_mul_bwd(a, torch.cat([b, b]), g),
        lambda: ext.silu_mul_bwd(a, b, torch.cat([g, g])),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="silu_mul_bwd"):
            call()
            pytest.fail(f"bad call {i} was accepted")
    x, gp = (t.to(DEV) for t in kr.silu_packed_case(3, 72))
    bad_calls = [
        lambda: ext.silu_mul_packed_bwd(x, gp.float()),
        lambda: ext.silu_mul_packed_bwd(x, gp.cpu()),
        lambda: ext.silu_mul_packed_bwd(x, torch.cat([gp, gp], 0)),
        lambda: ext.silu_mul_packed_bwd(x, torch.cat([gp, gp], 1)),
        lambda: ext.silu_mul_packed_bwd(x, torch.cat([gp, gp], 1)[:, :72]),
        lambda: ext.silu_mul_packed_bwd(x, gp.reshape(-1)),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="silu_mul_packed_bwd"):
            call()
            pytest.fail(f"packed: bad call {i} was accepted")
