"""fp64 references, planted-edge case builders and checkers for the kernel
edge suite (tests/test_kernel_edges.py on the CPU paths,
tests/test_kernel_edges_gpu.py on the HIP kernels).

References take the bf16/fp32 tensors the kernel sees, upcast to fp64 and run
the textbook formula; backward references are torch.autograd on that fp64
forward. Nothing here imports from d9d_amd.ops.

Design rule for the cases: the element on the boundary a case targets carries
the answer (a large value in the last column, the winning logit on a tile
edge, a dominant key on the mask edge), so a tail or mask that is off by one
is an O(1) error and not one dropped column out of thousands.

Every case is generated on the CPU from its own seeded generator, so the CPU
and the GPU suites see bit-identical inputs. The checkers take a `run`
callable that maps the case inputs to the outputs of the implementation under
test; references are always computed on the CPU.
"""

import math

import torch

IGNORE = -100
BF16 = torch.bfloat16

# tolerances: the project's own numbers for each op (tests/test_ops_kernels.py,
# tests/test_attention_gpu.py), against the fp64 reference
TOL_RMS_Y = dict(rtol=2e-2, atol=2e-2)
TOL_RMS_DX = dict(rtol=3e-2, atol=3e-2)
TOL_RMS_DW = dict(rtol=3e-2, atol=3e-1)
TOL_ROPE = dict(rtol=2e-2, atol=2e-2)
TOL_COMBINE = dict(rtol=2e-2, atol=2e-2)
TOL_CCE_LSE = dict(rtol=2e-3, atol=2e-3)
TOL_CCE_GRAD = dict(rtol=5e-2, atol=5e-2)
# linear_cross_entropy end to end with per-token gradient scale 1 on
# cce_case(130, 1001, 192): plain bf16 eager torch on the CPU (bf16 logits,
# fp32 softmax and filter, bf16 dlogits, bf16 GEMMs) needs atol 4.6e-4 for de
# and 1.16e-2 for dc at rtol 5e-2 against the filtered fp64 reference (max
# |de| 2.0, max |dc| 45.5). Twice that, both below the project's 5e-2.
TOL_CCE_DE_UNIT = dict(rtol=5e-2, atol=9.2e-4)
TOL_CCE_DC_UNIT = dict(rtol=5e-2, atol=2.32e-2)
TOL_ATTN_OUT = dict(rtol=3e-2, atol=3e-2)
TOL_ATTN_LSE = dict(rtol=1e-2, atol=1e-2)
TOL_ATTN_GRAD = dict(rtol=5e-2, atol=5e-2)
# dq = scale * dS @ k is linear in k, and the project's 5e-2 is stated for
# k ~ N(0,1). The planted keys (attn_case) have a per-component std of 2.1 at
# D = 64 (1.5 at D = 128, 4.4 at D = 16) and |k| = 16 instead of sqrt(D), so
# the absolute error of dq scales by that factor: twice the project's atol,
# at every D. dk, dv and dsinks keep 5e-2 with dout ~ N(0,1).
# (The issue's other route, twice the error of plain bf16 eager torch on the
# CPU, would allow far more: bf16 eager needs an atol of 1.18 for dq, 0.34
# for dk and 0.14 for dv on these cases, because it rounds logits of 15.)
TOL_ATTN_DQ = dict(rtol=5e-2, atol=1e-1)
TOL_FP32 = dict(rtol=1e-4, atol=1e-5)
# cce_dlogits_ writes bf16 from exact fp32 math on the same bf16 logits and
# fp32 lse: the only error is the final round-to-nearest (half an ulp,
# 2**-9 = 2.0e-3 relative) plus the fp32 exp (about 1e-6 relative at
# |logit - lse| <= 30). 1e-2 is five half-ulps; atol covers flushed denormals.
TOL_DLOGITS = dict(rtol=1e-2, atol=1e-6)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _close(got, ref, rtol, atol):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    return (got - ref).abs() <= atol + rtol * ref.abs()


def assert_close(got, ref, tol, what):
    ok = _close(got, ref, **tol)
    if not bool(ok.all()):
        got64 = got.detach().cpu().double()
        err = (got64 - ref.detach().cpu().double()).abs()
        bad = (~ok).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(
            f"{what}: {int((~ok).sum())}/{ok.numel()} elements out of tolerance "
            f"{tol}; max abs err {err.max().item():.4g}; first at {first}: "
            f"got {got64[first].item():.6g}, want {ref[first].item():.6g}"
        )


def assert_bitwise(got, ref, what):
    got = got.detach().cpu()
    ref = ref.detach().cpu()
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError(
            f"{what}: {bad.shape[0]} elements differ, first at {tuple(bad[0].tolist())}"
        )


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------

RMS_HEAD_SHAPES = [(1, 8), (5, 64), (67, 72), (64, 120), (130, 128), (65541, 64)]
RMS_SMALL_N = [1, 7, 60, 63, 101, 127, 129, 200, 255, 257, 500, 511, 512]
RMS_SMALL_SHAPES = [(m, n) for n in RMS_SMALL_N for m in (3, 37)] + [(8200, 60)]
RMS_LDS_SHAPES = [(5, 513), (5, 520), (5, 1027), (2100, 520)]
RMS_EPS = 1e-6


def rms_case(M, N, seed=0):
    """bf16 x, w, dy with |x| = 32 planted in column N-1 and in the first
    column of the scalar tail, 8*(N//8); w and dy carry other large values on
    the same columns."""
    g = _gen(1000 + seed)
    x = torch.randn(M, N, generator=g)
    w = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    cols = sorted({N - 1, 8 * (N // 8)} - {N})
    sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)
    for c in cols:
        x[:, c] = 32.0 * sign
        w[c] = 4.0
        dy[:, c] = -8.0
    return x.to(BF16), w.to(BF16), dy.to(BF16)


def rms_ref(x, w, dy, zero_centered, eps=RMS_EPS):
    x64 = x.detach().cpu().double().requires_grad_(True)
    w64 = w.detach().cpu().double().requires_grad_(True)
    inv = torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps)
    y = x64 * inv * (w64 + (1.0 if zero_centered else 0.0))
    y.backward(dy.detach().cpu().double())
    return y.detach(), inv.detach().squeeze(-1), x64.grad, w64.grad


def check_rms(run, M, N, zero_centered):
    """run(x, w, dy, zero_centered) -> (y, inv_rms, dx, dw)."""
    x, w, dy = rms_case(M, N)
    y, inv, dx, dw = run(x, w, dy, zero_centered)
    ry, rinv, rdx, rdw = rms_ref(x, w, dy, zero_centered)
    assert_close(inv, rinv, TOL_FP32, "inv_rms")
    assert_close(y, ry, TOL_RMS_Y, "y")
    assert_close(dx, rdx, TOL_RMS_DX, "dx")
    assert_close(dw, rdw, TOL_RMS_DW, "dw")


# ---------------------------------------------------------------------------
# Fused linear + cross-entropy
# ---------------------------------------------------------------------------

CCE_FWD_SHAPES = [
    (1, 40, 64), (63, 127, 64), (64, 128, 192), (65, 129, 576),
    (130, 1000, 320), (70, 333, 1024), (33, 257, 128),
]


def cce_planted_columns(V):
    """The columns that take the dominant logit in turn: tile edges of the
    128-wide vocab tile and its 64-wide halves, the last column, the first
    column of the padded last tile, one column used as a target and one that
    never is a target."""
    tgt_col = max(V - 2, 0)
    non_tgt_col = V // 3
    cand = [0, 63, 64, 127, 128, V - 1, 128 * (V // 128), tgt_col, non_tgt_col]
    cols = []
    for c in cand:
        if 0 <= c < V and c not in cols:
            cols.append(c)
    return cols, tgt_col, non_tgt_col


def cce_case(T, V, K, seed=0):
    """bf16 e (T, K), c (V, K) and int64 targets. Row r belongs to group
    g = r % len(cols); e[r, g] = 4 and c[cols[g], g] = 2, so logit
    (r, cols[g]) is 8 above a background of std ~1 (|logit| <= 12)."""
    g = _gen(2000 + seed)
    cols, tgt_col, non_tgt_col = cce_planted_columns(V)
    e = torch.randn(T, K, generator=g) * 0.5
    c = torch.randn(V, K, generator=g) * (0.5 / math.sqrt(K))
    targets = torch.randint(0, V, (T,), generator=g)
    group = torch.arange(T) % len(cols)
    for gi, col in enumerate(cols):
        e[group == gi, gi] = 4.0
        c[col, gi] = 2.0
    last_tile_col = min(128 * (V // 128), V - 1)
    for r in range(T):
        col = cols[int(group[r])]
        if col == tgt_col:
            targets[r] = tgt_col
        elif targets[r] == non_tgt_col:
            targets[r] = (non_tgt_col + 1) % V
    # special targets on the first rows that are free to take them
    free = [r for r in range(T) if cols[int(group[r])] != tgt_col]
    special = [s for s in (V - 1, last_tile_col, IGNORE, 0) if s != non_tgt_col]
    for r, s in zip(free, special):
        targets[r] = s
    return e.to(BF16), c.to(BF16), targets


def cce_fwd_ref(e, c, targets):
    """(lse, target logit) in fp64; target logit 0 at ignored rows."""
    logits = e.detach().cpu().double() @ c.detach().cpu().double().t()
    lse = torch.logsumexp(logits, -1)
    t = targets.detach().cpu()
    valid = t != IGNORE
    tl = logits.gather(1, t.clamp(min=0).unsqueeze(1)).squeeze(1)
    return lse, torch.where(valid, tl, torch.zeros_like(tl)), logits


def check_cce_fwd(run, T, V, K):
    """run(e, c, targets, vocab_start) -> (lse, tgt_logit) of the shard."""
    e, c, targets = cce_case(T, V, K)
    lse, tl = run(e, c, targets, 0)
    rlse, rtl, logits = cce_fwd_ref(e, c, targets)
    # the case must do what it says: the planted column dominates every row
    top = logits.max(-1).values
    assert float((rlse - top).abs().max()) < 0.7
    assert float(logits.abs().max()) <= 12.5
    assert_close(lse, rlse, TOL_CCE_LSE, "lse")
    assert_close(tl, rtl, TOL_CCE_LSE, "target logit")


def check_cce_rounded_lse(run, T, V, K):
    """run(e, c, targets) -> lse of the logits rounded to bf16, the one the
    backward pairs with its bf16 logits buffer. A logit that sits on a bf16
    rounding tie can round either way from an fp32 accumulator (summation
    order moves it by about 0.003 bf16 ulp at K = 1024), so rows that hold a
    logit within 0.01 ulp of a tie whose flip would move the lse by more than
    a quarter of the tolerance are left out: at most 10% of the rows."""
    e, c, targets = cce_case(T, V, K)
    got = run(e, c, targets)
    _, _, z = cce_fwd_ref(e, c, targets)
    zb = z.float().to(BF16).double()
    rlse = torch.logsumexp(zb, -1)
    ulp = torch.exp2(torch.floor(torch.log2(z.abs().clamp_min(1e-30))) - 7)
    near_tie = ((z - zb).abs() / ulp - 0.5).abs() < 0.01
    weight = torch.exp(zb - rlse.unsqueeze(1)) * ulp
    keep = ~(near_tie & (weight > TOL_CCE_LSE["atol"] / 4)).any(-1)
    assert int(keep.sum()) >= 0.9 * T
    assert_close(got.cpu()[keep], rlse[keep], TOL_CCE_LSE, "rounded lse")
    # and it differs from the fp32 lse by more than that tolerance somewhere,
    # so the check above cannot be met by returning the fp32 lse
    assert float((rlse - torch.logsumexp(z, -1)).abs().max()) > 4 * TOL_CCE_LSE["atol"]


CCE_SHARDS = [(0, 100), (100, 257), (257, 1000)]


def check_cce_vocab_parallel(run):
    """Three shards of a V=1000 classifier, merged like the vocab-parallel
    all-reduce: lse by logsumexp, target logit by sum."""
    T, V, K = 130, 1000, 320
    e, c, targets = cce_case(T, V, K)
    for lo, hi in CCE_SHARDS:  # targets below, inside and above each shard
        valid = targets[targets != IGNORE]
        assert bool((valid >= lo).logical_and(valid < hi).any())
    lses, tls = [], []
    for lo, hi in CCE_SHARDS:
        lse, tl = run(e, c[lo:hi].contiguous(), targets, lo)
        lses.append(lse.detach().cpu().double())
        tls.append(tl.detach().cpu().double())
    lse = torch.logsumexp(torch.stack(lses), 0)
    tl = torch.stack(tls).sum(0)
    rlse, rtl, _ = cce_fwd_ref(e, c, targets)
    assert_close(lse, rlse, TOL_CCE_LSE, "merged lse")
    assert_close(tl, rtl, TOL_CCE_LSE, "merged target logit")


CCE_DLOGITS_SHAPES = [
    (3, 7), (5, 8), (4, 1001), (6, 4099), (2, 128 * 2048 + 13), (4200, 40),
]
CCE_FILTER_EPS = [0.0, 2.0 ** -12, 0.05]


def cce_dlogits_case(R, V, vocab_start, with_dlse, seed=0):
    """bf16 logits of one vocab shard with fp32 lse/dl/dlse and GLOBAL
    targets: in-shard (including the last column and the first tail column),
    below and above the shard, ignored rows (dl = 0) and dl == 0 rows."""
    g = _gen(3000 + seed)
    logits = (torch.randn(R, V, generator=g) * 2.0)
    logits[:, V - 1] = 5.0                      # last (tail) column is the mode
    logits[0::2, 8 * ((V - 1) // 8)] = 4.0      # first column of the tail group
    if R > 1:  # row 1's target: 0.01 < p < 0.05, so only eps = 0.05 is above it
        logits[1, 8 * ((V - 1) // 8)] = 2.0
    logits = logits.to(BF16)
    # the row's lse over the FULL vocab: other shards add mass when sharded
    lse = torch.logsumexp(logits.double(), -1)
    if vocab_start:
        lse = lse + math.log(2.0)
    lse = lse.float()
    local = torch.randint(0, V, (R,), generator=g)
    local[0] = V - 1
    if R > 1:
        local[1] = 8 * ((V - 1) // 8)
    targets = local + vocab_start
    dl = torch.rand(R, generator=g) + 0.5
    if R > 2:
        targets[2] = IGNORE
        dl[2] = 0.0
    if R > 3:
        dl[3] = 0.0
    if R > 4:
        targets[4] = vocab_start + V           # first id above the shard
    if R > 5 and vocab_start:
        targets[5] = vocab_start - 1           # last id below the shard
    dlse = (torch.randn(R, generator=g) * 0.5) if with_dlse else None
    return logits, lse, targets, dl, dlse


def cce_dlogits_ref(logits, lse, targets, dl, dlse, vocab_start, eps):
    """Documented rule: p = exp(logit - lse); zero p where p < eps and the
    column is not the target; out = p * (dl + dlse) - onehot(target) * dl.
    Returns (filtered, unfiltered, ambiguous) where `ambiguous` marks the
    elements whose p is within 1e-4 relative of eps."""
    z = logits.detach().cpu().double()
    R, V = z.shape
    p = torch.exp(z - lse.detach().cpu().double().unsqueeze(1))
    t = targets.detach().cpu()
    local = torch.where(t == IGNORE, torch.full_like(t, -1), t - vocab_start)
    is_tgt = torch.arange(V).unsqueeze(0) == local.unsqueeze(1)
    g = dl.detach().cpu().double().unsqueeze(1)
    gp = g + (dlse.detach().cpu().double().unsqueeze(1) if dlse is not None else 0.0)
    onehot = is_tgt.double() * g
    unfiltered = p * gp - onehot
    if eps > 0:
        pf = torch.where((p < eps) & ~is_tgt, torch.zeros_like(p), p)
        ambiguous = ((p / eps - 1.0).abs() < 1e-4) & ~is_tgt
    else:
        pf = p
        ambiguous = torch.zeros_like(is_tgt)
    return pf * gp - onehot, unfiltered, ambiguous


def check_cce_dlogits(run, R, V, vocab_start, with_dlse, eps):
    """run(logits, lse, targets, dl, dlse, vocab_start, eps) -> dlogits bf16
    (R, V); `logits` may be consumed in place."""
    logits, lse, targets, dl, dlse = cce_dlogits_case(R, V, vocab_start, with_dlse)
    ref, ref_unf, amb = cce_dlogits_ref(logits, lse, targets, dl, dlse, vocab_start, eps)
    assert int(amb.sum()) <= 1e-3 * amb.numel(), "too many elements at the threshold"
    if eps > 0:  # the filter must decide something in this case
        assert bool((ref != ref_unf).any())
    got = run(logits.clone(), lse, targets, dl, dlse, vocab_start, eps)
    assert got.dtype == BF16
    ok = _close(got, ref, **TOL_DLOGITS) | (amb & _close(got, ref_unf, **TOL_DLOGITS))
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(
            f"dlogits: {bad.shape[0]}/{ok.numel()} elements wrong, first at {i}: "
            f"got {float(got[i])}, want {float(ref[i])}"
        )


def cce_e2e_ref(e, c, targets, eps):
    """loss (mean over valid tokens), de, dc of the filtered backward."""
    e64 = e.detach().cpu().double()
    c64 = c.detach().cpu().double()
    t = targets.detach().cpu()
    logits = e64 @ c64.t()
    lse = torch.logsumexp(logits, -1)
    valid = t != IGNORE
    n = int(valid.sum())
    nll = lse - logits.gather(1, t.clamp(min=0).unsqueeze(1)).squeeze(1)
    loss = torch.where(valid, nll, torch.zeros_like(nll)).sum() / n
    dl = valid.double() / n
    p = torch.exp(logits - lse.unsqueeze(1))
    is_tgt = torch.arange(logits.shape[1]).unsqueeze(0) == t.unsqueeze(1)
    if eps > 0:
        p = torch.where((p < eps) & ~is_tgt, torch.zeros_like(p), p)
    dz = (p - is_tgt.double()) * dl.unsqueeze(1)
    return loss, dz @ c64, dz.t() @ e64


# ---------------------------------------------------------------------------
# Router
# ---------------------------------------------------------------------------

ROUTER_SHAPES = [
    (5, 8, 2), (64, 64, 1), (130, 65, 8), (33, 16, 16), (64, 1024, 16),
    (257, 100, 4), (3, 2, 2),
]
ROUTER_BIAS = ["none", "small", "decisive"]


def router_case(T, E, K, bias_kind, seed=123):
    """fp32 N(0,1) logits with the winning expert planted on
    {0, 63, 64, 65, E-1} in turn; upstream grad for the top-k probs."""
    g = _gen(seed)
    logits = torch.randn(T, E, generator=g)
    winners = [c for c in (0, 63, 64, 65, E - 1) if c < E]
    w = torch.tensor([winners[r % len(winners)] for r in range(T)])
    logits[torch.arange(T), w] = 4.0 + 0.25 * torch.rand(T, generator=g)
    dtop = torch.randn(T, K, generator=g)
    if bias_kind == "none":
        bias = None
    elif bias_kind == "small":
        bias = torch.randn(E, generator=g) * 0.01
    else:
        bias = torch.zeros(E)
        bias[torch.tensor(sorted({1 % E, E // 2, max(E - 2, 0)}))] = 0.5
    return logits, bias, dtop, w


def router_ref(logits, bias, K, renorm, dtop=None):
    """fp64 softmax; selection on probs + bias, ties to the lower index
    (stable descending sort); returned probs are bias-free, renormalised over
    the selection. Also `keep`: the rows whose top-(K+1) scores are pairwise
    separated by at least 64 fp32 ulps, i.e. whose selection AND order an
    fp32 implementation must reproduce exactly."""
    z = logits.detach().cpu().double().requires_grad_(True)
    p = torch.softmax(z, -1)
    score = p.detach() + (bias.detach().cpu().double() if bias is not None else 0.0)
    sorted_score, order = torch.sort(score, dim=-1, descending=True, stable=True)
    idx = order[:, :K]
    top = p.gather(-1, idx)
    if renorm:
        top = top / top.sum(-1, keepdim=True).clamp_min(1e-20)
    E = z.shape[1]
    head = sorted_score[:, : min(K + 1, E)]
    # A score p_j + bias_j carries an fp32 error of a few ulps of ITSELF (the
    # softmax denominator's error is common to the row and cannot reorder
    # it), so each adjacent pair is held against 64 ulps of the larger score
    # of the pair.
    if head.shape[1] > 1:
        gap = head[:, :-1] - head[:, 1:]
        scale = torch.maximum(head[:, :-1].abs(), head[:, 1:].abs())
        keep = (gap >= 64 * 2.0 ** -23 * scale).all(-1)
    else:
        keep = torch.ones(z.shape[0], dtype=torch.bool)
    dz = None
    if dtop is not None:
        top.backward(dtop.detach().cpu().double())
        dz = z.grad
    return top.detach(), idx, keep, dz


def check_router(run, T, E, K, bias_kind, renorm):
    """run(logits, bias, K, renorm, dtop) -> (top_probs, indices, dlogits)."""
    logits, bias, dtop, w = router_case(T, E, K, bias_kind)
    rtop, ridx, keep, rdz = router_ref(logits, bias, K, renorm, dtop)
    assert int((~keep).sum()) <= 0.02 * T, f"{int((~keep).sum())} of {T} rows near-tied"
    if bias_kind == "none":  # the planted winner is every row's first pick
        assert bool((ridx[:, 0] == w).all())
    elif bias_kind == "decisive":  # the bias must change the selection on most rows
        _, plain, _, _ = router_ref(logits, None, K, renorm)
        if K < E:
            changed = (plain.sort(-1).values != ridx.sort(-1).values).any(-1)
            assert float(changed.double().mean()) > 0.5
    top, idx, dz = run(logits, bias, K, renorm, dtop)
    assert idx.dtype == torch.int64
    assert_bitwise(idx.cpu()[keep], ridx[keep], "router indices on decided rows")
    assert_close(top.cpu()[keep], rtop[keep], TOL_FP32, "top probs")
    assert_close(dz.cpu()[keep], rdz[keep], TOL_FP32, "dlogits")


def router_tie_case():
    """(logits, K, expected indices): all-equal rows and duplicated top
    values. The rule (moe_router.hip): lower expert index first among equals."""
    E, K = 70, 4
    logits = torch.zeros(4, E)
    want = torch.zeros(4, K, dtype=torch.int64)
    want[0] = torch.tensor([0, 1, 2, 3])                      # all equal
    logits[1, [3, 64, 65, 69]] = 2.0                          # four tied winners
    want[1] = torch.tensor([3, 64, 65, 69])
    logits[2, 66] = 3.0                                       # one winner, rest tied
    want[2] = torch.tensor([66, 0, 1, 2])
    logits[3, [5, 63]] = 2.0                                  # two tied, then a
    logits[3, 10] = 1.0                                       # clear third, then ties
    want[3] = torch.tensor([5, 63, 10, 0])
    return logits, K, want


# ---------------------------------------------------------------------------
# MoE permute / combine
# ---------------------------------------------------------------------------

MOE_SHAPES = [(1, 8, 4, 1), (37, 4, 8, 2), (64, 100, 16, 4), (130, 520, 6, 3), (50, 1037, 128, 8)]


def moe_case(T, H, E, K, one_expert=False, seed=0):
    """Token row t is the constant t (exact in bf16 for t <= 256); expert
    output row r is a function of r; the routing leaves about half of the experts
    without tokens (`one_expert` sends every replica to expert E-1)."""
    g = _gen(4000 + seed)
    n_allowed = max(K, E // 2)
    allowed = torch.randperm(E, generator=g)[:n_allowed]
    if one_expert:
        indices = torch.full((T, K), E - 1, dtype=torch.int64)
    else:
        indices = torch.stack(
            [allowed[torch.randperm(n_allowed, generator=g)[:K]] for _ in range(T)]
        )
    tokens = torch.arange(T, dtype=torch.float32).unsqueeze(1).expand(T, H).contiguous()
    probs = torch.rand(T, K, generator=g) + 0.1
    probs = probs / probs.sum(-1, keepdim=True)
    R = T * K
    r = torch.arange(R).unsqueeze(1)
    h = torch.arange(H).unsqueeze(0)
    expert_out = ((r * 7 + h * 3) % 31 - 15).float() / 16.0   # exact in bf16
    grad_rows = torch.randn(R, H, generator=g)
    grad_out = torch.randn(T, H, generator=g) * 0.25
    return dict(
        tokens=tokens.to(BF16), indices=indices, probs=probs,
        expert_out=expert_out.to(BF16), grad_rows=grad_rows.to(BF16),
        grad_out=grad_out.to(BF16), E=E,
    )


def moe_permute_ref(indices, E):
    """Python-loop reference: flat replica ids sorted by expert, stable."""
    T, K = indices.shape
    flat = indices.reshape(-1).tolist()
    order, counts = [], []
    for e in range(E):
        rows = [i for i, x in enumerate(flat) if x == e]
        order.extend(rows)
        counts.append(len(rows))
    order = torch.tensor(order, dtype=torch.int64)
    return order, order // K, torch.tensor(counts, dtype=torch.int64)


def check_moe_permute(run, T, H, E, K, one_expert=False, dtype=BF16):
    """run(tokens, indices, probs, E, grad_rows) ->
    (permuted_tokens, permuted_probs, tokens_per_expert, d_tokens)."""
    case = moe_case(T, H, E, K, one_expert)
    tokens = case["tokens"].to(dtype)
    grad_rows = case["grad_rows"].to(dtype)
    order, row_to_token, counts = moe_permute_ref(case["indices"], E)
    assert int((counts == 0).sum()) >= min(E - 1, 2), "case must leave experts empty"
    perm, pprobs, tpe, d_tokens = run(tokens, case["indices"], case["probs"], E, grad_rows)
    assert_bitwise(perm, tokens[row_to_token], "permuted_tokens")
    assert_bitwise(pprobs, case["probs"].reshape(-1)[order], "permuted_probs")
    assert_bitwise(tpe, counts, "tokens_per_expert")
    ref_d = torch.zeros(T, H, dtype=torch.float64).index_add_(
        0, row_to_token, grad_rows.double()
    )
    assert_close(d_tokens, ref_d, TOL_COMBINE, "d tokens")


def moe_unpermute_ref(expert_out, pprobs, row_to_token, T, grad_out):
    eo = expert_out.detach().cpu().double().requires_grad_(True)
    pp = pprobs.detach().cpu().double().requires_grad_(True)
    out = torch.zeros(T, eo.shape[1], dtype=torch.float64).index_add(
        0, row_to_token, eo * pp.unsqueeze(1)
    )
    out.backward(grad_out.detach().cpu().double())
    return out.detach(), eo.grad, pp.grad


def check_moe_unpermute(run, T, H, E, K, one_expert=False):
    """run(tokens, indices, probs, E, expert_out, grad_out) ->
    (out, d_expert_out, d_permuted_probs) with expert_out and the permuted
    probs as autograd leaves."""
    case = moe_case(T, H, E, K, one_expert)
    order, row_to_token, _ = moe_permute_ref(case["indices"], E)
    pprobs = case["probs"].reshape(-1)[order]
    out, d_eo, d_pp = run(
        case["tokens"], case["indices"], case["probs"], E, case["expert_out"],
        case["grad_out"],
    )
    rout, rd_eo, rd_pp = moe_unpermute_ref(
        case["expert_out"], pprobs, row_to_token, T, case["grad_out"]
    )
    assert_close(out, rout, TOL_COMBINE, "unpermute out")
    assert_close(d_eo, rd_eo, TOL_COMBINE, "d expert_out")
    assert_close(d_pp, rd_pp, TOL_FP32, "d probs")


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------

ROPE_SHAPES = [
    (1, 3, 1, 1, 4, 4), (2, 17, 3, 1, 36, 32), (1, 64, 4, 2, 128, 64),
    (2, 33, 2, 2, 64, 64), (1, 2049, 16, 4, 64, 64),
]


def rope_case(B, S, Hq, Hkv, D, rope_dim, expanded=False, seed=0):
    """bf16 q/k and their upstream grads with +-4 planted on the last rotated
    dim, the first pass-through dim and the last dim; fp32 cos/sin
    (B, S, rope_dim) with duplicated halves, optionally one (1, S, rope_dim)
    table expanded over the batch (not contiguous)."""
    g = _gen(5000 + seed)
    half = rope_dim // 2

    def planted(*shape):
        t = torch.randn(*shape, generator=g)
        for d in {half - 1, half, rope_dim - 1, min(rope_dim, D - 1), D - 1}:
            t[..., d] = torch.where(torch.arange(shape[1]) % 2 == 0, 4.0, -4.0).view(1, -1, 1)
        return t.to(BF16)

    q, gq = planted(B, S, Hq, D), planted(B, S, Hq, D)
    k, gk = planted(B, S, Hkv, D), planted(B, S, Hkv, D)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(half, dtype=torch.float64) * 2 / rope_dim))
    if expanded:
        pos = torch.arange(S, dtype=torch.float64).view(1, S)
    else:  # a different position offset per batch row
        pos = torch.arange(S, dtype=torch.float64).view(1, S) + 7.0 * torch.arange(B).view(B, 1)
    ang = pos.unsqueeze(-1) * inv_freq
    ang = torch.cat([ang, ang], -1)
    cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    if expanded:
        cos, sin = cos.expand(B, S, rope_dim), sin.expand(B, S, rope_dim)
        assert B > 1 and not cos.is_contiguous()
    return q, k, cos, sin, gq, gk


def rope_ref(x, cos, sin, gx):
    x64 = x.detach().cpu().double().requires_grad_(True)
    c = cos.detach().cpu().double().unsqueeze(-2)
    s = sin.detach().cpu().double().unsqueeze(-2)
    rd = c.shape[-1]
    xr, xp = x64[..., :rd], x64[..., rd:]
    rot = torch.cat([-xr[..., rd // 2:], xr[..., : rd // 2]], -1)
    out = torch.cat([xr * c + rot * s, xp], -1)
    out.backward(gx.detach().cpu().double())
    return out.detach(), x64.grad


def check_rope(run, B, S, Hq, Hkv, D, rope_dim, expanded=False):
    """run(q, k, cos, sin, gq, gk) -> (q_out, k_out, dq, dk)."""
    q, k, cos, sin, gq, gk = rope_case(B, S, Hq, Hkv, D, rope_dim, expanded)
    got = run(q, k, cos, sin, gq, gk)
    rq, rdq = rope_ref(q, cos, sin, gq)
    rk, rdk = rope_ref(k, cos, sin, gk)
    for name, g, r in zip(("q_out", "k_out", "dq", "dk"), got, (rq, rk, rdq, rdk)):
        assert_close(g, r, TOL_ROPE, name)
    if rope_dim < D:  # pass-through dims are copied, bit for bit
        for name, g, src in zip(("q_out", "k_out", "dq", "dk"), got, (q, k, gq, gk)):
            assert_bitwise(
                g[..., rope_dim:].to(src.dtype), src[..., rope_dim:], name + " pass-through"
            )


# ---------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------


def attn_mask(Sq, Skv, causal, window_left, off):
    """True where key j is hidden from query i (global position i + off)."""
    qpos = torch.arange(Sq).unsqueeze(1) + off
    kpos = torch.arange(Skv).unsqueeze(0)
    mask = torch.zeros(Sq, Skv, dtype=torch.bool)
    if causal:
        mask |= kpos > qpos
    if window_left >= 0:
        mask |= kpos < qpos - window_left
    return mask


def attn_fwd64(q, k, v, causal, scale, window_left, sinks, off):
    """Textbook attention on fp64 (B, S, H, D) tensors -> out (B,Sq,Hq,D),
    lse (B,Hq,Sq). A sink is one extra logit per head in the denominator."""
    B, Sq, Hq, D = q.shape
    Skv, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    qh = q.permute(0, 2, 1, 3)
    kh = k.permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    vh = v.permute(0, 2, 1, 3).repeat_interleave(rep, 1)
    s = qh @ kh.transpose(-1, -2) * scale
    s = s.masked_fill(attn_mask(Sq, Skv, causal, window_left, off), float("-inf"))
    if sinks is not None:
        full = torch.cat([s, sinks.view(1, Hq, 1, 1).expand(B, Hq, Sq, 1)], -1)
        lse = torch.logsumexp(full, -1)
    else:
        lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse.unsqueeze(-1))
    return (p @ vh).permute(0, 2, 1, 3), lse


def _plant_keys(q, k, scale, causal, window_left, off):
    """Add to k[j] a component along q[i] worth a logit of 10 for the pairs
    (i, j) the case targets. Every pairing is one-to-one, so a key carries at
    most four such components and the logits stay near +-15.
    Inside the mask: the causal diagonal j = i + off (which walks over every
    64/128 tile edge and ends on Skv-1) and, with a window, on odd rows the
    first in-window key j = i + off - window_left; non-causal rows pair with
    j = Skv-1-i. Outside the mask, always: the key one past the diagonal and
    the key one before the window."""
    Sq, Hq, D = q.shape
    Skv, Hkv, _ = k.shape
    rep = Hq // Hkv
    qg = q.view(Sq, Hkv, rep, D)[:, :, 0]            # heads of a group share q
    unit = qg / (qg.pow(2).sum(-1, keepdim=True) * scale) * 10.0
    for i in range(Sq):
        pos = i + off
        if causal:
            inside = min(pos, Skv - 1)
            if window_left >= 0 and i % 2 == 1 and pos - window_left >= 0:
                inside = pos - window_left
        else:
            inside = (Skv - 1 - i) % Skv
            if window_left >= 0:
                inside = max(pos - window_left, 0)
        targets = [inside]
        if causal and pos + 1 < Skv:
            targets.append(pos + 1)                  # one past the diagonal
        if window_left >= 0 and pos - window_left - 1 >= 0:
            targets.append(pos - window_left - 1)    # one before the window
        for j in targets:
            k[j] += unit[i]


def attn_case(B, Sq, Skv, Hq, Hkv, D, causal=True, window_left=-1, q_offset=0,
              with_sinks=False, seed=0):
    """bf16 q, k, v, dout (B, S, H, D), fp32 dlse and sinks, with planted
    keys (see _plant_keys). Query heads of one GQA group share their vectors
    up to sign so that a kv head can be aligned with all of them."""
    g = _gen(6000 + seed)
    scale = 1.0 / math.sqrt(D)
    rep = Hq // Hkv
    qg = torch.randn(B, Sq, Hkv, 1, D, generator=g)
    q = qg.expand(B, Sq, Hkv, rep, D).reshape(B, Sq, Hq, D).clone()
    k = torch.randn(B, Skv, Hkv, D, generator=g) * 0.3
    v = torch.randn(B, Skv, Hkv, D, generator=g)
    for b in range(B):
        _plant_keys(q[b], k[b], scale, causal, window_left, q_offset)
    dout = torch.randn(B, Sq, Hq, D, generator=g)
    dlse = torch.randn(B, Hq, Sq, generator=g)
    sinks = (8.0 + torch.randn(Hq, generator=g)) if with_sinks else None
    return dict(
        q=q.to(BF16), k=k.to(BF16), v=v.to(BF16), dout=dout.to(BF16), dlse=dlse,
        sinks=sinks, causal=causal, scale=scale, window_left=window_left,
        q_offset=q_offset,
    )


def attn_ref(case, use_dlse=False):
    """fp64 out, lse and grads (dq, dk, dv, dsinks) of
    loss = (out*dout).sum() [+ (lse*dlse).sum()]."""
    q, k, v = (case[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    sinks = case["sinks"].double().requires_grad_(True) if case["sinks"] is not None else None
    out, lse = attn_fwd64(
        q, k, v, case["causal"], case["scale"], case["window_left"], sinks,
        case["q_offset"],
    )
    loss = (out * case["dout"].double()).sum()
    if use_dlse:
        loss = loss + (lse * case["dlse"].double()).sum()
    loss.backward()
    return dict(
        out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad,
        dsinks=sinks.grad if sinks is not None else None,
    )


def check_attn(run, case, use_dlse=False, backward=True):
    """run(case, use_dlse, backward) -> dict with out, lse and, when
    `backward`, dq, dk, dv (and dsinks when the case has sinks)."""
    ref = attn_ref(case, use_dlse)
    got = run(case, use_dlse, backward)
    assert_close(got["out"], ref["out"], TOL_ATTN_OUT, "out")
    assert_close(got["lse"], ref["lse"], TOL_ATTN_LSE, "lse")
    if backward:
        assert_close(got["dq"], ref["dq"], TOL_ATTN_DQ, "dq")
        for n in ("dk", "dv"):
            assert_close(got[n], ref[n], TOL_ATTN_GRAD, n)
        if case["sinks"] is not None:
            assert_close(got["dsinks"], ref["dsinks"], TOL_ATTN_GRAD, "dsinks")


def attn_varlen_case(lens_q, lens_k, Hq, Hkv, D, causal=True, window_left=-1,
                     with_sinks=False, seed=0):
    """Packed (total, H, D) tensors built from one planted dense case per
    sequence; causal masking aligns the END of q with the END of kv."""
    parts = []
    for i, (lq, lk) in enumerate(zip(lens_q, lens_k)):
        parts.append(attn_case(
            1, lq, lk, Hq, Hkv, D, causal, window_left, lk - lq, False, seed * 100 + i
        ))
    g = _gen(6500 + seed)
    cat = lambda n: torch.cat([p[n][0] for p in parts], 0)
    cu = lambda lens: torch.tensor([0] + list(lens), dtype=torch.int32).cumsum(0).to(torch.int32)
    return dict(
        q=cat("q"), k=cat("k"), v=cat("v"), dout=cat("dout"),
        dlse=torch.cat([p["dlse"][0] for p in parts], 1),
        sinks=(8.0 + torch.randn(Hq, generator=g)) if with_sinks else None,
        cu_q=cu(lens_q), cu_k=cu(lens_k), causal=causal, scale=1.0 / math.sqrt(D),
        window_left=window_left,
    )


def attn_varlen_ref(case, use_dlse=False):
    q, k, v = (case[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    sinks = case["sinks"].double().requires_grad_(True) if case["sinks"] is not None else None
    cu_q, cu_k = case["cu_q"].tolist(), case["cu_k"].tolist()
    outs, lses = [], []
    for s in range(len(cu_q) - 1):
        lq, lk = cu_q[s + 1] - cu_q[s], cu_k[s + 1] - cu_k[s]
        o, l = attn_fwd64(
            q[cu_q[s]:cu_q[s + 1]].unsqueeze(0), k[cu_k[s]:cu_k[s + 1]].unsqueeze(0),
            v[cu_k[s]:cu_k[s + 1]].unsqueeze(0), case["causal"], case["scale"],
            case["window_left"], sinks, lk - lq,
        )
        outs.append(o[0])
        lses.append(l[0])
    out, lse = torch.cat(outs, 0), torch.cat(lses, 1)     # (total,Hq,D), (Hq,total)
    loss = (out * case["dout"].double()).sum()
    if use_dlse:
        loss = loss + (lse * case["dlse"].double()).sum()
    loss.backward()
    return dict(
        out=out.detach(), lse=lse.detach(), dq=q.grad, dk=k.grad, dv=v.grad,
        dsinks=sinks.grad if sinks is not None else None,
    )


def check_attn_varlen(run, case, use_dlse=False):
    ref = attn_varlen_ref(case, use_dlse)
    got = run(case, use_dlse)
    assert_close(got["out"], ref["out"], TOL_ATTN_OUT, "out")
    assert_close(got["lse"], ref["lse"], TOL_ATTN_LSE, "lse")
    assert_close(got["dq"], ref["dq"], TOL_ATTN_DQ, "dq")
    for n in ("dk", "dv"):
        assert_close(got[n], ref[n], TOL_ATTN_GRAD, n)
    if case["sinks"] is not None:
        assert_close(got["dsinks"], ref["dsinks"], TOL_ATTN_GRAD, "dsinks")


def check_attn_plant(case):
    """The case must do what it says: on most query rows one visible key holds
    more than half of the softmax mass, and no hidden key has any."""
    q, k = case["q"].double(), case["k"].double()
    rep = q.shape[2] // k.shape[2]
    s = q.permute(0, 2, 1, 3) @ k.permute(0, 2, 1, 3).repeat_interleave(rep, 1).transpose(-1, -2)
    s = s * case["scale"]
    mask = attn_mask(q.shape[1], k.shape[1], case["causal"], case["window_left"], case["q_offset"])
    hidden_top = s.masked_fill(~mask, float("-inf")).max(-1).values
    if bool(mask.any()):  # the decoys are as strong as the planted visible key
        assert float(hidden_top[hidden_top.isfinite()].median()) > 6.0
    p = torch.softmax(s.masked_fill(mask, float("-inf")), -1)
    assert float((p.max(-1).values > 0.5).double().mean()) > 0.5


def tol_needed(got, ref):
    """Smallest x for which |got - ref| <= x * (1 + |ref|) holds everywhere:
    the rtol = atol = x a comparison of `got` with `ref` needs."""
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    return float(((got - ref).abs() / (1.0 + ref.abs())).max())


def _scaled(tol, tol_scale):
    return {key: val * tol_scale for key, val in tol.items()}


# ---------------------------------------------------------------------------
# GatedDeltaNet: chunk kernels and causal conv + SiLU
# ---------------------------------------------------------------------------

GDN_D = 64
GDN_CHUNK = 64
# B*H = 6 takes the Dv-split instantiation (DVT = 32, n_wg * 2 <= 384),
# B*H = 193 the full-width one (DVT = 64)
GDN_FWD_SHAPES = [(2, 3, s) for s in (1, 63, 64, 65, 130, 192)] + [
    (1, 193, s) for s in (65, 128)
]
GDN_BWD_SHAPES = [(2, 3, 128), (1, 193, 128), (2, 3, 130)]
GDN_VARLEN_LENS = [1, 64, 63, 65, 0, 130, 7]   # tests/test_gdn_varlen.py LENS
GDN_FLAG_TRIPLES = [
    (False, False, False), (True, False, False), (True, True, False), (False, True, True),
]

# out and final_state: the project's figure (tests/test_blocks_extra.py).
# gdn_chunk_emul(cast=True) needs 9.1e-3..1.15e-2 for out (0.30-0.38 of it) and
# at most 3.3e-3 for the final state on GDN_FWD_SHAPES (S > 1).
TOL_GDN_OUT = dict(rtol=3e-2, atol=3e-2)
TOL_GDN_FS = dict(rtol=3e-2, atol=3e-2)
# No project figure exists for the aux outputs and for the gradients against
# an independent oracle. Each is twice what gdn_chunk_emul(cast=True) needs
# against gdn_step_ref (tol_needed: rtol = atol = x), the largest over the
# cases the suite runs; the factor covers MFMA accumulation order, exp2 and
# the rounding points of the reverse scan, which the straight-through
# emulation does not model. r and s0 are capped at the project's 3e-2.
#   r     : 9.97e-4 on GDN_FWD_SHAPES (max |r| 1.75; 1e-6 where S <= 64)
#   s0    : 3.413e-3 on GDN_FWD_SHAPES (max |s0| 0.34)
#   dq    : 1.859e-2  dk: 2.375e-2  dv: 2.025e-2  dbeta: 4.937e-2  dg: 9.349e-2
#           on GDN_BWD_SHAPES and GDN_VARLEN_LENS (max |dq| 7, |dk| 11,
#           |dv| 5, |dbeta| 135, |dg| 5); of these 2.5e-3..3.3e-3 is the bf16
#           rounding of dq, dk, dv themselves
#   drhs  : 1.143e-2 on gdn_case(2, 3, 100, zero_beta=False) (max |drhs| 4.1)
#   dS0   : 2.631e-3 on the same case (max |dS0| 1.5)
TOL_GDN_R = dict(rtol=2.0e-3, atol=2.0e-3)
TOL_GDN_S0 = dict(rtol=6.83e-3, atol=6.83e-3)
TOL_GDN_GRAD = dict(
    dq=dict(rtol=3.72e-2, atol=3.72e-2),
    dk=dict(rtol=4.75e-2, atol=4.75e-2),
    dv=dict(rtol=4.05e-2, atol=4.05e-2),
    dbeta=dict(rtol=9.88e-2, atol=9.88e-2),
    dg=dict(rtol=1.87e-1, atol=1.87e-1),
)
TOL_GDN_DRHS = dict(rtol=2.29e-2, atol=2.29e-2)
TOL_GDN_DS0 = dict(rtol=5.27e-3, atol=5.27e-3)


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def gdn_case(B, H, S, zero_beta=True, poison_all=False, seed=0):
    """bf16 q, k, v, dout (B, H, S, 64), fp32 beta and decay_log (B, H, S).
    Unit q and k, |v| <= 0.75 elementwise (1 on the tail row), beta in [0.25, 1), g in (-0.2, 0].
    Planted:
      * rows with (t // 8) odd: the key is +-(the block's first key),
        beta = 1 and q = k, so M is +-e^{..} ~ +-1 inside the block (the
        triangular solve needs all 7 orders) and the output is v_t;
      * g = -6 on rows 8 mod 16 (the state is wiped where a repeated-key
        block starts; never on a chunk boundary, so every chunk uses the
        state it inherits at full strength), g = 0 on the other rows
        0 mod 4, beta = 0 on rows 3 mod 16 (`zero_beta`; the backward
        scan case needs beta >= 0.25 to recover drhs = dv / beta);
      * the tail row S-1 has q = k, beta = 1 and v = 1: its output is 1;
      * row 0 of every (b, h) after the first (`poison_all`: of the first
        too, for documents packed behind one another) follows the previous
        head's tail in memory and carries |k| = |v| = 8 with beta = 1/64
        (|k| = 2, beta = 1/4 without `zero_beta`), so beta |k|^2 = 1 and the
        head itself stays O(1) while an unmasked tail load of the previous
        head writes an O(1) error into its state."""
    gen = _gen(7000 + seed)
    D = GDN_D
    q = _unit(torch.randn(B, H, S, D, generator=gen)).to(BF16)
    k = _unit(torch.randn(B, H, S, D, generator=gen)).to(BF16)
    v = torch.rand(B, H, S, D, generator=gen) * 1.5 - 0.75
    beta = 0.25 + 0.75 * torch.rand(B, H, S, generator=gen)
    g = -0.2 * torch.rand(B, H, S, generator=gen)
    dout = torch.randn(B, H, S, D, generator=gen)
    big = _unit(torch.randn(B, H, D, generator=gen)) * 8.0
    t = torch.arange(S)
    g[..., t % 4 == 0] = 0.0
    g[..., t % 16 == 8] = -6.0
    if zero_beta:
        beta[..., t % 16 == 3] = 0.0
    rep = (t // 8) % 2 == 1
    sign = torch.where(t % 2 == 0, 1.0, -1.0).view(1, 1, S, 1).to(BF16)
    k = torch.where(rep.view(1, 1, S, 1), k[:, :, (t // 8) * 8] * sign, k)
    q = torch.where(rep.view(1, 1, S, 1), k, q)
    beta[..., rep] = 1.0
    q[:, :, S - 1] = k[:, :, S - 1]
    beta[:, :, S - 1] = 1.0
    v[:, :, S - 1] = 1.0
    kmul, b0 = (8.0, 1.0 / 64) if zero_beta else (2.0, 0.25)
    poison = torch.ones(B * H, dtype=torch.bool)
    poison[0] = poison_all
    poison = poison.view(B, H)
    k[:, :, 0] = torch.where(poison.unsqueeze(-1), k[:, :, 0] * kmul, k[:, :, 0])
    v[:, :, 0] = torch.where(poison.unsqueeze(-1), big, v[:, :, 0])
    beta[:, :, 0] = torch.where(poison, torch.full_like(beta[:, :, 0], b0), beta[:, :, 0])
    return dict(q=q, k=k, v=v.to(BF16), beta=beta, g=g, dout=dout.to(BF16),
                rep=rep, poison=poison)


def _gdn_step_block(q, k, v, beta, g, dout):
    """One block of heads, (n, S, D) fp64: the per-timestep recurrence
        S_t = e^{g_t} S_{t-1} + k_t r_t^T,
        r_t = beta_t (v_t - (e^{g_t} S_{t-1})^T k_t),   o_t = S_t^T q_t
    and, with `dout`, torch.autograd of sum(out * dout)."""
    need = dout is not None
    if need:
        q, k, v, beta, g = (x.clone().requires_grad_(True) for x in (q, k, v, beta, g))
    n, S, D = q.shape
    state = torch.zeros(n, D, D, dtype=torch.float64, requires_grad=need)
    bounds, outs, rs = [], [], []
    for t in range(S):
        if t % GDN_CHUNK == 0:
            if need and t > 0:
                # a node of its own: the state also feeds output row t-1,
                # which is not part of the gradient of the state handed on
                state = state.clone()
                state.retain_grad()
            bounds.append(state)
        state = state * torch.exp(g[:, t]).view(n, 1, 1)
        pred = torch.einsum("nk,nkv->nv", k[:, t], state)
        r = beta[:, t, None] * (v[:, t] - pred)
        state = state + k[:, t, :, None] * r[:, None, :]
        outs.append(torch.einsum("nk,nkv->nv", q[:, t], state))
        rs.append(r)
    out, r = torch.stack(outs, 1), torch.stack(rs, 1)
    res = dict(out=out.detach(), r=r.detach(), fs=state.detach(),
               s0=torch.stack([b.detach() for b in bounds], 1))
    if need:
        (out * dout).sum().backward()
        res.update(dq=q.grad, dk=k.grad, dv=v.grad, dbeta=beta.grad, dg=g.grad,
                   ds0=torch.stack([b.grad for b in bounds], 1))
    return res


def _gdn_flat(case, dtype):
    n = case["q"].shape[0] * case["q"].shape[1]
    return [case[x].detach().cpu().to(dtype).reshape(n, *case[x].shape[2:])
            for x in ("q", "k", "v", "beta", "g", "dout")]


def _gdn_unflat(res, B, H):
    return {name: t.reshape(B, H, *t.shape[1:]) for name, t in res.items()}


def gdn_step_ref(case, backward=False, head_block=40):
    """fp64 reference on the bf16 inputs: out, the write vectors r (the
    kernel's `r` aux rows), the state at every 64-row boundary `s0`
    (B, H, nc, D, D), the final state `fs` and, with `backward`, dq, dk, dv,
    dbeta, dg and `ds0`, the gradient of each retained boundary state."""
    B, H = case["q"].shape[:2]
    q, k, v, beta, g, dout = _gdn_flat(case, torch.float64)
    parts = []
    for lo in range(0, B * H, head_block):
        sl = slice(lo, lo + head_block)
        parts.append(_gdn_step_block(
            q[sl], k[sl], v[sl], beta[sl], g[sl], dout[sl] if backward else None
        ))
    res = {name: torch.cat([p[name] for p in parts], 0) for name in parts[0]}
    return _gdn_unflat(res, B, H)


def _ste_bf16(x):
    """Round to bf16 in the forward, identity in the backward."""
    return x + (x.to(BF16).to(x.dtype) - x).detach()


def gdn_chunk_emul(case, cast=True, backward=False, solve_order=None):
    """The yardstick: the WY chunk formulation (csrc/gdn.hip header) in fp32
    torch. With `cast` it rounds to bf16 where the kernel does: the state
    before K@S and Q@S, e^{gc}K and e^{gc}Q, N, R before N@R, the output, and
    K e^{gc_last - gc} in the state update (without that last one the
    emulation's s0 and final state carry no rounding at all, 1e-7, and would
    be no yardstick for a kernel that does round there).
    Rounding is straight-through so that autograd gives the gradients of the
    same graph; q, k, v are bf16 leaves (their gradients come back in bf16
    like the op's), `dv32` is the unrounded dv. `solve_order` = n replaces the
    triangular solve by its Neumann series up to M^n: a deliberately broken
    solve that the planted case must expose."""
    B, H, S = case["q"].shape[:3]
    n, C, D = B * H, GDN_CHUNK, GDN_D
    rnd = _ste_bf16 if cast else (lambda x: x)
    q16, k16, v16 = (case[x].detach().cpu().reshape(n, S, D).clone().requires_grad_(backward)
                     for x in ("q", "k", "v"))
    beta = case["beta"].detach().cpu().float().reshape(n, S).clone().requires_grad_(backward)
    g = case["g"].detach().cpu().float().reshape(n, S).clone().requires_grad_(backward)
    q, k, v = q16.float(), k16.float(), v16.float()
    if backward:
        v.retain_grad()
    state = torch.zeros(n, D, D, requires_grad=backward)
    bounds, outs, rs = [], [], []
    eye = torch.eye(C)
    for s0 in range(0, S, C):
        c = min(C, S - s0)
        pad = (0, 0, 0, C - c)
        Q, K, V = (torch.nn.functional.pad(x[:, s0:s0 + c], pad) for x in (q, k, v))
        b = torch.nn.functional.pad(beta[:, s0:s0 + c], (0, C - c))
        gc = torch.nn.functional.pad(g[:, s0:s0 + c], (0, C - c)).cumsum(-1)
        if backward and s0 > 0:
            state.retain_grad()
        bounds.append(state)
        diff = (gc.unsqueeze(-1) - gc.unsqueeze(-2)).tril(0)
        ratio = torch.exp(diff).tril(0)
        M = (b.unsqueeze(-1) * (K @ K.transpose(-1, -2)) * ratio).tril(-1)
        E = torch.exp(gc).unsqueeze(-1)
        EK, EQ, Sb = rnd(E * K), rnd(E * Q), rnd(state)
        rhs = b.unsqueeze(-1) * (V - EK @ Sb)
        if solve_order is None:
            R = torch.linalg.solve_triangular(M + eye, rhs, upper=False)
        else:
            R, term = rhs, rhs
            for _ in range(solve_order):
                term = -(M @ term)
                R = R + term
        N = rnd(((Q @ K.transpose(-1, -2)) * ratio).tril(0))
        outs.append(rnd(EQ @ Sb + N @ rnd(R))[:, :c])
        rs.append(R[:, :c])
        g_tot = gc[:, -1:]
        wK = rnd(K * torch.exp(g_tot - gc).unsqueeze(-1))
        state = torch.exp(g_tot).unsqueeze(-1) * state + wK.transpose(-1, -2) @ R
    out, r = torch.cat(outs, 1), torch.cat(rs, 1)
    res = dict(out=out.detach(), r=r.detach(), fs=state.detach(),
               s0=torch.stack([x.detach() for x in bounds], 1))
    if backward:
        dout = case["dout"].detach().cpu().float().reshape(n, S, D)
        (out * dout).sum().backward()
        res.update(dq=q16.grad, dk=k16.grad, dv=v16.grad, dv32=v.grad, dbeta=beta.grad,
                   dg=g.grad, ds0=torch.stack([x.grad for x in bounds], 1))
    return _gdn_unflat(res, B, H)


def check_gdn_plant(case, ref):
    """The case must do what it says."""
    q, k, v, beta, g = (case[x].double() for x in ("q", "k", "v", "beta", "g"))
    S = q.shape[2]
    assert float((q.norm(dim=-1) - 1).abs().max()) < 0.01          # |q| = 1 everywhere
    kn = k.norm(dim=-1)
    assert float((kn[:, :, 1:] - 1).abs().max() if S > 1 else 0.0) < 0.01
    assert float(v[:, :, 1:].abs().max() if S > 1 else 0.0) <= 1.0
    if bool(case["poison"].any()):                                 # the poisoned rows
        assert float(kn[:, :, 0][case["poison"]].min()) >= 1.99
        assert float(v[:, :, 0].norm(dim=-1)[case["poison"]].min()) > 7.9
        assert float((beta[:, :, 0] * kn[:, :, 0] ** 2 - 1)[case["poison"]].abs().max()) < 0.01
    rep = case["rep"]
    if bool(rep.any()):  # the output of a repeated-key row is the value just written
        assert float((ref["out"][:, :, rep] - v[:, :, rep]).abs().max()) < 0.02
    if S > 1:
        assert float((ref["out"][:, :, S - 1] - 1).abs().max()) < 0.02  # the tail row
    if S > 8:
        assert bool((g[:, :, 8] == -6).all())
    if S > GDN_CHUNK:  # the carry is real: every head hands an O(1) state on
        assert float(ref["s0"][:, :, 1].flatten(-2).norm(dim=-1).min()) > 0.5
    assert float(ref["out"].abs().max()) <= 1.5


def check_gdn_fwd(run, B, H, S, tol_scale=1.0):
    """run(case) -> dict(out, fs, r, s0) of one planted case; every output
    against the fp64 recurrence. `tol_scale` < 1 tightens every tolerance
    (the CPU suite holds the emulation to half of them)."""
    case = gdn_case(B, H, S)
    ref = gdn_step_ref(case)
    check_gdn_plant(case, ref)
    got = run(case)
    for name, tol in (("out", TOL_GDN_OUT), ("fs", TOL_GDN_FS), ("r", TOL_GDN_R),
                      ("s0", TOL_GDN_S0)):
        assert_close(got[name], ref[name], _scaled(tol, tol_scale), name)


GDN_GRADS = ("dq", "dk", "dv", "dbeta", "dg")


def gdn_varlen_case(lens, H, seed=0):
    """One packed row (1, H, sum(lens), 64) of planted documents; every
    document after the first starts with the poisoned row, which follows the
    previous document's tail in memory. Returns (case, per-document cases)."""
    docs = [gdn_case(1, H, n, poison_all=i > 0, seed=100 * seed + i + 1)
            for i, n in enumerate(lens) if n > 0]
    case = {x: torch.cat([d[x] for d in docs], 2) for x in ("q", "k", "v", "beta", "g", "dout")}
    cu = torch.tensor([0] + list(lens), dtype=torch.int64).cumsum(0).to(torch.int32)
    case["cu"] = cu
    return case, docs


def _gdn_cat_docs(parts, names):
    """Per-document results (1, H, len, ...) back into packed rows."""
    return {x: torch.cat([p[x] for p in parts], 2) for x in names}


def check_gdn_bwd(run, B, H, S, tol_scale=1.0):
    """run(case) -> dict(out, dq, dk, dv, dbeta, dg) through the op with bf16
    q, k, v leaves and fp32 beta, decay_log leaves, loss = sum(out * dout)."""
    case = gdn_case(B, H, S)
    ref = gdn_step_ref(case, backward=True)
    check_gdn_plant(case, ref)
    got = run(case)
    assert_close(got["out"], ref["out"], _scaled(TOL_GDN_OUT, tol_scale), "out")
    for name in GDN_GRADS:
        assert_close(got[name], ref[name], _scaled(TOL_GDN_GRAD[name], tol_scale), name)


def check_gdn_varlen_bwd(run, lens, H, tol_scale=1.0):
    """The same on packed documents: run(case, docs) with case["cu"] (docs:
    the per-document cases); the reference is the recurrence on every
    document alone."""
    case, docs = gdn_varlen_case(lens, H)
    refs = [gdn_step_ref(d, backward=True) for d in docs]
    for d, r in zip(docs, refs):
        check_gdn_plant(d, r)
    ref = _gdn_cat_docs(refs, ("out",) + GDN_GRADS)
    assert ref["out"].shape[2] == int(case["cu"][-1]) and 0 in lens
    got = run(case, docs)
    assert_close(got["out"], ref["out"], _scaled(TOL_GDN_OUT, tol_scale), "out")
    for name in GDN_GRADS:
        assert_close(got[name], ref[name], _scaled(TOL_GDN_GRAD[name], tol_scale), name)


def check_gdn_bwd_scan(run, B, H, S, tol_scale=1.0):
    """run(case) -> (drhs (B, H, S, 64), dS0 (B, H, nc, 64, 64)) of the
    reverse scan. No second derivation: dv_t = beta_t drhs_t, so
    drhs_t = dv_t / beta_t with beta >= 0.25 in this case, and dS0[c] is the
    autograd gradient of the state the recurrence holds at row 64 c."""
    case = gdn_case(B, H, S, zero_beta=False)
    assert float(case["beta"].min()) >= 0.25
    ref = gdn_step_ref(case, backward=True)
    check_gdn_plant(case, ref)
    drhs, ds0 = run(case)
    assert_close(drhs, ref["dv"] / case["beta"].double().unsqueeze(-1),
                 _scaled(TOL_GDN_DRHS, tol_scale), "drhs")
    assert_close(ds0, ref["ds0"], _scaled(TOL_GDN_DS0, tol_scale), "dS0")


# ---- causal depthwise conv + SiLU -------------------------------------------

# K = 1..4 at S below, at and above K, one block; and 2 109 440 elements, more
# than the 8192 x 256 threads of the capped grid
CONV_SHAPES = [(2, s, 48, k) for k in (1, 2, 3, 4) for s in (1, 2, 37)] + [(2, 1030, 1024, 4)]
TOL_CONV_Y = dict(rtol=2e-2, atol=2e-2)       # tests/test_blocks_extra.py
TOL_CONV_DX = dict(rtol=3e-2, atol=3e-2)
TOL_CONV_DW = dict(rtol=3e-2, atol=2e-1)


def conv_case(B, S, C, K, seed=0):
    """bf16 x, dy (B, S, C) and w (C, K); |x| = |dy| = 4 on rows 0, K-1 and
    S-1: the rows where a tap first reaches before the sequence, first does
    not, and last exists."""
    gen = _gen(7500 + seed)
    x = torch.randn(B, S, C, generator=gen)
    w = torch.randn(C, K, generator=gen) * 0.5
    dy = torch.randn(B, S, C, generator=gen)
    sign = torch.where(torch.arange(C) % 2 == 0, 4.0, -4.0)
    for row in {0, K - 1, S - 1}:
        if row < S:
            x[:, row] = sign
            dy[:, row] = -sign
    return x.to(BF16), w.to(BF16), dy.to(BF16)


def conv_ref(x, w, dy):
    """fp64 pad / conv1d / SiLU chain and its autograd."""
    x64 = x.detach().cpu().double().requires_grad_(True)
    w64 = w.detach().cpu().double().requires_grad_(True)
    C, K = w64.shape
    xt = torch.nn.functional.pad(x64.transpose(1, 2), (K - 1, 0))
    pre = torch.nn.functional.conv1d(xt, w64.unsqueeze(1), groups=C).transpose(1, 2)
    y = pre * torch.sigmoid(pre)
    y.backward(dy.detach().cpu().double())
    return y.detach(), x64.grad, w64.grad


def check_conv(run, B, S, C, K):
    """run(x, w, dy) -> (y, dx, dw)."""
    x, w, dy = conv_case(B, S, C, K)
    assert float(x[:, S - 1].abs().min()) == 4.0 and float(dy[:, 0].abs().min()) == 4.0
    y, dx, dw = run(x, w, dy)
    ry, rdx, rdw = conv_ref(x, w, dy)
    assert_close(y, ry, TOL_CONV_Y, "y")
    assert_close(dx, rdx, TOL_CONV_DX, "dx")
    assert_close(dw, rdw, TOL_CONV_DW, "dw")


# ---------------------------------------------------------------------------
# Stochastic rounding and AdamW
# ---------------------------------------------------------------------------

_SM64_GAMMA = 0x9E3779B97F4A7C15
_SM64_M1 = 0xBF58476D1CE4E5B9
_SM64_M2 = 0x94D049BB133111EB


def splitmix64(z):
    """numpy uint64 array -> splitmix64 of every element."""
    import numpy as np

    with np.errstate(over="ignore"):
        z = z + np.uint64(_SM64_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_SM64_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_SM64_M2)
        return z ^ (z >> np.uint64(31))


def sr_noise16(n, seed):
    """The 16 noise bits of every element of an n-element tensor: the seed
    contract of csrc/stochastic.hip, which checkpoint-resume relies on.
    Vector body (i < 4 * (n // 4)): field i % 4 of splitmix64(seed ^ (i // 4));
    scalar tail: the low field of splitmix64(seed ^ (2**63 | i))."""
    import numpy as np

    i = np.arange(n, dtype=np.uint64)
    s = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
    body = (splitmix64(s ^ (i // np.uint64(4))) >> (np.uint64(16) * (i % np.uint64(4))))
    tail = splitmix64(s ^ (np.uint64(1 << 63) | i))
    return np.where(i < np.uint64(4 * (n // 4)), body, tail) & np.uint64(0xFFFF)


def sr_round_bits(src, noise16):
    """fp32 tensor + uint64 noise -> bf16 tensor: (bits + noise16) >> 16 in
    32-bit arithmetic; a NaN keeps its upper half with the quiet bit set."""
    import numpy as np

    bits = src.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).astype(np.uint64)
    out = ((bits + noise16) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)
    nan = (bits & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    out = np.where(nan, (bits >> np.uint64(16)) | np.uint64(0x40), out)
    return torch.from_numpy(out.astype(np.uint16).view(np.int16)).view(BF16)


def sr_oracle(src, seed):
    return sr_round_bits(src, sr_noise16(src.numel(), seed))


def assert_same_bits(got, ref, what):
    """Bitwise equality that also holds NaN payloads to account."""
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    view = {2: torch.int16, 4: torch.int32}[got.element_size()]
    assert_bitwise(got.detach().cpu().contiguous().view(view),
                   ref.detach().cpu().contiguous().view(view), what)


# 2 097 152 = 2048 blocks x 256 threads x 4 elements: the last size sends
# both the vector loop and the tail loop of every single-tensor kernel
# through a second grid-stride iteration
SR_BIG = 2_097_152 + 4 * 37 + 3
SR_COPY_SIZES = [1, 3, 4, 5, 1027, SR_BIG]
SR_FRACTIONS = [0x0001, 0x4000, 0x8000, 0xC000, 0xFFFF]


def _f32_from_bits(bits):
    import numpy as np

    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def sr_copy_case(n, seed=0):
    """fp32 source: N(0, 4) with, from both ends inward, the low-half
    fractions of SR_FRACTIONS on +1.5 and -1.5, values on the bf16 grid,
    +-0, +-inf and NaN. Returns (src, on_grid mask)."""
    gen = _gen(8000 + seed)
    src = torch.randn(n, generator=gen) * 2.0
    special = _f32_from_bits(
        [0x3FC00000 | f for f in SR_FRACTIONS] + [0xBFC00000 | f for f in SR_FRACTIONS]
        + [0x3F800000, 0xC0600000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
           0x7FC00001, 0xFFA00000]
    )
    m = min(n, special.numel())
    src[:m] = special[:m]
    src[n - m:] = special[:m].flip(0)
    low = src.view(torch.int32) & 0xFFFF
    return src, (low == 0) & ~src.isnan()


def check_sr_copy(run, n, seed):
    """run(src, seed) -> bf16: bitwise against the oracle."""
    src, on_grid = sr_copy_case(n)
    ref = sr_oracle(src, seed)
    # the oracle does what it says: grid values are exact, NaN stays NaN,
    # everything else is one of the two neighbours
    assert torch.equal(ref[on_grid].float(), src[on_grid])
    assert bool(ref[src.isnan()].isnan().all())
    if n >= 18:
        assert bool(src.isnan().any()) and bool(src.isinf().any()) and int(on_grid.sum()) >= 6
    check_sr_neighbours(ref, src)
    assert_same_bits(run(src, seed), ref, f"SR copy n={n} seed={seed}")


def check_sr_neighbours(got, src):
    """Every result is the truncation of src to bf16 or the next bf16 away
    from zero (NaN stays NaN)."""
    bits = src.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    floor = bits >> 16
    g = got.view(torch.int16).to(torch.int64) & 0xFFFF
    ok = (g == floor) | (g == ((floor + 1) & 0xFFFF)) | (src.isnan() & got.isnan())
    on_grid = (bits & 0xFFFF) == 0
    ok &= ~on_grid | (g == floor) | src.isnan()
    assert bool(ok.all()), f"{int((~ok).sum())} results are not a neighbour of the source"


def check_sr_statistics(run, seed, N=1 << 20):
    """run(src, seed) -> bf16. For every fraction f / 65536 of SR_FRACTIONS,
    on +1.5 and -1.5, the frequency of rounding away from zero over N equal
    elements is within 6 sigma of f, sigma = sqrt(f (1 - f) / N)."""
    for base in (0x3FC00000, 0xBFC00000):
        for frac in SR_FRACTIONS:
            src = _f32_from_bits([base | frac]).expand(N).contiguous()
            got = run(src, seed)
            up = (got.view(torch.int16).to(torch.int64) & 0xFFFF) == (base >> 16) + 1
            down = (got.view(torch.int16).to(torch.int64) & 0xFFFF) == (base >> 16)
            assert bool((up | down).all())
            f = frac / 65536.0
            sigma = math.sqrt(f * (1 - f) / N)
            freq = float(up.double().mean())
            assert abs(freq - f) <= 6 * sigma, (hex(base), hex(frac), freq, f, sigma)


ADAMW_SIZES = [1, 3, 4, 5, 4097, SR_BIG]
ADAMW_BETAS = (0.9, 0.95)
ADAMW_EPS = 1e-8
ADAMW_HYPER = [dict(lr=1e-2, weight_decay=0.1, step=3), dict(lr=1e-4, weight_decay=0.0, step=1)]
TOL_ADAMW_M = dict(rtol=1e-5, atol=1e-6)      # tests/test_ops_kernels.py
TOL_ADAMW_V = dict(rtol=1e-5, atol=1e-7)


def adamw_case(n, seed=0):
    """bf16 p, g ~ N(0, 1); fp32 m ~ 0.1 N(0, 1), v ~ 0.01 U(0, 1)."""
    gen = _gen(8100 + seed)
    p = torch.randn(n, generator=gen).to(BF16)
    g = torch.randn(n, generator=gen).to(BF16)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    return p, g, m, v


def adamw_ref(p, g, m, v, lr, weight_decay, step, betas=ADAMW_BETAS, eps=ADAMW_EPS):
    """Decoupled-weight-decay Adam in fp64 -> (p, m, v), nothing rounded."""
    b1, b2 = betas
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    p = p * (1 - lr * weight_decay)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - lr * (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + eps)
    return p, m, v


def ulp_bf16(x):
    """Spacing of the bf16 grid at |x| (fp64 tensor)."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def check_adamw(run, n, hyper):
    """run(p, g, m, v, lr, weight_decay, step, seed) -> (p, m, v) after one
    fused step. m and v at the project's fp32 tolerances. p, element by
    element: stochastic rounding moves the fp32 result to one of its two bf16
    neighbours, and the fp32 result differs from the fp64 one by ulps of
    fp32 -- of the two terms of the final subtraction, p (1 - lr wd) and the
    update, not of their difference: where they cancel (p = -1.8e-3 stepping
    to p_ref = -1.5e-7) plain fp32 arithmetic is 1.6 bf16 ulps of the RESULT
    away from fp64. So with slack = 2**-20 (|p (1 - lr wd)| + |update|), 16
    fp32 ulps of the terms,
        |p_new - p_ref| <= ulp_bf16(|p_ref| + slack) (1 + 2**-10) + slack.
    Away from a cancellation the slack is 2**-12 of a bf16 ulp.

    That bound alone cannot see a bias below one bf16 ulp, such as a dropped
    weight decay (lr wd |p| = 1e-3 |p| against an ulp of 4e-3..8e-3 |p|) or,
    at lr = 1e-4, a parameter left as it was. SR is unbiased, so for fixed
    signs s_i the sum T = sum_i s_i (p_new_i - p_ref_i) has mean 0 and
    variance sum_i ulp_i^2 q_i (1 - q_i), q_i the position of p_ref_i between
    its neighbours. T is held to 6 sigma, plus the summed fp32 slack of the
    bound above, for s = sign(p) (a dropped decay moves it by 1e-3 sum |p_i| =
    0.8e-3 n against 6 sigma = 0.012 sqrt(n)) and for s = sign(p_ref - p) (an
    unchanged parameter moves it by sum |p_ref_i - p_i|)."""
    p, g, m, v = adamw_case(n)
    rp, rm, rv = adamw_ref(p, g, m, v, **hyper)
    decayed = p.double() * (1 - hyper["lr"] * hyper["weight_decay"])
    slack = 2.0 ** -20 * (decayed.abs() + (decayed - rp).abs())
    ulp = ulp_bf16(rp.abs() + slack)
    got_p, got_m, got_v = run(p.clone(), g, m.clone(), v.clone(), seed=1234 + n, **hyper)
    assert got_p.dtype == BF16
    assert_close(got_m, rm, TOL_ADAMW_M, "exp_avg")
    assert_close(got_v, rv, TOL_ADAMW_V, "exp_avg_sq")
    err = got_p.detach().cpu().double() - rp
    bad = err.abs() > ulp * (1 + 2.0 ** -10) + slack
    assert not bool(bad.any()), (
        f"p: {int(bad.sum())}/{n} elements further than one bf16 ulp from the fp64 step; "
        f"first at {int(bad.nonzero()[0])}"
    )
    if n >= 4097:
        q = torch.remainder(rp.abs() / ulp, 1.0)
        sigma = float((ulp ** 2 * q * (1 - q)).sum().sqrt())
        slack = float(ulp.sum()) * 2.0 ** -10 + float(slack.sum())
        moved = (rp - p.double()).abs().sum()
        if n >= 1 << 20:  # at this size an unchanged p shows, four times over
            assert float(moved) > 4 * (6 * sigma + slack)
        for name, s in (("sign(p)", torch.sign(p.double())),
                        ("sign(step)", torch.sign(rp - p.double()))):
            bias = float((s * err).sum())
            assert abs(bias) <= 6 * sigma + slack, (name, bias, sigma, slack)


def check_adamw_sr_mean(run, N=1 << 20):
    """Where SR matters: N equal elements p = 1, g = 0.5, m = v = 0, lr = 1e-4,
    no decay, step 1. p_ref = 0.9999 lies between 1 - 2**-8 and 1 at
    q = 0.0256 from the upper one; the mean of p_new is within 6 sigma =
    3.6e-6 of it (sigma = 2**-8 sqrt(q (1 - q) / N)), where round-to-nearest
    is off by 1e-4."""
    p = torch.ones(N, dtype=BF16)
    g = torch.full((N,), 0.5, dtype=BF16)
    m, v = torch.zeros(N), torch.zeros(N)
    rp, _, _ = adamw_ref(p, g, m, v, lr=1e-4, weight_decay=0.0, step=1)
    assert abs(float(rp[0]) - 0.9999) < 1e-9
    q = (1.0 - float(rp[0])) * 256
    sigma = 2.0 ** -8 * math.sqrt(q * (1 - q) / N)
    assert abs(6 * sigma - 3.6e-6) < 0.1e-6
    got, _, _ = run(p, g, m, v, lr=1e-4, weight_decay=0.0, step=1, seed=99)
    vals = got.detach().cpu().double()
    assert bool(((vals == 1.0) | (vals == 1.0 - 2.0 ** -8)).all())
    assert abs(float(vals.mean()) - float(rp[0])) <= 6 * sigma, float(vals.mean())


# The multi-tensor kernel walks 8-element slots with 16384 x 256 threads.
ADAMW_MULTI_STRIDE = 16384 * 256
ADAMW_MULTI_SMALL = dict(
    sizes=[1000, 257, 0, 4096, 3, 1004], steps=[1, 3, 1000, 1000, 2, 7],
    seeds=[11, 2 ** 40 + 22, 33, 2 ** 62 + 5, 44, 55],
)


def adamw_multi_big_sizes():
    """One tensor that leaves the grid 100 slots short of a full stride, 50
    tensors of 1..50 elements (one of them emptied) and one of 300 001: the
    second slot of the first 100 threads lands in the small tensors, that of
    the following ones in the last tensor, each several tensors after its
    first."""
    sizes = [8 * (ADAMW_MULTI_STRIDE - 100)] + list(range(1, 51)) + [300_001]
    sizes[20] = 0
    slots = [(s + 7) // 8 for s in sizes]
    assert sum(slots) > ADAMW_MULTI_STRIDE          # the pipelined loop iterates
    assert slots[0] < ADAMW_MULTI_STRIDE < slots[0] + sum(slots[1:51])
    assert sum(slots[:51]) < ADAMW_MULTI_STRIDE + 200 < sum(slots)
    return sizes


def adamw_multi_case(sizes, seed=0):
    """Lists of bf16 p, g and fp32 m, v, one generator for the whole list."""
    gen = _gen(8200 + seed)
    ps = [torch.randn(n, generator=gen).to(BF16) for n in sizes]
    gs = [torch.randn(n, generator=gen).to(BF16) for n in sizes]
    ms = [torch.randn(n, generator=gen) * 0.1 for n in sizes]
    vs = [torch.rand(n, generator=gen) * 0.01 for n in sizes]
    return ps, gs, ms, vs


def stochastic_adamw_seed(seed, step_count, idx):
    """The documented per-parameter seed of optim.StochasticAdamW: idx counts
    the parameters WITH a gradient, from 1, over all groups of one step."""
    return (seed * 0x9E3779B9 + step_count * 0x85EBCA6B + idx * 0xC2B2AE35) & 0x7FFFFFFFFFFFFFFF


ADD_BF16_SIZES = [0, 1, 7, 8, 9, 33_554_432 + 8 * 5 + 3]   # 16384 x 256 x 8 + tail


def check_add_bf16_into_f32(run, n):
    """run(acc, x) -> acc + x: one IEEE add per element, so bitwise."""
    gen = _gen(8300)
    acc = torch.randn(n, generator=gen)
    x = torch.randn(n, generator=gen).to(BF16)
    if n:
        acc[-1], x[-1] = 1.0, -3.0
    got = run(acc.clone(), x)
    assert_same_bits(got, acc + x.float(), f"add n={n}")


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------

# 4 194 304 = 2048 blocks x 256 threads x 8 elements
SILU_SIZES = [1, 7, 8, 9, 1_000_003, 4_194_304 + 8 * 37 + 5]
SILU_PACKED_SHAPES = [(1, 8), (3, 72), (130, 1536), (4100, 1032)]  # 528 900 > 2048 x 256 vectors
# -100: exp2 overflows and the sigmoid must become 0, not NaN; +-88: the
# sigmoid is (sub)normal; -1.278 (-1.28125 in bf16): silu' crosses zero
SILU_GATES = [-100.0, 88.0, -1.278, -88.0, 20.0, -20.0, -0.0, 0.0]
# fp32 math and one bf16 rounding (TOL_DLOGITS); the atol also covers the
# ~1e-7 |g b| <= 6.4e-6 of fp32 cancellation at the zero of silu'
TOL_SILU = dict(rtol=1e-2, atol=1e-5)


def _silu_plant(a, b, g):
    n = a.numel()
    m = min(n, len(SILU_GATES))
    gates = torch.tensor(SILU_GATES)
    a[:m] = gates[:m]
    a[n - m:] = gates[:m].flip(0)
    for t, mag in ((b, 8.0), (g, -8.0)):
        t[:m] = mag
        t[n - m:] = -mag


def silu_case(n, seed=0):
    """bf16 gate a ~ N(0, 4), up b and upstream grad g ~ N(0, 1) clipped to
    |.| <= 8 (|g b| <= 64), SILU_GATES with |b| = |g| = 8 on both ends."""
    gen = _gen(9000 + seed)
    a = torch.randn(n, generator=gen) * 2.0
    b = torch.randn(n, generator=gen).clamp(-8, 8)
    g = torch.randn(n, generator=gen).clamp(-8, 8)
    _silu_plant(a, b, g)
    return a.to(BF16), b.to(BF16), g.to(BF16)


def silu_ref(a, b, g):
    a64, b64, g64 = (t.detach().cpu().double() for t in (a, b, g))
    sig = torch.sigmoid(a64)
    return a64 * sig * b64, g64 * b64 * sig * (1 + a64 * (1 - sig)), g64 * a64 * sig


def check_silu(run, n):
    """run(a, b, g) -> (out, da, db)."""
    a, b, g = silu_case(n)
    assert float(a[-1]) == -100.0 and float((g.float() * b.float()).abs().max()) <= 64.0
    got = run(a, b, g)
    for name, x, r in zip(("out", "da", "db"), got, silu_ref(a, b, g)):
        assert x.dtype == BF16 and not bool(x.isnan().any()), name
        assert_close(x, r, TOL_SILU, name)


def silu_packed_case(rows, inter, seed=0):
    """bf16 x (rows, 2 I) = [gate | up] and g (rows, I): the largest gate (20)
    and up (+-8) values in the last column of each half, |g| = 8 there,
    SILU_GATES down the first column of the gate half."""
    gen = _gen(9100 + seed)
    gate = torch.randn(rows, inter, generator=gen) * 2.0
    up = torch.randn(rows, inter, generator=gen).clamp(-4, 4)
    g = torch.randn(rows, inter, generator=gen).clamp(-8, 8)
    sign = torch.where(torch.arange(rows) % 2 == 0, 1.0, -1.0)
    gate[:, 0] = torch.tensor(SILU_GATES)[torch.arange(rows) % len(SILU_GATES)]
    gate.clamp_(max=19.0)
    gate[:, inter - 1] = 20.0
    up[:, inter - 1] = 8.0 * sign
    g[:, inter - 1] = -8.0
    return torch.cat([gate, up], 1).to(BF16), g.to(BF16)


def check_silu_packed(run, rows, inter):
    """run(x, g) -> (out (rows, I), dx (rows, 2 I)); the halves of dx are
    compared separately."""
    x, g = silu_packed_case(rows, inter)
    a, b = x[:, :inter], x[:, inter:]
    assert float(a.max()) == 20.0 and bool((a[:, inter - 1] == 20.0).all())
    assert float(b.abs().max()) == 8.0 and bool((b[:, inter - 1].abs() == 8.0).all())
    out, dx = run(x, g)
    assert out.shape == (rows, inter) and dx.shape == (rows, 2 * inter)
    rout, rda, rdb = silu_ref(a, b, g)
    assert_close(out, rout, TOL_SILU, "out")
    assert_close(dx[:, :inter], rda, TOL_SILU, "dx gate half")
    assert_close(dx[:, inter:], rdb, TOL_SILU, "dx up half")
