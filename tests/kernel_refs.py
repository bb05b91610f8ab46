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
