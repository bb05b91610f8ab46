"""Planted cases for the tiled CCE forward (256 x 256 tiles, vocab spans).

kernel_refs.cce_planted_columns plants at the edges of 128-wide tiles; the
tiled kernel's edges are the 256-wide vocab tile, the last (padded) tile and
the vocab spans that separate blocks sweep before their partials are merged.
Built like kernel_refs.cce_case (e = 4, c = 2 on the planted column over a
background of std ~1), generated on the CPU from a seeded generator, checked
against kernel_refs.cce_fwd_ref.
"""

import math

import torch

from tests import kernel_refs as kr

TILE = 256

EDGE_SHAPES = [(1, 1, 64), (1, 300, 64), (257, 255, 128), (256, 256, 192), (258, 257, 64)]
SPAN_SHAPES = [(130, 1000, 320), (70, 333, 1024)]
ROUNDED_SHAPES = [(257, 600, 192), (258, 257, 64), (300, 2100, 1024)]


def n_tiles(V):
    return -(-V // TILE)


def span_columns(V, n_spans, s):
    """First and last column of span s when V's tiles are cut into n_spans
    spans: tiles [s * n / n_spans, (s + 1) * n / n_spans), the kernel's rule."""
    n = n_tiles(V)
    n_spans = min(max(n_spans, 1), n)
    lo = s * n // n_spans
    hi = (s + 1) * n // n_spans
    return lo * TILE, min(hi * TILE, V) - 1


def span_counts(V):
    """One span, one value between (where there is one), the maximum, and a
    request above the maximum, which the kernel caps."""
    n = n_tiles(V)
    return sorted({1, (n + 2) // 2, n}) + [n + 5]


def planted_columns(V, n_spans):
    n = n_tiles(V)
    spans = min(max(n_spans, 1), n)
    first, last = span_columns(V, spans, spans // 2)  # an inner span if any
    tgt_col = max(V - 2, 0)
    non_tgt_col = V // 3
    cand = [0, 255, 256, V - 1, TILE * ((V - 1) // TILE), first, last, tgt_col, non_tgt_col]
    cols = []
    for c in cand:
        if 0 <= c < V and c not in cols:
            cols.append(c)
    return cols, tgt_col, non_tgt_col


def tiled_case(T, V, K, n_spans=1, seed=0):
    """bf16 e (T, K), c (V, K) and int64 LOCAL targets as cce_fwd takes them.
    Row r belongs to group g = r % len(cols); e[r, g] = 4 and c[cols[g], g] = 2,
    so logit (r, cols[g]) is 8 above the background. Special targets: the last
    column, the first column of the last tile, IGNORE (-1 once local), column
    0, below the shard (-1) and above it (V + 5)."""
    g = kr._gen(7000 + seed)
    cols, tgt_col, non_tgt_col = planted_columns(V, n_spans)
    e = torch.randn(T, K, generator=g) * 0.5
    c = torch.randn(V, K, generator=g) * (0.5 / math.sqrt(K))
    targets = torch.randint(0, V, (T,), generator=g)
    group = torch.arange(T) % len(cols)
    for gi, col in enumerate(cols):
        e[group == gi, gi] = 4.0
        c[col, gi] = 2.0
    for r in range(T):
        col = cols[int(group[r])]
        if col == tgt_col:
            targets[r] = tgt_col
        elif targets[r] == non_tgt_col:
            targets[r] = (non_tgt_col + 1) % V
    free = [r for r in range(T) if cols[int(group[r])] != tgt_col]
    special = [s for s in (V - 1, TILE * ((V - 1) // TILE), kr.IGNORE, 0, -1, V + 5)
               if s != non_tgt_col]
    for r, s in zip(free, special):
        targets[r] = s
    if T > 0 and free and free[0] == 0 and n_tiles(V) > 1:
        # row 0: maximum in column 0 (the first span), target in the last tile
        assert cols[int(group[0])] == 0 and int(targets[0]) == V - 1
    return e.to(kr.BF16), c.to(kr.BF16), targets


def reference(e, c, targets):
    """(lse, target logit, logits) in fp64; target logit 0 where the row has
    none in [0, V)."""
    V = c.shape[0]
    t = targets.clone()
    t[(t < 0) | (t >= V)] = kr.IGNORE
    return kr.cce_fwd_ref(e, c, t)


def check_tiled_fwd(run, T, V, K, n_spans=1):
    """run(e, c, local_targets) -> (lse, target logit with 0 where there is
    none). Asserts what kr.check_cce_fwd asserts, on this module's case."""
    e, c, targets = tiled_case(T, V, K, n_spans)
    lse, tl = run(e, c, targets)
    rlse, rtl, logits = reference(e, c, targets)
    top = logits.max(-1).values
    assert float((rlse - top).abs().max()) < 0.7
    assert float(logits.abs().max()) <= 12.5
    kr.assert_close(lse, rlse, kr.TOL_CCE_LSE, "lse")
    kr.assert_close(tl, rtl, kr.TOL_CCE_LSE, "target logit")
