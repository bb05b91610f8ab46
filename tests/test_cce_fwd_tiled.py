"""The tiled CCE forward's cases on the CPU path.

Runs every case of tests/cce_tiled_cases.py through ops.cce._chunk_fwd, so the
case conditions (planted column dominates, |logit| <= 12.5) and the rounded-lse
check's 10% cap are verified without a GPU; tests/test_cce_fwd_tiled_gpu.py
runs the same cases on the HIP kernel.
"""

import pytest
import torch

from tests import cce_tiled_cases as tc
from tests import kernel_refs as kr


def _fwd_cpu(e, c, targets):
    from d9d_amd.ops.cce import LM_IGNORE_INDEX, _chunk_fwd

    # _chunk_fwd takes global targets: mark what has no column as ignored
    t = targets.clone()
    t[(t < 0) | (t >= c.shape[0])] = LM_IGNORE_INDEX
    return _chunk_fwd(e.float(), c, t, 0)


@pytest.mark.parametrize("shape", tc.EDGE_SHAPES, ids=str)
def test_tiled_cases_edges_cpu(shape):
    tc.check_tiled_fwd(_fwd_cpu, *shape)


@pytest.mark.parametrize("shape", tc.SPAN_SHAPES, ids=str)
def test_tiled_cases_spans_cpu(shape):
    for n_spans in tc.span_counts(shape[1]):
        tc.check_tiled_fwd(_fwd_cpu, *shape, n_spans)


def test_span_columns_cover_the_vocab():
    for V in (1, 255, 256, 257, 333, 1000):
        for n_spans in tc.span_counts(V):
            n = min(n_spans, tc.n_tiles(V))
            edges = [tc.span_columns(V, n_spans, s) for s in range(n)]
            assert edges[0][0] == 0 and edges[-1][1] == V - 1
            for (_, last), (first, _) in zip(edges, edges[1:]):
                assert first == last + 1


def test_case_has_the_rows_the_merge_needs():
    """A row whose maximum and target lie in different spans, ignored rows and
    targets outside the shard."""
    T, V, K = tc.SPAN_SHAPES[0]
    n = tc.n_tiles(V)
    e, c, targets = tc.tiled_case(T, V, K, n)
    _, _, logits = tc.reference(e, c, targets)
    assert int(logits[0].argmax()) // tc.TILE != int(targets[0]) // tc.TILE
    assert bool((targets == kr.IGNORE).any())
    assert bool((targets == -1).any()) and bool((targets >= V).any())


@pytest.mark.parametrize("shape", tc.ROUNDED_SHAPES, ids=str)
def test_rounded_lse_cases_cpu(shape):
    """kr.check_cce_rounded_lse keeps at least 90% of the rows at the shapes
    the GPU test uses (the CPU bf16 path takes its lse from rounded logits)."""
    from d9d_amd.ops.cce import _chunk_fwd

    kr.check_cce_rounded_lse(lambda e, c, t: _chunk_fwd(e, c, t, 0)[0], *shape)
