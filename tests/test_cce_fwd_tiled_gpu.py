"""The tiled CCE forward (cce_fwd_tiled_kernel + cce_fwd_merge_kernel) on the
GPU: 256 x 256 tile edges, the one- and two-k-tile pipelines, state carried
across the tiles of one span, the merge across spans, the rounded lse and
run-to-run bits. Cases: tests/cce_tiled_cases.py (validated on the CPU by
tests/test_cce_fwd_tiled.py).
"""

import pytest
import torch

from tests import cce_tiled_cases as tc
from tests import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _raw(e, c, targets, n_spans=0):
    from d9d_amd.ops._ext import get_ext

    return get_ext().cce_fwd(e.to(DEV), c.to(DEV), targets.to(DEV), n_spans)


def _run(n_spans):
    def run(e, c, targets):
        lse, tgt, _ = _raw(e, c, targets, n_spans)
        has = (targets >= 0) & (targets < c.shape[0])
        # rows without a column in the shard report -1e30
        assert bool((tgt.cpu()[~has] < -1e29).all())
        return lse, torch.where(has.to(DEV), tgt, torch.zeros_like(tgt))

    return run


@pytest.mark.parametrize("shape", tc.EDGE_SHAPES, ids=str)
def test_tiled_fwd_edges(shape):
    """T == 1, V == 1, V one short of / equal to / one past a tile, a second
    row tile of one row, K = 64 (one k-tile), 128 (nothing staged in the loop)
    and 192 (first steady-state k-tile); default n_spans."""
    tc.check_tiled_fwd(_run(0), *shape)


@pytest.mark.parametrize(
    "shape,n_spans",
    [(s, n) for s in tc.SPAN_SHAPES for n in tc.span_counts(s[1])],
    ids=str,
)
def test_tiled_fwd_spans(shape, n_spans):
    """One span (running state across every tile), the maximum (one tile per
    block, everything merged), a value between where V has more than two tiles
    ((70, 333, 1024) has two, so nothing lies between), and a request above
    the number of tiles. The dominant logit sits on the span's first and last
    column in turn; row 0 has its maximum and its target in different spans."""
    tc.check_tiled_fwd(_run(n_spans), *shape, n_spans)


@pytest.mark.parametrize("shape", tc.ROUNDED_SHAPES, ids=str)
def test_tiled_fwd_rounded_lse(shape):
    kr.check_cce_rounded_lse(lambda e, c, t: _raw(e, c, t)[2], *shape)


@pytest.mark.parametrize("shape,n_spans", [((258, 257, 64), 0), ((130, 1000, 320), 3)], ids=str)
def test_tiled_fwd_same_bits_twice(shape, n_spans):
    e, c, targets = tc.tiled_case(*shape, max(n_spans, 1))
    e, c, targets = e.to(DEV), c.to(DEV), targets.to(DEV)
    first = _raw(e, c, targets, n_spans)
    second = _raw(e, c, targets, n_spans)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_tiled_fwd_rejects_negative_n_spans():
    e, c, targets = tc.tiled_case(1, 1, 64)
    with pytest.raises(RuntimeError):
        _raw(e, c, targets, -1)
