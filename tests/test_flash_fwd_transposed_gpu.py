"""The flash forward computes S^T = K Q^T and O^T = V^T P^T: P stays in the
MFMA C registers and the K tile's rows are loaded in a permuted kv order
(pv_pos in d9d_amd/csrc/attention.hip). These cases aim at what that layout
can get wrong -- a slot of the permutation, the masking of ragged tiles in
permuted slots, the per-lane softmax state and the exchanged partial sums of
l, the repacked epilogue -- against the fp64 references of
tests/kernel_refs.py.
"""

import math

import pytest
import torch

from tests import kernel_refs as kr
from tests.test_kernel_edges import attn_run, attn_varlen_run

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


def test_chain_selfcheck():
    """C registers of X = A1 @ B1, computed with A1's rows taken in pv_pos
    order and packed as the forward packs P^T, are the B operand of
    Y = A2 @ X with A2 in natural order."""
    from d9d_amd.ops import _ext

    ext = _ext.get_ext()
    g = kr._gen(7100)
    a1 = torch.randn(32, 32, generator=g).to(BF16)
    b1 = torch.randn(32, 16, generator=g).to(BF16)
    a2 = torch.randn(16, 32, generator=g).to(BF16)
    y = ext.mfma_chain_selfcheck(a1.to(DEV), b1.to(DEV), a2.to(DEV)).cpu()
    x = a1.float() @ b1.float()
    ref = a2.float() @ x
    # The kernel rounds X to bf16 (half an ulp, 2^-9 relative) before the
    # second product; where Y's terms cancel that is not relative to Y, so it
    # enters as an absolute term: sum_k |A2[i,k]| |X[k,j]| 2^-9.
    bound = a2.float().abs() @ x.abs() * 2.0 ** -9
    err = (y - ref).abs()
    ok = err <= 1e-2 * ref.abs() + bound
    assert bool(ok.all()), f"max err {err.max().item():.4g}, {int((~ok).sum())} of 256 off"


def test_slot_sweep():
    """Row i's dominant key is kv i, over a full 64-row tile and a half tile:
    every pv_pos slot decides some row's output, so a wrong slot returns a
    wrong V row."""
    Sq = Skv = 96
    D = 64
    scale = 1.0 / math.sqrt(D)
    g = kr._gen(7200)
    q1 = torch.randn(1, Sq, 1, D, generator=g)
    k = torch.randn(1, Skv, 1, D, generator=g) * 0.3
    v = torch.randn(1, Skv, 1, D, generator=g)
    k += q1 / (q1.pow(2).sum(-1, keepdim=True) * scale) * 16.0   # logit 16 on (i, i)
    case = dict(
        q=q1.expand(1, Sq, 2, D).contiguous().to(BF16), k=k.to(BF16), v=v.to(BF16),
        dout=None, dlse=None, sinks=None, causal=False, scale=scale, window_left=-1,
        q_offset=0,
    )
    s = torch.einsum("bqhd,bkhd->bhqk", case["q"].double(), case["k"].double().expand(1, Skv, 2, D))
    p = torch.softmax(s * scale, -1)
    assert bool((p.max(-1).values > 0.9).all())
    assert bool((p.argmax(-1) == torch.arange(Sq)).all())
    ref_out, ref_lse = kr.attn_fwd64(
        case["q"].double(), case["k"].double(), case["v"].double(), False, scale, -1, None, 0
    )
    got = attn_run(DEV)(case, False, False)
    kr.assert_close(got["out"], ref_out, kr.TOL_ATTN_OUT, "out")
    kr.assert_close(got["lse"], ref_lse, kr.TOL_ATTN_LSE, "lse")


def _ragged_case(Sq, Skv, causal):
    off = Skv - Sq if causal else 0
    if off >= 0:
        return kr.attn_case(1, Sq, Skv, 4, 2, 64, causal=causal, q_offset=off)
    # Fewer keys than query rows: the planting of attn_case has no diagonal to
    # walk. The visible rows' dominant key is the LAST key, the row the
    # kernel's clamped loads duplicate into the rest of the tile.
    g = kr._gen(7300 + Skv)
    scale = 1.0 / 8.0
    qg = torch.randn(1, Sq, 2, 1, 64, generator=g)
    q = qg.expand(1, Sq, 2, 2, 64).reshape(1, Sq, 4, 64).clone()
    k = torch.randn(1, Skv, 2, 64, generator=g) * 0.3
    v = torch.randn(1, Skv, 2, 64, generator=g)
    last = qg[0, Sq - 1, :, 0]
    k[0, Skv - 1] += last / (last.pow(2).sum(-1, keepdim=True) * scale) * 10.0
    return dict(
        q=q.to(BF16), k=k.to(BF16), v=v.to(BF16), dout=None, dlse=None, sinks=None,
        causal=True, scale=scale, window_left=-1, q_offset=off,
    )


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("Skv", [1, 31, 33, 63, 65])
def test_ragged_tiles(Skv, causal):
    """The kv rows past Skv are clamped duplicates of the last key; they land
    in permuted slots of the tile and must stay masked."""
    Sq = 17
    case = _ragged_case(Sq, Skv, causal)
    ref_out, ref_lse = kr.attn_fwd64(
        case["q"].double(), case["k"].double(), case["v"].double(), causal,
        case["scale"], -1, None, case["q_offset"],
    )
    got = attn_run(DEV)(case, False, False)
    # rows that see no key at all (causal, Skv < Sq) have no softmax: the
    # reference is NaN there, the kernel's value is only required to be finite
    first = max(0, -case["q_offset"]) if causal else 0
    assert first < Sq
    assert bool(torch.isfinite(got["out"].float()).all())
    kr.assert_close(got["out"][:, first:], ref_out[:, first:], kr.TOL_ATTN_OUT, "out")
    kr.assert_close(got["lse"][..., first:], ref_lse[..., first:], kr.TOL_ATTN_LSE, "lse")


@pytest.mark.parametrize("D", [32, 64, 80, 96, 128])
def test_head_dims(D):
    """Every forward instantiation and a padded head dim; the unchanged
    backward consumes the new out and lse."""
    kr.check_attn(attn_run(DEV), kr.attn_case(1, 70, 70, 4, 2, D))


@pytest.mark.parametrize(
    "window_left,with_sinks", [(-1, True), (5, True), (0, False), (64, False)]
)
def test_sinks_and_windows(window_left, with_sinks):
    """The sink seeds l on one column class of each row and m on all lanes;
    windows leave rows of a tile with nothing visible before their first
    key."""
    case = kr.attn_case(1, 130, 130, 4, 2, 64, window_left=window_left, with_sinks=with_sinks)
    kr.check_attn(attn_run(DEV), case)


def test_varlen():
    case = kr.attn_varlen_case([1, 63, 65, 129], [1, 63, 65, 129], 4, 2, 64)
    kr.check_attn_varlen(attn_varlen_run(DEV), case)


def test_tile_order():
    """Three q-tiles per (batch, head): whichever order the grid walks them
    in, every tile must land on its own rows."""
    kr.check_attn(attn_run(DEV), kr.attn_case(2, 300, 300, 4, 2, 128))
