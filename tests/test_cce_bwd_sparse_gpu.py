"""Tile-skipping CCE backward: the tile mask, cce_bwd_de / cce_bwd_dc against
the fp64 reference and against the forced dense route, routing, host checks."""

import pytest
import torch

import kernel_refs as kr
from kernel_refs import (
    IGNORE, TOL_CCE_DC_UNIT, TOL_CCE_DE_UNIT, assert_close, cce_case, cce_e2e_ref,
)

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -12
SHAPES = [(130, 1001, 192), (64, 128, 64), (1, 129, 64)]


def _ext():
    from d9d_amd.ops._ext import get_ext

    return get_ext()


def _cce():
    from d9d_amd.ops import cce

    return cce


def _tile_any(d):
    """(ceil(R/64), ceil(V/128)) bool: the tile holds a nonzero."""
    R, V = d.shape
    nrb, nvt = -(-R // 64), -(-V // 128)
    pad = torch.zeros(nrb * 64, nvt * 128, dtype=torch.bool)
    pad[:R, :V] = d.detach().cpu().float() != 0
    return pad.view(nrb, 64, nvt, 128).any(3).any(1)


# ---- mask exactness ------------------------------------------------------------


@pytest.mark.parametrize("R,V", [(130, 1001), (64, 128), (1, 129), (200, 300), (70, 520)])
@pytest.mark.parametrize("vocab_start,with_dlse", [(0, False), (1000, True)])
def test_mask_matches_plain_dlogits(R, V, vocab_start, with_dlse):
    ext = _ext()
    logits, lse, targets, dl, dlse = kr.cce_dlogits_case(R, V, vocab_start, with_dlse)
    # second half of the rows: the target 12 above everything else, so only
    # it survives the filter; rows whose target is ignored or in another
    # shard have their mass elsewhere (lse 10 above the shard's)
    h = R // 2
    local = targets[h:] - vocab_start
    owned = (targets[h:] != IGNORE) & (local >= 0) & (local < V)
    logits[h:] = (logits[h:].float() * 0.25 - 7.0).to(kr.BF16)
    rows = torch.arange(h, R)[owned]
    logits[rows, local[owned]] = 5.0
    lse = torch.logsumexp(logits.double(), -1)
    lse[h:][~owned] += 10.0
    lse = lse.float()
    args = (lse.to(DEV), targets.to(DEV), dl.to(DEV), dlse.to(DEV) if with_dlse else None)
    plain = ext.cce_dlogits_(logits.to(DEV).clone(), *args, vocab_start, IGNORE, EPS)
    want = _tile_any(plain)
    assert bool(want.any())
    if V >= 512:  # wide enough for the peaked rows to leave tiles empty
        assert not bool(want.all())

    nrb, nvt = -(-R // 64), -(-V // 128)
    mask = torch.full((nrb, nvt), 7, dtype=torch.uint8, device=DEV)
    full = ext.cce_dlogits_mask_(
        logits.to(DEV).clone(), args[0], args[1], args[2], args[3], mask,
        vocab_start, IGNORE, EPS, True)
    kr.assert_bitwise(full, plain, "dlogits with write_zeros")
    assert torch.equal(mask.cpu().bool(), want)
    assert int(mask.max()) <= 1

    mask2 = torch.full((nrb, nvt), 7, dtype=torch.uint8, device=DEV)
    src = logits.to(DEV).clone()
    part = ext.cce_dlogits_mask_(
        src.clone(), args[0], args[1], args[2], args[3], mask2,
        vocab_start, IGNORE, EPS, False)
    assert torch.equal(mask2.cpu().bool(), want)
    # set tiles hold the dlogits, the others were left as they were
    sel = want.repeat_interleave(64, 0).repeat_interleave(128, 1)[:R, :V].to(DEV)
    kr.assert_bitwise(torch.where(sel, part, plain), plain, "set tiles")
    kr.assert_bitwise(torch.where(sel, src, part), src, "unset tiles untouched")


# ---- sparse against the reference and against forced dense --------------------


def _run(route, e, c, targets, eps, monkeypatch, chunk=None, with_lse=False, lse_w=0.25):
    """loss.sum() backward: each token's gradient has scale 1, the scale
    kernel_refs' unit tolerances are stated for."""
    cce = _cce()
    monkeypatch.setenv("D9D_CCE_BWD", route)
    if chunk is not None:
        monkeypatch.setattr(cce, "_ROW_CHUNK", chunk)
    ed = e.to(DEV).requires_grad_(True)
    cd = c.to(DEV).requires_grad_(True)
    loss, lse = cce.linear_cross_entropy(
        ed, cd, targets.to(DEV), filter_eps=eps, return_lse=True)
    total = loss.sum()
    if with_lse:
        total = total + lse_w * lse.sum()
    total.backward()
    return total.detach(), ed.grad, cd.grad


def _check(e, c, targets, eps, monkeypatch, chunk=None):
    loss_s, de_s, dc_s = _run("sparse", e, c, targets, eps, monkeypatch, chunk)
    loss_d, de_d, dc_d = _run("dense", e, c, targets, eps, monkeypatch, chunk)
    assert de_s.dtype == kr.BF16 and dc_s.dtype == kr.BF16
    n = int((targets != IGNORE).sum())
    rloss, rde, rdc = cce_e2e_ref(e, c, targets, eps)
    assert_close(loss_s / n, rloss, kr.TOL_CCE_LSE, "loss")
    assert_close(de_s, rde * n, TOL_CCE_DE_UNIT, "de sparse vs fp64")
    assert_close(dc_s, rdc * n, TOL_CCE_DC_UNIT, "dc sparse vs fp64")
    assert float(loss_s) == float(loss_d)
    # both routes multiply the same bf16 dlogits; they differ by the order of
    # the fp32 sums and one bf16 rounding of the result
    assert_close(de_s, de_d.double(), TOL_CCE_DE_UNIT, "de sparse vs dense")
    assert_close(dc_s, dc_d.double(), TOL_CCE_DC_UNIT, "dc sparse vs dense")
    return de_s, dc_s


def _ref(e, c, targets, eps, lse_w):
    """cce_e2e_ref's de and dc for loss.sum() + lse_w * lse.sum()."""
    e64, c64 = e.double(), c.double()
    z = e64 @ c64.t()
    p = torch.exp(z - torch.logsumexp(z, -1, keepdim=True))
    valid = (targets != IGNORE).double().unsqueeze(1)
    is_tgt = torch.arange(z.shape[1]).unsqueeze(0) == targets.unsqueeze(1)
    p = torch.where((p < eps) & ~is_tgt, torch.zeros_like(p), p)
    dz = p * (valid + lse_w) - is_tgt.double() * valid
    return dz @ c64, dz.t() @ e64


def _peaked(T, V, K, targets):
    """bf16 e, c with e rows along their target's classifier row, target
    logit 14: the other logits of a row are ~N(0, 1), every other p is below
    e^-9 < 2^-12, and only the target column survives the filter."""
    g = torch.Generator()
    g.manual_seed(77)
    c = (torch.randn(V, K, generator=g) * (0.5 / K ** 0.5)).to(kr.BF16)
    e = torch.randn(T, K, generator=g) * 0.5
    for r in range(T):
        t = int(targets[r])
        if t != IGNORE:
            e[r] = c[t].float() * (14.0 / float(c[t].float().pow(2).sum()))
    return e.to(kr.BF16), c


def _check_peaked(e, c, targets, monkeypatch, chunk=None):
    """Sparse and dense on a peaked case, with 0.25 * lse.sum() in the loss:
    p(target) is 0.998, so the loss alone leaves almost no gradient."""
    out_s = _run("sparse", e, c, targets, EPS, monkeypatch, chunk, with_lse=True)
    out_d = _run("dense", e, c, targets, EPS, monkeypatch, chunk, with_lse=True)
    rde, rdc = _ref(e, c, targets, EPS, 0.25)
    assert float(rde.abs().max()) > 10 * TOL_CCE_DE_UNIT["atol"]
    assert_close(out_s[1], rde, TOL_CCE_DE_UNIT, "de sparse vs fp64")
    assert_close(out_s[2], rdc, TOL_CCE_DC_UNIT, "dc sparse vs fp64")
    assert_close(out_s[1], out_d[1].double(), TOL_CCE_DE_UNIT, "de sparse vs dense")
    assert_close(out_s[2], out_d[2].double(), TOL_CCE_DC_UNIT, "dc sparse vs dense")
    return out_s[1], out_s[2]


@pytest.mark.parametrize("T,V,K", SHAPES)
def test_sparse_matches_reference(T, V, K, monkeypatch):
    e, c, targets = cce_case(T, V, K)
    _check(e, c, targets, EPS, monkeypatch)


@pytest.mark.parametrize("chunk", [64, 128])
def test_sparse_several_chunks(chunk, monkeypatch):
    e, c, targets = cce_case(200, 300, 128)
    _check(e, c, targets, EPS, monkeypatch, chunk=chunk)


def test_only_targets_survive(monkeypatch):
    """Only the target of each row is nonzero, the last partial vocab tile
    and the last partial row block included; most tiles are skipped."""
    T, V, K = 130, 1001, 192
    _, _, targets = cce_case(T, V, K)
    targets[targets == IGNORE] = 5
    targets[T - 1] = V - 1  # last row block, last (partial) vocab tile
    targets[64] = 0
    e, c = _peaked(T, V, K, targets)
    de, dc = _check_peaked(e, c, targets, monkeypatch)
    rows_hit = torch.zeros(V, dtype=torch.bool)
    rows_hit[targets[targets != IGNORE]] = True
    assert int((dc.cpu()[~rows_hit].float() != 0).sum()) == 0


def test_ignored_row_block_is_exact_zero(monkeypatch):
    T, V, K = 200, 300, 128
    e, c, targets = cce_case(T, V, K)
    targets[64:128] = IGNORE
    for chunk in (None, 64):
        de, dc = _check(e, c, targets, EPS, monkeypatch, chunk=chunk)
        assert int((de[64:128].cpu().float() != 0).sum()) == 0
        # the block adds nothing to dc: the same dc without its rows
        keep = torch.cat([torch.arange(0, 64), torch.arange(128, T)])
        _, _, dc_wo = _run("sparse", e[keep], c, targets[keep], EPS, monkeypatch, chunk=64)
        n_all, n_wo = int((targets != IGNORE).sum()), int((targets[keep] != IGNORE).sum())
        assert n_all == n_wo
        assert_close(dc, dc_wo.double(), TOL_CCE_DC_UNIT, "dc without the ignored block")


def test_vocab_tile_first_touched_by_a_later_chunk(monkeypatch):
    """Only targets are nonzero; the first chunk's targets stay below column
    128 and the later chunks' are in the last tile. The first chunk must set
    that tile of the accumulator to zero, and the later ones add to it."""
    T, V, K = 200, 300, 128
    targets = torch.empty(T, dtype=torch.int64)
    targets[:64] = torch.arange(64) % 100
    targets[64:] = 256 + torch.arange(T - 64) % 44
    e, c = _peaked(T, V, K, targets)
    _check_peaked(e, c, targets, monkeypatch, chunk=64)


def test_tiny_eps_sets_every_tile(monkeypatch):
    e, c, targets = cce_case(130, 1001, 192)
    _check(e, c, targets, 1e-30, monkeypatch)
    _check(e, c, targets, 1e-30, monkeypatch, chunk=64)


def test_dlse_supplied(monkeypatch):
    """loss - 0.25 * lse. The sign matters for what the tolerance can ask: the
    backward's p carries the rounding of its bf16 logit (3% at |logit| >= 8),
    and rtol is relative to the result. A positive lse weight cancels against
    the one-hot term at the planted rows and shrinks the result under that
    error; a negative one scales the softmax term to 0.75 and cancels nothing."""
    e, c, targets = cce_case(130, 1001, 192)
    out_s = _run("sparse", e, c, targets, EPS, monkeypatch, with_lse=True, lse_w=-0.25)
    out_d = _run("dense", e, c, targets, EPS, monkeypatch, with_lse=True, lse_w=-0.25)
    rde, rdc = _ref(e, c, targets, EPS, -0.25)
    assert_close(out_s[1], rde, TOL_CCE_DE_UNIT, "de with dlse vs fp64")
    assert_close(out_s[2], rdc, TOL_CCE_DC_UNIT, "dc with dlse vs fp64")
    assert_close(out_s[1], out_d[1].double(), TOL_CCE_DE_UNIT, "de with dlse vs dense")
    assert_close(out_s[2], out_d[2].double(), TOL_CCE_DC_UNIT, "dc with dlse vs dense")


def test_vocab_shard_with_offset(monkeypatch):
    """Local op on a shard whose first id is not 0: targets are global ids."""
    cce = _cce()
    T, V, K = 130, 1001, 192
    e, c, targets = cce_case(T, V, K)
    start = 4096
    shifted = torch.where(targets != IGNORE, targets + start, targets)
    outs = {}
    for route in ("sparse", "dense"):
        monkeypatch.setenv("D9D_CCE_BWD", route)
        ed = e.to(DEV).requires_grad_(True)
        cd = c.to(DEV).requires_grad_(True)
        loss, _ = cce._LinearCrossEntropyFunction.apply(
            ed, cd, shifted.to(DEV), None, start, start + V, EPS, None)
        loss.sum().backward()
        outs[route] = (loss.detach(), ed.grad, cd.grad)
    n = int((targets != IGNORE).sum())
    rloss, rde, rdc = cce_e2e_ref(e, c, targets, EPS)
    assert_close(outs["sparse"][1], rde * n, TOL_CCE_DE_UNIT, "shard de vs fp64")
    assert_close(outs["sparse"][2], rdc * n, TOL_CCE_DC_UNIT, "shard dc vs fp64")
    assert_close(outs["sparse"][1], outs["dense"][1].double(), TOL_CCE_DE_UNIT, "shard de")
    assert_close(outs["sparse"][2], outs["dense"][2].double(), TOL_CCE_DC_UNIT, "shard dc")


# ---- routing -------------------------------------------------------------------


class _Spy:
    """The extension with the new ops counted."""

    def __init__(self, ext):
        self._ext = ext
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._ext, name)
        if name in ("cce_dlogits_mask_", "cce_bwd_de", "cce_bwd_dc"):
            def wrapped(*a, **k):
                self.calls.append(name)
                return fn(*a, **k)
            return wrapped
        return fn


def _spy(monkeypatch):
    cce = _cce()
    spy = _Spy(_ext())
    monkeypatch.setattr(cce, "get_ext", lambda *a, **k: spy)
    return spy


def _backward(e, c, targets, **kw):
    cce = _cce()
    ed = e.to(DEV).requires_grad_(True)
    cd = c.to(DEV).requires_grad_(True)
    cce.linear_cross_entropy(ed, cd, targets.to(DEV), reduction="sum", **kw).backward()
    return ed.grad, cd.grad


def test_no_filter_and_softcap_keep_the_parent_code(monkeypatch):
    spy = _spy(monkeypatch)
    monkeypatch.setenv("D9D_CCE_BWD", "sparse")
    e, c, targets = cce_case(64, 128, 64)
    _backward(e, c, targets, filter_eps=None)
    _backward(e, c, targets, filter_eps=0.0)
    _backward(e, c, targets, softcap=30.0)
    _backward(e.float(), c.float(), targets)
    assert spy.calls == []
    _backward(e, c, targets)
    assert spy.calls == ["cce_dlogits_mask_", "cce_bwd_de", "cce_bwd_dc"]


def test_no_rows_returns_zeros(monkeypatch):
    monkeypatch.setenv("D9D_CCE_BWD", "sparse")
    e, c, targets = cce_case(64, 128, 64)
    de, dc = _backward(e[:0], c, targets[:0])
    assert de.shape == (0, 64) and dc.shape == c.shape
    assert int((dc != 0).sum()) == 0


def test_auto_is_dense_first_then_sparse(monkeypatch):
    cce = _cce()
    spy = _spy(monkeypatch)
    monkeypatch.setenv("D9D_CCE_BWD", "auto")
    monkeypatch.setattr(cce, "_router", cce._BwdRouter(threshold=0.5))
    T, V, K = 130, 1001, 192
    targets = torch.arange(T) % 100         # all in the first vocab tile: 3 of 24 tiles
    e, c = _peaked(T, V, K, targets)        # only targets survive
    _backward(e, c, targets)
    assert spy.calls == ["cce_dlogits_mask_"]   # dense GEMMs behind the masked dlogits
    torch.cuda.synchronize()                    # the count's event has completed
    spy.calls.clear()
    de_s, dc_s = _backward(e, c, targets)
    assert spy.calls == ["cce_dlogits_mask_", "cce_bwd_de", "cce_bwd_dc"]
    assert cce._router.density == pytest.approx(3 / 24)
    # and back to dense once the density is above the threshold
    cce._router.threshold = 0.05
    torch.cuda.synchronize()
    spy.calls.clear()
    _backward(e, c, targets)
    assert spy.calls == ["cce_dlogits_mask_"]


# ---- host checks ---------------------------------------------------------------


def test_new_ops_reject_bad_arguments():
    ext = _ext()
    R, V, K = 70, 300, 64
    d = torch.zeros(R, V, dtype=kr.BF16, device=DEV)
    e = torch.zeros(R, K, dtype=kr.BF16, device=DEV)
    c = torch.zeros(V, K, dtype=kr.BF16, device=DEV)
    de = torch.zeros(R, K, dtype=kr.BF16, device=DEV)
    dc = torch.zeros(V, K, dtype=kr.BF16, device=DEV)
    dc32 = dc.float()
    mask = torch.zeros(2, 3, dtype=torch.uint8, device=DEV)
    lse = torch.zeros(R, device=DEV)
    dl = torch.zeros(R, device=DEV)
    tg = torch.zeros(R, dtype=torch.int64, device=DEV)
    strided = torch.zeros(R, 2 * V, dtype=kr.BF16, device=DEV)[:, ::2]
    assert not strided.is_contiguous()

    def dlm(logits=d, lse=lse, tg=tg, dl=dl, dlse=None, mask=mask):
        return ext.cce_dlogits_mask_(logits, lse, tg, dl, dlse, mask, 0, IGNORE, EPS, True)

    bad_calls = [
        lambda: dlm(logits=d.float()),
        lambda: dlm(logits=strided),
        lambda: dlm(logits=d.cpu()),
        lambda: dlm(lse=lse.double()),
        lambda: dlm(lse=lse[:-1]),
        lambda: dlm(tg=tg.int()),
        lambda: dlm(dl=dl.bfloat16()),
        lambda: dlm(dlse=dl.double()),
        lambda: dlm(mask=mask.bool()),
        lambda: dlm(mask=mask[:, :2]),
        lambda: dlm(mask=torch.zeros(3, 3, dtype=torch.uint8, device=DEV)),
        lambda: dlm(mask=torch.zeros(3, 2, dtype=torch.uint8, device=DEV).t()),
        lambda: ext.cce_bwd_de(d.float(), c, mask, de),
        lambda: ext.cce_bwd_de(strided, c, mask, de),
        lambda: ext.cce_bwd_de(d, c[:-1], mask, de),
        lambda: ext.cce_bwd_de(d, c, mask.int(), de),
        lambda: ext.cce_bwd_de(d, c, mask[:1], de),
        lambda: ext.cce_bwd_de(d, c, mask, de.float()),
        lambda: ext.cce_bwd_de(d, c, mask, de[:-1]),
        lambda: ext.cce_bwd_de(d, c[:, :32].contiguous(), mask, de[:, :32].contiguous()),
        lambda: ext.cce_bwd_dc(d.float(), e, mask, dc, False),
        lambda: ext.cce_bwd_dc(d, e.float(), mask, dc, False),
        lambda: ext.cce_bwd_dc(d, e[:-1], mask, dc, False),
        lambda: ext.cce_bwd_dc(d, e, mask[:, :2], dc, False),
        lambda: ext.cce_bwd_dc(d, e, mask, dc.double(), False),
        lambda: ext.cce_bwd_dc(d, e, mask, dc[:-1], False),
        lambda: ext.cce_bwd_dc(d, e, mask, dc, True),
        lambda: ext.cce_bwd_dc(d, e, mask, dc32.t().contiguous().t(), False),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(RuntimeError, match="cce_"):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # and the good calls are accepted
    dlm()
    ext.cce_bwd_de(d, c, mask, de)
    ext.cce_bwd_dc(d, e, mask, dc, False)
    ext.cce_bwd_dc(d, e, mask, dc32, False)
    ext.cce_bwd_dc(d, e, mask, dc32, True)
    torch.cuda.synchronize()
