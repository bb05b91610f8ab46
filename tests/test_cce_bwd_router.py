"""The CCE backward's route state machine, without a GPU: first call, count
not yet ready, threshold crossing, env override, and which calls never reach
the tile kernels."""

import pytest
import torch

from d9d_amd.ops import cce


class _Event:
    """Stands in for torch.cuda.Event: done when the test says so."""

    def __init__(self):
        self.done = False
        self.recorded = False

    def record(self):
        self.recorded = True

    def query(self):
        return self.done


@pytest.fixture
def router(monkeypatch):
    monkeypatch.delenv("D9D_CCE_BWD", raising=False)
    events = []

    def new_event():
        events.append(_Event())
        return events[-1]

    r = cce._BwdRouter(threshold=0.25, new_event=new_event)
    r.events = events
    monkeypatch.setattr(cce, "_router", r)
    return r


def test_first_call_is_dense(router):
    assert router.decide() == "dense"
    assert router.density is None


def test_keeps_its_decision_until_the_count_has_arrived(router):
    router.record(torch.tensor(10), 100)
    assert router.events[0].recorded
    assert router.decide() == "dense"          # event not complete: no read
    assert router.density is None
    router.events[0].done = True
    assert router.decide() == "sparse"         # 10% <= 25%
    assert router.density == pytest.approx(0.10)
    # a second count while one is in flight is dropped, not queued
    router.record(torch.tensor(90), 100)
    router.record(torch.tensor(1), 100)
    assert len(router.events) == 2
    assert router.decide() == "sparse"
    router.events[1].done = True
    assert router.decide() == "dense"          # 90% > 25%
    assert router.density == pytest.approx(0.90)


def test_threshold_is_inclusive_and_crossed_both_ways(router):
    for count, want in [(25, "sparse"), (26, "dense"), (0, "sparse")]:
        router.record(torch.tensor(count), 100)
        router.events[-1].done = True
        assert router.decide() == want


def test_nothing_to_record(router):
    router.record(None, 0)                     # a backward with no rows
    assert router.events == []
    assert router.decide() == "dense"


def test_env_forces_the_route(router, monkeypatch):
    monkeypatch.setenv("D9D_CCE_BWD", "sparse")
    assert router.decide() == "sparse"
    assert cce._bwd_route(True, 2.0 ** -12, 768) == "sparse"
    monkeypatch.setenv("D9D_CCE_BWD", "dense")
    assert router.decide() == "dense"
    assert cce._bwd_route(True, 2.0 ** -12, 768) == "parent"   # no mask either
    monkeypatch.setenv("D9D_CCE_BWD", "auto")
    assert cce._bwd_route(True, 2.0 ** -12, 768) == "dense"    # masked, feeds the router
    assert router.route == "dense"             # forcing left the state alone
    monkeypatch.setenv("D9D_CCE_BWD", "fast")
    with pytest.raises(ValueError, match="D9D_CCE_BWD"):
        router.decide()


def test_calls_that_never_reach_the_tile_kernels(router, monkeypatch):
    monkeypatch.setenv("D9D_CCE_BWD", "sparse")
    assert cce._bwd_route(False, 2.0 ** -12, 768) == "parent"  # eager: CPU, fp32, softcap
    assert cce._bwd_route(True, 0.0, 768) == "parent"          # no filter, no zeros
    assert cce._bwd_route(True, None, 768) == "parent"
    assert cce._bwd_route(True, 2.0 ** -12, 96) == "parent"    # hidden % 64
    assert cce._bwd_route(True, 2.0 ** -12, 2048) == "parent"  # hidden > 1024
    assert cce._bwd_route(True, 2.0 ** -12, 1024) == "sparse"


def test_cpu_backward_is_unchanged(router, monkeypatch):
    """CPU tensors take the eager path whatever the env says, and record nothing."""
    monkeypatch.setenv("D9D_CCE_BWD", "sparse")
    g = torch.Generator().manual_seed(0)
    e = torch.randn(9, 64, generator=g, requires_grad=True)
    c = torch.randn(40, 64, generator=g, requires_grad=True)
    t = torch.randint(0, 40, (9,), generator=g)
    cce.linear_cross_entropy(e, c, t, reduction="mean").backward()
    ref = torch.nn.functional.cross_entropy(e.detach() @ c.detach().t(), t)
    assert router.events == []
    e2 = e.detach().clone().requires_grad_(True)
    c2 = c.detach().clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(e2 @ c2.t(), t).backward()
    torch.testing.assert_close(e.grad, e2.grad, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(c.grad, c2.grad, rtol=1e-4, atol=1e-5)
    assert torch.isfinite(ref)
