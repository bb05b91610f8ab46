"""CPU tests for the "square 256" head-dim route of the flash attention op."""

import pytest

from d9d_amd.ops.attention import head_dim_route


@pytest.mark.parametrize("dims", [(256, 256), (224, 200), (193, 256)])
def test_head_dim_route_square_256(dims):
    assert head_dim_route(*dims) == "square 256"


@pytest.mark.parametrize("dims", [(257, 256), (256, 257), (512, 512)])
def test_head_dim_route_rejects_above_256(dims):
    # the message names the old limit and the new range
    with pytest.raises(ValueError, match=r"192.*128.*193\.\.256"):
        head_dim_route(*dims)
