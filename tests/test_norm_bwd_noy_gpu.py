"""The y-free normalisation backward and the Adam kernel's beta1 == 0 / 16-byte form on the GPU (tests/norm_bwd_noy_checks.py)."""
import pytest
import torch

import norm_bwd_noy_checks as nc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("fixed_stats", [0, 1])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("act", sorted(nc.ACTS))
@pytest.mark.parametrize("shape", nc.NOY_SHAPES)
def test_modes_bit_equal(dev, shape, act, affine, fixed_stats):
    nc.check_modes_bit_equal(dev, shape, act, affine, fixed_stats)


@pytest.mark.parametrize("act", sorted(nc.ACTS))
@pytest.mark.parametrize("pc", [(37, 6), (300, 40)])
def test_kink(dev, pc, act):
    assert nc.check_kink(dev, pc[0], pc[1], act) >= pc[1]


@pytest.mark.parametrize("pc", [(37, 6), (1000, 40), (4100, 64)])
def test_values_against_fp64(dev, pc):
    nc.check_values(dev, *pc)


def test_bad_arguments(dev):
    nc.check_bad_args(dev)


@pytest.mark.parametrize("tick", [0, 1])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("beta1", [0.0, 0.5])
@pytest.mark.parametrize("n", nc.ADAM_NS)
def test_adam_range(dev, n, beta1, offset, tick):
    nc.check_adam_range(dev, n, beta1, offset, tick)
