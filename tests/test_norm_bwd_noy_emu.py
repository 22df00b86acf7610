"""The y-free normalisation backward and the Adam kernel's beta1 == 0 / 16-byte form on the SIMT emulator (tests/norm_bwd_noy_checks.py)."""
import pytest
import torch

import norm_bwd_noy_checks as nc

DEV = torch.device("cpu")


@pytest.mark.parametrize("fixed_stats", [0, 1])
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("act", sorted(nc.ACTS))
@pytest.mark.parametrize("shape", nc.NOY_SHAPES)
def test_modes_bit_equal(emu_lib, shape, act, affine, fixed_stats):
    nc.check_modes_bit_equal(DEV, shape, act, affine, fixed_stats)


@pytest.mark.parametrize("act", sorted(nc.ACTS))
@pytest.mark.parametrize("pc", [(37, 6), (300, 40)])
def test_kink(emu_lib, pc, act):
    assert nc.check_kink(DEV, pc[0], pc[1], act) >= pc[1]


@pytest.mark.parametrize("pc", [(37, 6), (1000, 40), (4100, 64)])
def test_values_against_fp64(emu_lib, pc):
    nc.check_values(DEV, *pc)


def test_bad_arguments(emu_lib):
    nc.check_bad_args(DEV)


@pytest.mark.parametrize("tick", [0, 1])
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("beta1", [0.0, 0.5])
@pytest.mark.parametrize("n", nc.ADAM_NS)
def test_adam_range(emu_lib, n, beta1, offset, tick):
    nc.check_adam_range(DEV, n, beta1, offset, tick)


def test_model_step_with_and_without_y(emu_lib):
    """one D + G step of the small fixture of test_model_emu.py with ops.norm_bwd_from_x on and off: bit-equal losses and gradients"""
    nc.check_model_step(DEV)
