"""The adaptation-target kernel of the test-time finetune (csrc/roll_flip.hip, ops.roll_flip) on the MI355X."""
import pytest
import torch

import finetune_graph_checks as fc

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


# ---- (a) the kernel
@pytest.mark.parametrize('h,w', fc.SIZES)
def test_roll_flip_equals_cat_and_flip(hip_lib, h, w):
    fc.check_roll_flip(dev(), h, w)


def test_roll_flip_reads_its_parameters_on_the_device(hip_lib):
    fc.check_params_are_read_on_the_device(dev())


def test_roll_flip_clamps_out_of_range_parameters(hip_lib):
    fc.check_out_of_range_params(dev())


def test_roll_flip_refusals(hip_lib):
    fc.check_refusals(dev())
