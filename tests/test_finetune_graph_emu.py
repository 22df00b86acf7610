"""The adaptation-target kernel of the test-time finetune (csrc/roll_flip.hip, ops.roll_flip) on the emulator."""
import pytest
import torch

import finetune_graph_checks as fc

DEV = torch.device('cpu')


# ---- (a) the kernel
@pytest.mark.parametrize('h,w', fc.SIZES)
def test_roll_flip_equals_cat_and_flip_emu(emu_lib, h, w):
    fc.check_roll_flip(DEV, h, w)


def test_roll_flip_reads_its_parameters_on_the_device_emu(emu_lib):
    fc.check_params_are_read_on_the_device(DEV)


def test_roll_flip_clamps_out_of_range_parameters_emu(emu_lib):
    fc.check_out_of_range_params(DEV)


def test_roll_flip_refusals_emu(emu_lib):
    fc.check_refusals(DEV)
