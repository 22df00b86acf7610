"""Frozen-weight inference (few-shot-vid2vid_amd/infer.py) on the emulator: the operator-level checks at the shapes of the hardware
tests, the session against the eager path bit for bit (the "graph" is the same body re-run on the static buffers), and the launch
accounting of a steady frame from the emulator's per-kernel counter."""
import ctypes

import pytest
import torch

import infer_session_checks as ic

DEV = torch.device('cpu')


def _launches(emu_lib):
    fn = emu_lib.get_lib().fsv_emu_launch_count
    fn.restype = ctypes.c_longlong
    return lambda: int(fn())


# ---- operator level
@pytest.mark.parametrize('cout,cin,k,nbatch', ic.COL_SCALE_SHAPES)
def test_col_scale_layout_is_bit_equal_to_torch_emu(emu_lib, cout, cin, k, nbatch):
    ic.check_col_scale(DEV, cout, cin, k, nbatch)


def test_col_scale_bad_arguments_emu(emu_lib):
    ic.check_col_scale_bad_args(DEV, _launches(emu_lib))


def test_image_u8_matches_tensor2im_emu(emu_lib):
    ic.check_image_u8(DEV)


@pytest.mark.parametrize('cout,stride,spectral,bias', ic.FOLD_CASES)
def test_folded_launch_against_float64_emu(emu_lib, cout, stride, spectral, bias):
    ic.check_fold_launch(DEV, cout, stride, spectral, bias, report=ic.emu_report)


# ---- session level
@pytest.mark.parametrize('case', ic.FIXTURES)
def test_session_equals_eager_on_fixture_emu(emu_lib, case):
    ic.check_fixture_bits(case, DEV, ic.emu_report)


def test_session_equals_eager_nshot2_emu(emu_lib):
    ic.check_tiny_bits(DEV, ic.NSHOT2, 330, b=2)


def test_session_equals_eager_ring_depth2_emu(emu_lib):
    ic.check_tiny_bits(DEV, ic.RING2, 340)


def test_two_sequences_emu(emu_lib):
    ic.check_two_sequences('pose_combine', DEV, ic.emu_report)


def test_steady_frame_launch_accounting_emu(emu_lib):
    ic.check_launch_accounting(DEV, ic.emu_report)


def test_fold_norms_model_level_emu(emu_lib):
    ic.check_fold_model(DEV, ic.emu_report)


def test_fold_norms_nothing_to_fold_emu(emu_lib):
    ic.check_fold_nothing_to_fold(DEV)


def test_nothing_leaks_after_close_emu(emu_lib):
    ic.check_nothing_leaks(DEV)


def test_refreeze_follows_new_weights_emu(emu_lib):
    ic.check_refreeze(DEV)


def test_finetune_through_session_emu(emu_lib):
    ic.check_finetune(DEV)


def test_session_refuses_train_mode_emu(emu_lib):
    ic.check_refusals(DEV)
