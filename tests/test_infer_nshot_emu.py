"""The kept reference side of n_shot > 1 sequences (few-shot-vid2vid_amd/infer.py `keep_references`, `inputs_u8`) on the emulator:
the two widened kernels at the shapes of the hardware tests, the kept session against the eager path frame for frame (the "graph" is
the same body re-run on the static buffers), what the session owns, and the launch accounting of a kept steady frame."""
import pytest
import torch

import infer_nshot_checks as nc
import infer_session_checks as ic

DEV = torch.device('cpu')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')


# ---- operator level
@pytest.mark.parametrize('scale', nc.GSUM_SCALES)
@pytest.mark.parametrize('rows,c,groups', nc.GSUM_SHAPES)
def test_softmax_group_sums_against_float64_emu(emu_lib, rows, c, groups, scale):
    nc.check_softmax_gsum(DEV, rows, c, groups, scale)


def test_softmax_group_sums_bad_arguments_emu(emu_lib):
    nc.check_softmax_gsum_bad_args(DEV)


def test_image_from_u8_matches_torch_emu(emu_lib):
    nc.check_image_from_u8(DEV)


def test_from_u8_refuses_misaligned_buffers_emu(emu_lib):
    nc.check_from_u8_alignment(DEV)


# ---- session level
@pytest.mark.parametrize('name', sorted(nc.CONFIGS))
def test_kept_session_equals_eager_emu(emu_lib, name):
    nc.check_frames(name, DEV, ic.emu_report)


def test_kept_session_with_fold_norms_emu(emu_lib):
    nc.check_fold_norms(DEV)


def test_inputs_u8_equal_converted_inputs_emu(emu_lib):
    nc.check_inputs_u8(DEV)


def test_two_sequences_refill_in_place_emu(emu_lib):
    nc.check_two_sequences(DEV)


def test_steady_frames_do_not_read_the_references_emu(emu_lib):
    nc.check_steady_references_are_not_read(DEV)


def test_refreeze_drops_the_kept_references_emu(emu_lib):
    nc.check_refreeze(DEV)


def test_close_leaves_nothing_on_the_model_emu(emu_lib):
    nc.check_close(DEV)


def test_finetune_with_kept_references_emu(emu_lib):
    nc.check_finetune(DEV)


def test_kept_frame_launch_accounting_emu(emu_lib):
    nc.check_launch_accounting(DEV, ic.emu_report)
