"""The kept reference side of n_shot > 1 sequences (few-shot-vid2vid_amd/infer.py `keep_references`, `inputs_u8`) on the MI355X: the two
widened kernels at the shapes of tests/test_infer_nshot_emu.py, and the kept session with a REAL capture - one hipGraph, replayed across
frames and across two sequences - against the eager path in the fixed-order mode."""
import pytest
import torch

import infer_nshot_checks as nc


def dev():
    return torch.device('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('scale', nc.GSUM_SCALES)
@pytest.mark.parametrize('rows,c,groups', nc.GSUM_SHAPES)
def test_softmax_group_sums_against_float64(hip_lib, rows, c, groups, scale):
    nc.check_softmax_gsum(dev(), rows, c, groups, scale)


@pytest.mark.gpu
def test_softmax_group_sums_bad_arguments(hip_lib):
    nc.check_softmax_gsum_bad_args(dev())


@pytest.mark.gpu
def test_image_from_u8_matches_torch(hip_lib):
    nc.check_image_from_u8(dev())


@pytest.mark.gpu
def test_from_u8_refuses_misaligned_buffers(hip_lib):
    nc.check_from_u8_alignment(dev())


@pytest.mark.gpu
def test_kept_session_equals_eager(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    nc.check_frames('mul', dev())


@pytest.mark.gpu
def test_two_sequences_one_capture(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    nc.check_two_sequences(dev())


@pytest.mark.gpu
def test_inputs_u8_equal_converted_inputs(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    nc.check_inputs_u8(dev())
