"""Frozen-weight inference (few-shot-vid2vid_amd/infer.py) on the MI355X: the operator-level checks of tests/test_infer_session_emu.py
at the same shapes, and the session with REAL captures - one hipGraph per configuration, replayed across frames and sequences -
against the eager path bit for bit in the fixed-order mode."""
import pytest
import torch

import infer_session_checks as ic


def dev():
    return torch.device('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('cout,cin,k,nbatch', ic.COL_SCALE_SHAPES)
def test_col_scale_layout_is_bit_equal_to_torch(hip_lib, cout, cin, k, nbatch):
    ic.check_col_scale(dev(), cout, cin, k, nbatch)


@pytest.mark.gpu
def test_col_scale_bad_arguments(hip_lib):
    ic.check_col_scale_bad_args(dev())


@pytest.mark.gpu
def test_image_u8_matches_tensor2im(hip_lib):
    ic.check_image_u8(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('cout,stride,spectral,bias', ic.FOLD_CASES)
def test_folded_launch_against_float64(hip_lib, cout, stride, spectral, bias):
    ic.check_fold_launch(dev(), cout, stride, spectral, bias)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ic.FIXTURES)
def test_session_equals_eager_on_fixture(hip_lib, monkeypatch, case):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_fixture_bits(case, dev())


@pytest.mark.gpu
def test_session_equals_eager_nshot2(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_tiny_bits(dev(), ic.NSHOT2, 330, b=2)


@pytest.mark.gpu
def test_session_equals_eager_ring_depth2(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_tiny_bits(dev(), ic.RING2, 340)


@pytest.mark.gpu
def test_two_sequences_one_capture(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_two_sequences('pose_combine', dev())


@pytest.mark.gpu
def test_fold_norms_model_level(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_fold_model(dev())


@pytest.mark.gpu
def test_fold_norms_nothing_to_fold(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_fold_nothing_to_fold(dev())


@pytest.mark.gpu
def test_nothing_leaks_after_close(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_nothing_leaks(dev())


@pytest.mark.gpu
def test_refreeze_follows_new_weights(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    ic.check_refreeze(dev())


@pytest.mark.gpu
def test_finetune_through_session(hip_lib):
    ic.check_finetune(dev())


@pytest.mark.gpu
def test_session_refuses_train_mode(hip_lib):
    ic.check_refusals(dev())
