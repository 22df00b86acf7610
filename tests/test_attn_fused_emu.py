"""The streaming few-shot attention (few-shot-vid2vid_amd/csrc/attention.hip, ops.attention_fused, FSV_ATTN_FUSED,
InferenceSession(fused_attention=True)) on the emulator: the operator against float64, the online-softmax rescaling, determinism,
the untouched default path, fallback and bounds, the step level and the kept session.  The real size runs on hardware only
(tests/test_attn_fused_gpu.py)."""
import pytest
import torch

import attn_fused_checks as af

DEV = torch.device('cpu')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    monkeypatch.delenv(af.SWITCH, raising=False)
    monkeypatch.delenv(af.ab.SWITCH, raising=False)


@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['small', 'prod', 'ragged'])
def test_fused_attention_against_float64_emu(emu_lib, case, second):
    af.check_operator(DEV, case, second)


@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['wide', 'two_walks'])
def test_more_output_tiles_than_one_walk_emu(emu_lib, case, second):
    af.check_walks(DEV, case, second)


def test_key_ranges_and_finishing_pass_emu(emu_lib):
    af.check_splits(DEV)


@pytest.mark.parametrize('placement', ['first', 'last'])
def test_online_softmax_rescaling_emu(emu_lib, placement):
    af.check_rescale(DEV, placement)


def test_same_bits_on_every_run_emu(emu_lib):
    af.check_determinism(DEV)


def test_default_path_is_untouched_emu(emu_lib):
    af.check_default_path(DEV)


def test_unsupported_shape_falls_back_emu(emu_lib):
    af.check_fallback(DEV)


def test_entry_point_bounds_emu(emu_lib):
    af.check_bounds(DEV)


def test_reference_fixture_step_with_fused_d_pass_emu(emu_lib):
    af.check_fixture_step(DEV)


@pytest.mark.parametrize('name', ['mul', 'concat'])
def test_fused_kept_session_emu(emu_lib, name):
    af.check_session(DEV, name)
