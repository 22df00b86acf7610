"""The streaming few-shot attention (few-shot-vid2vid_amd/csrc/attention.hip) on the MI355X: the checks of
tests/test_attn_fused_emu.py on hardware - the kept session with a real capture that holds the fused launch - and the real size
(hw = 128 x 128, three references) that the banded code needs a 2 GiB buffer for."""
import pytest
import torch

import attn_fused_checks as af


def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    monkeypatch.delenv(af.SWITCH, raising=False)
    monkeypatch.delenv(af.ab.SWITCH, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['small', 'prod', 'ragged'])
def test_fused_attention_against_float64(hip_lib, case, second):
    af.check_operator(dev(), case, second)


@pytest.mark.gpu
@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['wide', 'two_walks'])
def test_more_output_tiles_than_one_walk(hip_lib, case, second):
    af.check_walks(dev(), case, second)


@pytest.mark.gpu
def test_key_ranges_and_finishing_pass(hip_lib):
    af.check_splits(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('placement', ['first', 'last'])
def test_online_softmax_rescaling(hip_lib, placement):
    af.check_rescale(dev(), placement)


@pytest.mark.gpu
def test_same_bits_on_every_run(hip_lib):
    af.check_determinism(dev())


@pytest.mark.gpu
def test_default_path_is_untouched(hip_lib):
    af.check_default_path(dev())


@pytest.mark.gpu
def test_unsupported_shape_falls_back(hip_lib):
    af.check_fallback(dev())


@pytest.mark.gpu
def test_entry_point_bounds(hip_lib):
    af.check_bounds(dev())


@pytest.mark.gpu
def test_reference_fixture_step_with_fused_d_pass(hip_lib):
    af.check_fixture_step(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mul', 'concat'])
def test_fused_kept_session(hip_lib, name):
    af.check_session(dev(), name)


@pytest.mark.gpu
def test_real_size_without_the_attention_tensor(hip_lib):
    af.check_real_size(dev())
