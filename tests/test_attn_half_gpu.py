"""The streaming few-shot attention on the f16 matrix cores (few-shot-vid2vid_amd/csrc/attention_h.hip) on the MI355X: the checks of
tests/test_attn_half_emu.py on hardware, the kept session with a real capture that holds the half launch.  The shapes are the
small ones of attn_half_checks; the real size is measured and compared by tools/attn_half.py."""
import pytest
import torch

import attn_half_checks as ah


def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    for k in (ah.SWITCH, ah.af.SWITCH, ah.ab.SWITCH):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.gpu
def test_half_prep_is_bit_exact(hip_lib):
    ah.check_prep(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['small', 'c24', 'ragged', 'prod'])
def test_half_attention_against_float64(hip_lib, case, second):
    ah.check_operator(dev(), case, second)


@pytest.mark.gpu
def test_low_parts_of_the_split(hip_lib):
    ah.check_offset(dev())


@pytest.mark.gpu
def test_half_key_ranges_and_finishing_pass(hip_lib):
    ah.check_splits(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('placement', ['first', 'last'])
def test_half_online_softmax_rescaling(hip_lib, placement):
    ah.check_rescale(dev(), placement)


@pytest.mark.gpu
def test_half_same_bits_on_every_run(hip_lib):
    ah.check_determinism(dev())


@pytest.mark.gpu
def test_half_switch_leaves_the_default_path(hip_lib):
    ah.check_default_path(dev())


@pytest.mark.gpu
def test_half_entry_point_bounds(hip_lib):
    ah.check_bounds(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mul', 'concat'])
def test_half_kept_session(hip_lib, name):
    ah.check_session(dev(), name)
