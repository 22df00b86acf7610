"""The attention of n_shot > 1 in query bands (few-shot-vid2vid_amd/networks.py attention_band_plan) on the MI355X: the checks of
tests/test_attn_band_emu.py on hardware - the kept session with a real capture that contains the band launches - and the two sizes
past 2 GiB that the unbanded code refuses."""
import pytest
import torch

import attn_band_checks as ab


def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    monkeypatch.delenv(ab.SWITCH, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
@pytest.mark.parametrize('mode', sorted(ab.FORCED))
def test_banded_attention_against_float64(hip_lib, mode, grad):
    ab.check_operator(dev(), mode, grad)


@pytest.mark.gpu
@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
def test_second_feature_map_not_announced(hip_lib, grad):
    ab.check_operator(dev(), 'uneven', grad, announce=False)


@pytest.mark.gpu
def test_default_path_issues_the_unbanded_launches(hip_lib):
    ab.check_default_path(dev())


@pytest.mark.gpu
def test_host_side_bounds(hip_lib):
    ab.check_host_bounds(dev())


@pytest.mark.gpu
def test_reference_fixture_step_in_bands(hip_lib):
    ab.check_fixture_step(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('banded', [True, False], ids=['banded', 'unbanded'])
def test_tiny_nshot3_step(hip_lib, banded):
    ab.check_tiny_step(dev(), banded)


@pytest.mark.gpu
def test_kept_session_in_bands(hip_lib):
    ab.check_session(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(ab.REAL_CASES))
def test_attention_past_two_gib(hip_lib, name):
    ab.check_real_limit(dev(), name)
