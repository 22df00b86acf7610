"""The attention of n_shot > 1 in query bands (few-shot-vid2vid_amd/networks.py attention_band_plan) on the emulator: the operator
against float64 under forced band sizes, the default path launch for launch, the band rule and the host-side bounds, the step level
and the kept session.  The sizes past 2 GiB themselves run on hardware only (tests/test_attn_band_gpu.py)."""
import pytest
import torch

import attn_band_checks as ab

DEV = torch.device('cpu')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    monkeypatch.delenv(ab.SWITCH, raising=False)


@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
@pytest.mark.parametrize('mode', sorted(ab.FORCED))
def test_banded_attention_against_float64_emu(emu_lib, mode, grad):
    ab.check_operator(DEV, mode, grad)


@pytest.mark.parametrize('grad', [False, True], ids=['no_grad', 'grad'])
def test_second_feature_map_not_announced_emu(emu_lib, grad):
    ab.check_operator(DEV, 'uneven', grad, announce=False)


def test_default_path_issues_the_unbanded_launches_emu(emu_lib):
    ab.check_default_path(DEV)


def test_band_rule_at_the_launch_bound(emu_lib):
    ab.check_band_rule()


def test_host_side_bounds_emu(emu_lib):
    ab.check_host_bounds(DEV)


def test_reference_fixture_step_in_bands_emu(emu_lib):
    ab.check_fixture_step(DEV)


@pytest.mark.parametrize('banded', [True, False], ids=['banded', 'unbanded'])
def test_tiny_nshot3_step_emu(emu_lib, banded):
    ab.check_tiny_step(DEV, banded)


def test_kept_session_in_bands_emu(emu_lib):
    ab.check_session(DEV)
