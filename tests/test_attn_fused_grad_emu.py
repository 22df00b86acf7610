"""The differentiable streaming few-shot attention (fsv_attention_fused_fwd_lse, fsv_attention_fused_bwd, ops.attention_fused_grad,
FSV_ATTN_FUSED_GRAD) on the emulator: the forward with statistics, the gradients against float64, forced key ranges and NULL
outputs, energies in the hundreds, determinism, fallback and bounds, the untouched default path and the step level.  The graphed
step and the real size run on hardware only (tests/test_attn_fused_grad_gpu.py)."""
import pytest
import torch

import attn_fused_grad_checks as ag

DEV = torch.device('cpu')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    monkeypatch.delenv(ag.SWITCH, raising=False)
    monkeypatch.delenv(ag.af.SWITCH, raising=False)
    monkeypatch.delenv(ag.ab.SWITCH, raising=False)


@pytest.mark.parametrize('case', ['small', 'prod', 'ragged'])
def test_forward_with_statistics_emu(emu_lib, case):
    ag.check_forward_lse(DEV, case)


@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['small', 'prod', 'ragged'])
def test_gradients_against_float64_emu(emu_lib, case, second):
    ag.check_gradients(DEV, case, second)


def test_forced_key_ranges_and_null_outputs_emu(emu_lib):
    ag.check_splits(DEV)


@pytest.mark.parametrize('placement', ['first', 'last'])
def test_energies_in_the_hundreds_emu(emu_lib, placement):
    ag.check_rescale(DEV, placement)


def test_same_bits_on_every_run_emu(emu_lib):
    ag.check_determinism(DEV)


def test_unsupported_shapes_fall_back_emu(emu_lib):
    ag.check_fallback(DEV)


def test_backward_entry_point_bounds_emu(emu_lib):
    ag.check_bounds(DEV)


def test_default_path_is_untouched_emu(emu_lib):
    ag.check_default_path(DEV)


def test_reference_fixture_step_with_both_switches_emu(emu_lib):
    ag.check_fixture_step(DEV)


def test_tiny_nshot3_step_emu(emu_lib):
    ag.check_tiny_step(DEV)
