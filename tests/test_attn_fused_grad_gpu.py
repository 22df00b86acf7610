"""The differentiable streaming few-shot attention (csrc/attention.hip, csrc/attention_bwd.hip) on the MI355X: the checks of
tests/test_attn_fused_grad_emu.py on hardware, the graphed training step with a real capture that holds the backward launches, and
the real size (hw = 128 x 128, two references) whose attention tensor would be 2 GiB."""
import pytest
import torch

import attn_fused_grad_checks as ag


def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    monkeypatch.delenv(ag.SWITCH, raising=False)
    monkeypatch.delenv(ag.af.SWITCH, raising=False)
    monkeypatch.delenv(ag.ab.SWITCH, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['small', 'prod', 'ragged'])
def test_forward_with_statistics(hip_lib, case):
    ag.check_forward_lse(dev(), case)


@pytest.mark.gpu
@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['small', 'prod', 'ragged'])
def test_gradients_against_float64(hip_lib, case, second):
    ag.check_gradients(dev(), case, second)


@pytest.mark.gpu
def test_forced_key_ranges_and_null_outputs(hip_lib):
    ag.check_splits(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('placement', ['first', 'last'])
def test_energies_in_the_hundreds(hip_lib, placement):
    ag.check_rescale(dev(), placement)


@pytest.mark.gpu
def test_same_bits_on_every_run(hip_lib):
    ag.check_determinism(dev())


@pytest.mark.gpu
def test_unsupported_shapes_fall_back(hip_lib):
    ag.check_fallback(dev())


@pytest.mark.gpu
def test_backward_entry_point_bounds(hip_lib):
    ag.check_bounds(dev())


@pytest.mark.gpu
def test_default_path_is_untouched(hip_lib):
    ag.check_default_path(dev())


@pytest.mark.gpu
def test_reference_fixture_step_with_both_switches(hip_lib):
    ag.check_fixture_step(dev())


@pytest.mark.gpu
def test_tiny_nshot3_step(hip_lib):
    ag.check_tiny_step(dev())


@pytest.mark.gpu
def test_graphed_step_captures_the_backward(hip_lib):
    ag.check_graphed_capture(dev())


@pytest.mark.gpu
def test_graphed_step_replays_the_backward(hip_lib):
    """bit for bit against the eager loop, in the fixed-order mode"""
    ag.check_graphed_step(dev())


@pytest.mark.gpu
def test_real_size_without_the_attention_tensor(hip_lib):
    ag.check_real_size(dev())
