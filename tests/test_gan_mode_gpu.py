"""--gan_mode ls / original / w on the MI355X: the GANLoss reduction (csrc/losses.hip) against float64 with the bar from torch's own
fp32 error (both evaluated on the device), the hinge path bit-equal, bad arguments, the reference step fixtures and the temporal
fixture, and graphed replay against the eager loop in the fixed-order mode."""
import pytest
import torch

import gan_mode_checks as gm
import graph_step_checks as gc


@pytest.mark.gpu
@pytest.mark.parametrize('n', gm.SIZES)
@pytest.mark.parametrize('real', [True, False])
@pytest.mark.parametrize('mode', gm.MODES)
def test_gan_loss_against_float64(hip_lib, mode, real, n):
    gm.check_kernel(torch.device('cuda:0'), gm.inputs((n,), 11 + n % 13), real, mode, ref_device='cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('shape,nhwc', [((2, 1, 3, 5), False), ((2, 4, 3, 5), True)])
@pytest.mark.parametrize('real', [True, False])
@pytest.mark.parametrize('mode', gm.MODES)
def test_gan_loss_against_float64_4d(hip_lib, mode, real, shape, nhwc):
    gm.check_kernel(torch.device('cuda:0'), gm.inputs(shape, 17, nhwc), real, mode, ref_device='cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('n', [257, 512 * 256 + 3])
def test_hinge_mode_is_hinge_loss(hip_lib, n):
    gm.check_hinge_untouched(torch.device('cuda:0'), n)


@pytest.mark.gpu
def test_bad_arguments(hip_lib):
    gm.check_bad_arguments(torch.device('cuda:0'))


@pytest.mark.gpu
@pytest.mark.parametrize('case', gm.STEP_CASES)
def test_step_reproduces_reference_iteration_on_gpu(hip_lib, case):
    gm.check_step(torch.device('cuda:0'), case)


@pytest.mark.gpu
def test_temporal_second_frame_reproduces_reference_on_gpu(hip_lib):
    gm.check_temporal(torch.device('cuda:0'))


@pytest.mark.gpu
def test_graphed_replay_equals_eager_gan_mode(hip_lib, monkeypatch):
    """fixed-order mode, --gan_mode original: the captured iteration replays the eager loop bit for bit over four iterations"""
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    dev = torch.device('cuda:0')
    ref, pG, pD, _ = gc._run(dev, False, 4, 500, gm.KW)
    got, qG, qD, step = gc._run(dev, True, 4, 500, gm.KW)
    assert any(e.graphs is not None for e in step.entries.values()), 'nothing was captured'
    for it, (a, b) in enumerate(zip(ref, got)):
        assert a['d'] == b['d'] and a['g'] == b['g'], (it, a['d'], b['d'], a['g'], b['g'])
        assert torch.equal(a['img'], b['img']), it
    assert torch.equal(pG, qG) and torch.equal(pD, qD)
