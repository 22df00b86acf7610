"""--norm_G spectralspadeinstance / --norm_F spectralinstance / spectralnone on the MI355X: the SPADE kernels with per-sample
statistics against float64 (shapes and bars of tests/test_norm_instance_emu.py), the grouped statistics epilogue of
csrc/spade_conv3.hip, the reference step and inference fixtures, eval() against train(), and graphed replay against the eager loop."""
import pytest
import torch

import graph_step_checks as gc
import norm_instance_checks as ni


def dev():
    return torch.device('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('act', [True, False])
@pytest.mark.parametrize('up', [False, True])
@pytest.mark.parametrize('chs,per_sample', [((4,), True), ((12,), False), ((4, 12, 4), True), ((12, 4, 12), False)])
@pytest.mark.parametrize('c', [16, 20])
def test_spade_instance_ragged_tile(hip_lib, c, chs, per_sample, up, act):
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_instance(dev(), c=c, chs=chs, per_sample=per_sample, h=h, w=w, up=up, act=act, bwd='twin')


@pytest.mark.gpu
@pytest.mark.parametrize('up', [False, True])
@pytest.mark.parametrize('c', [16, 20])
def test_spade_instance_tile_walk(hip_lib, c, up):
    ni.check_spade_instance(dev(), c=c, chs=(4, 12), per_sample=True, h=24, w=20, up=up, act=True, bwd='twin', max_gx=1)


@pytest.mark.gpu
@pytest.mark.parametrize('up', [False, True])
@pytest.mark.parametrize('chs,per_sample', [((4,), True), ((12, 4, 12), False)])
def test_spade_instance_elementwise_backward(hip_lib, chs, per_sample, up):
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_instance(dev(), c=16, chs=chs, per_sample=per_sample, h=h, w=w, up=up, act=True, bwd='elem')


@pytest.mark.gpu
@pytest.mark.parametrize('up', [False, True])
def test_spade_instance_k3(hip_lib, up):
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_instance(dev(), c=16, chs=(4, 12), per_sample=True, h=h, w=w, up=up, act=True, k=3)


@pytest.mark.gpu
def test_spade_instance_ignores_mode_and_buffers(hip_lib):
    ni.check_spade_instance_eval_and_buffers(dev())


@pytest.mark.gpu
@pytest.mark.parametrize('up', [False, True])
def test_spade_conv_s_instance(hip_lib, up):
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_conv_s_instance(dev(), h=h, w=w, up=up)


@pytest.mark.gpu
@pytest.mark.parametrize('up', [False, True])
def test_spade_conv3_instance_and_grouped_statistics(hip_lib, up):
    ni.check_spade_conv3_instance(dev(), up=up)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ni.STEP_CASES)
def test_step_reproduces_reference_iteration_on_gpu(hip_lib, case):
    ni.check_step(dev(), case)


@pytest.mark.gpu
def test_inference_reproduces_reference_on_gpu(hip_lib):
    ni.check_inference(dev())


@pytest.mark.gpu
def test_eval_equals_train_bit_for_bit(hip_lib):
    ni.check_eval_equals_train(dev())


@pytest.mark.gpu
def test_graphed_replay_equals_eager_instance_norm(hip_lib, monkeypatch):
    """fixed-order mode, instance-normalised pose_combine configuration: the captured iteration replays the eager loop bit for bit"""
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    kw = dict(ni.KW, warp_ref=True, spade_combine=True)
    ref, pG, pD, _ = gc._run(dev(), False, 4, 500, kw)
    got, qG, qD, step = gc._run(dev(), True, 4, 500, kw)
    assert any(e.graphs is not None for e in step.entries.values()), 'nothing was captured'
    for it, (a, b) in enumerate(zip(ref, got)):
        assert a['d'] == b['d'] and a['g'] == b['g'], (it, a['d'], b['d'], a['g'], b['g'])
        assert torch.equal(a['img'], b['img']), it
    assert torch.equal(pG, qG) and torch.equal(pD, qD)
