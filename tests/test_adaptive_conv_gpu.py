"""--use_label_ref concat / --adaptive_conv on the MI355X: the pooled-row kernel (csrc/pool_rows.hip) at every encoder level of the
pose 512x512 B = 2 and street 1024x512 B = 1 generators, the four reference step fixtures and the inference fixture, eager against
graphed replay, and bit reproducibility in the fixed-order mode."""
import pytest
import torch

import adaptive_conv_checks as ac
import graph_step_checks as gc

# ngf 32, n_downsample_G 5: encoder level i holds CH[i] channels at 512 >> i (pose) / (512 >> i, 1024 >> i) (street)
CH = [32, 64, 128, 256, 512, 1024]
LEVELS = [(2, CH[i], 512 >> i, 512 >> i) for i in range(6)] + [(1, CH[i], 512 >> i, 1024 >> i) for i in range(6)]


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(64, 64), (32, 32), (16, 16), (2, 2), (7, 5), (40, 72), (33, 97)])
@pytest.mark.parametrize('c', [4, 8, 36])
def test_pool_rows_windows_against_torch(hip_lib, h, w, c):
    ac.check_pool_windows(torch.device('cuda:0'), 2, c, h, w)


@pytest.mark.gpu
@pytest.mark.parametrize('b,c,h,w', LEVELS)
def test_pool_rows_at_pose_and_street_levels(hip_lib, b, c, h, w):
    # float64 and torch's own fp32 result both on the device (the CPU would need minutes for the full-resolution levels)
    ac.check_pool_random(torch.device('cuda:0'), b, c, h, w, ref_device='cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('case', ac.STEP_CASES)
def test_step_reproduces_reference_iteration_on_gpu(hip_lib, case):
    ac.check_step(torch.device('cuda:0'), case)


@pytest.mark.gpu
def test_inference_reuses_cached_conv_weights_on_gpu(hip_lib):
    ac.check_inference(torch.device('cuda:0'))


KW = dict(warp_ref=True, spade_combine=True, remove_face_labels=True, fineSize=32, loadSize=32, n_downsample_G=3, n_adaptive_layers=2,
          use_label_ref='concat', adaptive_conv=True)


@pytest.mark.gpu
def test_graphed_replay_equals_eager_aconv(hip_lib, monkeypatch):
    """fixed-order mode: the captured iteration replays the eager loop bit for bit, learning rates of 1e-5 / 3e-5 included"""
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    dev = torch.device('cuda:0')
    ref, pG, pD, _ = gc._run(dev, False, 4, 500, KW)
    got, qG, qD, step = gc._run(dev, True, 4, 500, KW)
    assert any(e.graphs is not None for e in step.entries.values()), 'nothing was captured'
    for it, (a, b) in enumerate(zip(ref, got)):
        assert a['d'] == b['d'] and a['g'] == b['g'], (it, a['d'], b['d'], a['g'], b['g'])
        assert torch.equal(a['img'], b['img']), it
    assert torch.equal(pG, qG) and torch.equal(pD, qD)


@pytest.mark.gpu
def test_fixed_order_mode_is_bit_reproducible_aconv(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    dev = torch.device('cuda:0')
    a, pG, pD, _ = gc._run(dev, False, 2, 510, KW)
    b, qG, qD, _ = gc._run(dev, False, 2, 510, KW)
    for x, y in zip(a, b):
        assert x['d'] == y['d'] and x['g'] == y['g'] and torch.equal(x['img'], y['img'])
    assert torch.equal(pG, qG) and torch.equal(pD, qD)
