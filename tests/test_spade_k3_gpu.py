"""--spade_ks 3 / --embed_ks 3 on the MI355X: the 3x3 SPADE operator (csrc/spade_k3.hip) at every SPADE shape of the pose 512x512 B = 2
generator, the three reference step fixtures, eager against graphed replay, and bit reproducibility in the fixed-order mode."""
import os

import pytest
import torch

import graph_step_checks as gc
import spade_k3_checks as sk

# pose 512 x 512, ngf 32, n_downsample_G 5: level i runs at 512 >> i with maps of ch[i] channels (three maps at levels 0 - 1, with
# spade_combine); its block normalises ch[i + 1] channels of the up-sampled input (bn_0 / bn_s, x read through the x2 index) and
# ch[i] channels (bn_1)
CH = [32, 64, 128, 256, 512, 1024, 1024]
SHAPES = [(2, c, [CH[i]] * (3 if i < 2 else 1), 512 >> i, 512 >> i, up)
          for i in range(6) for (c, up) in ((CH[i + 1], True), (CH[i], False))]


@pytest.mark.gpu
@pytest.mark.parametrize('n,c,chs,h,w,up', SHAPES)
def test_spade_k3_op_at_pose_512_shapes(hip_lib, n, c, chs, h, w, up):
    # h: against float64 on the CPU over rows at both borders (statistics of the whole tensor); everything: against float64 on the
    # device (the CPU would need minutes for the full-resolution levels)
    sk.check_op(torch.device('cuda:0'), n, c, chs, h, w, per_sample0=True, up=up, band=True, ref_device='cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('case', sk.STEP_CASES)
def test_step_reproduces_reference_iteration_on_gpu(hip_lib, case):
    sk.check_step(torch.device('cuda:0'), case)


KW = dict(warp_ref=True, spade_combine=True, remove_face_labels=True, fineSize=32, loadSize=32, n_downsample_G=3, n_adaptive_layers=2,
          spade_ks=3, embed_ks=3)


@pytest.mark.gpu
def test_graphed_replay_equals_eager_ks3(hip_lib, monkeypatch):
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
def test_fixed_order_mode_is_bit_reproducible_ks3(hip_lib, monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    dev = torch.device('cuda:0')
    a, pG, pD, _ = gc._run(dev, False, 2, 510, KW)
    b, qG, qD, _ = gc._run(dev, False, 2, 510, KW)
    for x, y in zip(a, b):
        assert x['d'] == y['d'] and x['g'] == y['g'] and torch.equal(x['img'], y['img'])
    assert torch.equal(pG, qG) and torch.equal(pD, qD)
