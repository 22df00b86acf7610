"""--spade_ks 3 / --embed_ks 3 on the emulator: the 3x3 SPADE operator (csrc/spade_k3.hip through ops._SpadeFn) against a float64
restatement, one D + G iteration of the product against fixtures minted from the unmodified reference, the checkpoint layout, the
1x1-only fusions declining a 3x3 SPADE, and the option values that keep raising.

Mint the fixtures (needs the reference tree):   python tests/test_spade_k3_emu.py
"""
import contextlib
import copy
import json
import os
import sys

import pytest
import torch

import model_checks as mc
import spade_k3_checks as sk

DEV = torch.device('cpu')
LAYOUT = os.path.join(sk.GOLD, 'ref_state_layout_ks3.json')


@pytest.mark.parametrize('n,c,chs,h,w,per_sample0,up', [
    (2, 8, [8], 7, 5, False, False),            # one map, shared weights; odd H x W: every border tap
    (2, 8, [8, 4, 4], 7, 5, True, False),       # three maps, map 0 per sample (C = 8: the general width of the tiny fixtures)
    (2, 32, [8, 8, 8], 6, 4, True, True),       # x through the nearest x2 index; C = 32 (128 x 32 tile)
    (1, 32, [12], 9, 7, False, False),
    (2, 40, [8], 4, 6, True, True),             # 64 x 64 tile with a channel tail
])
def test_spade_k3_op_against_float64(emu_lib, n, c, chs, h, w, per_sample0, up):
    sk.check_op(DEV, n, c, chs, h, w, per_sample0=per_sample0, up=up)


def test_spade_k3_op_without_activation_and_a_band_of_rows(emu_lib):
    sk.check_op(DEV, 2, 8, [8, 4, 4], 14, 10, per_sample0=True, up=True, act=False, band=True)


@pytest.mark.parametrize('case', sk.STEP_CASES)
def test_step_reproduces_reference_iteration_emu(emu_lib, case):
    sk.check_step(DEV, case)


def test_state_dict_layout_equals_reference():
    ref = json.load(open(LAYOUT))
    for cfg, layout in ref.items():
        opt = sk.opt_from_flags(layout['flags'])
        M = mc._model()
        with torch.device('meta'):
            model = M.create_model(opt)
        for net, want in ((model.netG, layout['netG']), (model.netD, layout['netD'])):
            mine = {k: list(v.shape) for k, v in net.state_dict().items()}
            assert set(mine) == set(want), (cfg, sorted(set(mine) ^ set(want))[:10])
            bad = [k for k in want if mine[k] != want[k]]
            assert not bad, (cfg, bad[:10])
    assert any(k.endswith('mlp_gamma2.weight') and v[-1] == 3 for k, v in ref['C3_pose_512_ks3']['netG'].items())


@pytest.mark.parametrize('kw,word', [(dict(spade_ks=3, amp='O1'), 'amp'), (dict(spade_ks=5), 'spade_ks'),
                                     (dict(conv_ks=5), 'conv_ks'), (dict(embed_ks=5), 'embed_ks')])
def test_options_that_still_raise(kw, word):
    net = mc._net()
    with torch.device('meta'):
        with pytest.raises(NotImplementedError, match=word):
            net.define_G(mc.tiny_opt(**kw))


def test_fused_spade_launches_decline_a_3x3_spade(emu_lib, monkeypatch):
    """bn_s -> conv_s (on by default) and FSV_SPADE_CONV3 are 1x1-only: with every switch on, a 3x3 SPADE block runs
    the 3x3 modulation kernel and plain convolutions, and gives the same output as with the switches off"""
    from importlib import import_module
    net, lib = mc._net(), import_module('few-shot-vid2vid_amd.lib')
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 64, 4, 4, generator=g)
    label = torch.randn(2, 8, 8, 8, generator=g)
    torch.manual_seed(0)
    blk0 = net.SPADEResnetBlock(64, 32, hidden_nc=8, spade=True, spade_ks=3)
    outs = []
    for on in ('0', '1'):
        for k in ('FSV_SPADE_CONV_S', 'FSV_SPADE_CONV3'):
            monkeypatch.setenv(k, on)
        seen, real = [], lib.call
        monkeypatch.setattr(lib, 'call', lambda name, *a: (seen.append(name), real(name, *a))[1])
        blk = copy.deepcopy(blk0)          # (a forward advances the spectral-norm vectors and the running statistics)
        outs.append(blk(x.contiguous(memory_format=torch.channels_last), label, up=True).detach().clone())
        monkeypatch.setattr(lib, 'call', real)
        assert seen.count('fsv_spade_k3_fwd') == 3, seen
        assert not [s for s in seen if s.startswith(('fsv_spade_conv', 'fsv_spade_mod'))], seen
    assert torch.equal(outs[0], outs[1])


def mint():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import make_golden as mg, ref_import
    flags = {'pose_combine_ks3': mg.CONFIGS['pose_combine'] + ' --spade_ks 3 --embed_ks 3',
             'face_sks3': mg.CONFIGS['face'] + ' --spade_ks 3',
             'face_eks3': mg.CONFIGS['face'] + ' --embed_ks 3'}
    for name, f in flags.items():
        mg.step(name, f)
    lay = mg.LAYOUT_CONFIGS['C3_pose_512'] + ' --spade_ks 3 --embed_ks 3'
    opt, model = ref_import.build_model(lay.split())
    res = {'C3_pose_512_ks3': dict(flags=lay, netG={k: list(v.shape) for k, v in model.netG.state_dict().items()},
                                   netD={k: list(v.shape) for k, v in model.netD.state_dict().items()})}
    with open(LAYOUT, 'w') as fh:
        json.dump(res, fh)
    for p in [os.path.join(sk.GOLD, 'step_%s.pt' % n) for n in flags] + [LAYOUT]:
        print(p, os.path.getsize(p), 'bytes')


if __name__ == '__main__':
    with contextlib.suppress(KeyboardInterrupt):
        mint()
