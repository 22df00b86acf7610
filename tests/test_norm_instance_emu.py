"""--norm_G spectralspadeinstance / --norm_F spectralinstance / spectralnone on the emulator: the SPADE kernels with per-sample
statistics against float64, the grouped statistics epilogue of csrc/spade_conv3.hip, one D + G iteration and three inference frames of
the product against fixtures minted from the unmodified reference, the state_dict layout, the options, eval() against train(), the
torch operators of an instance-normalised iteration against the default one, and the graphed iteration.

Mint the fixtures (needs the reference tree):   python tests/test_norm_instance_emu.py
"""
import contextlib
import json
import os
import sys

import pytest
import torch

import model_checks as mc
import norm_instance_checks as ni

DEV = torch.device('cpu')


# ---- 1: kernels with per-sample statistics against float64 (normalization.py:37-52)
# c 16: the prepared fast path, c 20: the general path; one and three maps of widths 4 and 12; generated and shared weights
@pytest.mark.parametrize('act', [True, False])
@pytest.mark.parametrize('up', [False, True])
@pytest.mark.parametrize('chs,per_sample', [((4,), True), ((12,), False), ((4, 12, 4), True), ((12, 4, 12), False)])
@pytest.mark.parametrize('c', [16, 20])
def test_spade_instance_ragged_tile(emu_lib, c, chs, per_sample, up, act):
    """9 x 7 (up: 10 x 6 from 5 x 3): ragged and smaller than one tile"""
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_instance(DEV, c=c, chs=chs, per_sample=per_sample, h=h, w=w, up=up, act=act, bwd='twin')


@pytest.mark.parametrize('up', [False, True])
@pytest.mark.parametrize('c', [16, 20])
def test_spade_instance_tile_walk(emu_lib, c, up):
    """24 x 20 with one workgroup per channel tile and sample: the pixel-tile walk"""
    ni.check_spade_instance(DEV, c=c, chs=(4, 12), per_sample=True, h=24, w=20, up=up, act=True, bwd='twin', max_gx=1)


@pytest.mark.parametrize('up', [False, True])
@pytest.mark.parametrize('chs,per_sample', [((4,), True), ((12, 4, 12), False)])
def test_spade_instance_elementwise_backward(emu_lib, chs, per_sample, up):
    """the other backward design on the fast path: gamma | beta materialised, fsv_spade_bwd_elem"""
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_instance(DEV, c=16, chs=chs, per_sample=per_sample, h=h, w=w, up=up, act=True, bwd='elem')


@pytest.mark.parametrize('up', [False, True])
def test_spade_instance_k3(emu_lib, up):
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_instance(DEV, c=16, chs=(4, 12), per_sample=True, h=h, w=w, up=up, act=True, k=3)


def test_spade_instance_ignores_mode_and_buffers(emu_lib):
    ni.check_spade_instance_eval_and_buffers(DEV)


@pytest.mark.parametrize('up', [False, True])
def test_spade_conv_s_instance(emu_lib, up):
    h, w = (10, 6) if up else (9, 7)
    ni.check_spade_conv_s_instance(DEV, h=h, w=w, up=up)


@pytest.mark.parametrize('up', [False, True])
def test_spade_conv3_instance_and_grouped_statistics(emu_lib, up):
    ni.check_spade_conv3_instance(DEV, up=up)


# ---- 2: the reference fixtures.  On a tree that ignores --norm_G / --norm_F these fail: it normalises over the batch
@pytest.mark.parametrize('case', ni.STEP_CASES)
def test_step_reproduces_reference_iteration_emu(emu_lib, case):
    ni.check_step(DEV, case)


def test_inference_reproduces_reference_emu(emu_lib):
    ni.check_inference(DEV)


def test_state_dict_layout_equals_the_reference():
    ni.check_layout()


# ---- 3: options
def test_unknown_norms_raise():
    ni.check_unknown_norms()


def test_non_default_norms_under_amp_raise():
    ni.check_amp_raises()


def test_eval_equals_train_bit_for_bit(emu_lib):
    ni.check_eval_equals_train(DEV)


def test_instance_iteration_issues_no_new_torch_operator(emu_lib):
    ni.check_no_new_torch_operator(DEV)


def test_graphed_iteration_equals_plain_loop(emu_lib):
    """three iterations of the instance-normalised pose_combine configuration: bit-equal weights between the plain loop and
    GraphedIteration, and not the batch-normalised network's"""
    import graph_step_checks as gc
    kw = dict(ni.KW, warp_ref=True, spade_combine=True)
    ref, pG, pD, _ = gc._run(DEV, False, 3, 520, kw)
    got, qG, qD, step = gc._run(DEV, True, 3, 520, kw)
    assert len(step.entries) == 1
    assert float((pG - qG).abs().max()) == 0.0 and float((pD - qD).abs().max()) == 0.0
    for a, b in zip(ref, got):
        assert a['d'] == b['d'] and a['g'] == b['g']


# ---- 4: minting
def _resave(path):
    """written through a file object the archive members carry a fixed short prefix (tests/test_gan_mode_emu.py)"""
    obj = torch.load(path, weights_only=False)
    with open(path, 'wb') as fh:
        torch.save(obj, fh)


def mint(only=None):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import make_golden as mg
    from oracle import ref_import
    layout = {}
    for name, (base, extra) in ni.LAYOUT_FLAGS.items():
        flags = mg.CONFIGS[base] + extra
        opt, model = ref_import.build_model(flags.split())
        layout[name] = dict(flags=flags, netG={k: list(v.shape) for k, v in model.netG.state_dict().items()})
        del model
    with open(ni.LAYOUT_FILE, 'w') as f:
        json.dump(layout, f)
    for name, (base, extra) in ni.STEP_FLAGS.items():
        if only and name not in only:
            continue
        mg.step(name, mg.CONFIGS[base] + extra)
        path = os.path.join(ni.GOLD, 'step_%s.pt' % name)
        _resave(path)
        print(name, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < 2 ** 20
    if not only or 'inference' in only:
        mg.inference(ni.INFERENCE_CASE, mg.CONFIGS['pose_combine'] + ni.STEP_FLAGS['pose_combine_inorm'][1])
        path = os.path.join(ni.GOLD, 'inference_%s.pt' % ni.INFERENCE_CASE)
        _resave(path)
        print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    with contextlib.suppress(KeyboardInterrupt):
        mint(sys.argv[1:])
