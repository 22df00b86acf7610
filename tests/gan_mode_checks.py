"""Shared checks of --gan_mode ls / original / w: the GANLoss reduction (csrc/losses.hip fsv_hinge_fwd / _bwd with a mode, through
ops.gan_loss) against a float64 evaluation with the bar taken from torch's own fp32 error on the same inputs, the hinge path left
bit-equal, bad arguments, and one D + G iteration / two temporal frames of the product against fixtures minted from the unmodified
reference (`python tests/test_gan_mode_emu.py`).  Used by tests/test_gan_mode_emu.py (emulator) and tests/test_gan_mode_gpu.py
(hardware)."""
import contextlib
import os
from importlib import import_module

import numpy as np
import torch
import torch.nn.functional as F

import adaptive_conv_checks as ac
import model_checks as mc

GOLD = ac.GOLD
MODES = ['ls', 'original', 'w']
SIZES = [1, 255, 256, 257, 4099, 512 * 256 + 3]        # the last: more than one pass of the 512-block grid
PLANTED = [0.0, 1.0, -1.0, 30.0, -30.0, 100.0, -100.0]
STEP_CASES = ['face_ls', 'face_original', 'face_w', 'face_numD2_ls', 'pose_combine_original']
# new fixture -> (oracle.make_golden.CONFIGS key, flags appended, committed hinge fixture of the same base configuration)
STEP_FLAGS = {'face_ls': ('face', ' --gan_mode ls', 'face'), 'face_original': ('face', ' --gan_mode original', 'face'),
              'face_w': ('face', ' --gan_mode w', 'face'), 'face_numD2_ls': ('face_numD2', ' --gan_mode ls', 'face_numD2'),
              'pose_combine_original': ('pose_combine', ' --gan_mode original', 'pose_combine')}
TEMPORAL_CASE = 'pose_combine_dt_ls'
KW = dict(gan_mode='original', fineSize=32, loadSize=32, n_downsample_G=3, n_adaptive_layers=2)


def _ops():
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.ops')


def _lib():
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.lib')


def opt_from_flags(flags):
    """adaptive_conv_checks.opt_from_flags plus --gan_mode (it rejects flags it does not know)"""
    toks = flags.split()
    mode = None
    if '--gan_mode' in toks:
        i = toks.index('--gan_mode')
        mode = toks[i + 1]
        del toks[i:i + 2]
    opt = _ac_opt_from_flags(' '.join(toks))
    if mode is not None:
        opt.gan_mode = mode
    return opt


_ac_opt_from_flags = ac.opt_from_flags


@contextlib.contextmanager
def _gan_mode_flags():
    """adaptive_conv_checks.check_step reads its fixture's flags with a parser that stops at --gan_mode: lend it the one above"""
    saved = ac.opt_from_flags
    ac.opt_from_flags = opt_from_flags
    try:
        yield
    finally:
        ac.opt_from_flags = saved


# ------------------------------------------------------------------------------------------------ the kernel against float64
def inputs(shape, seed, nhwc=False):
    """standard normal values x 3 with 0, +-1, +-30, +-100 planted (as many as fit)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 3.0
    flat = x.view(-1)
    k = min(flat.numel(), len(PLANTED))
    flat[:k] = torch.tensor(PLANTED[:k])
    if nhwc:
        x = x.contiguous(memory_format=torch.channels_last)
    return x


def formula(x, real, mode):
    """the table of the objectives (loss.py:50-53, 57-61, 85-90) spelled out; x in the dtype it is to be evaluated in"""
    t = 1.0 if real else 0.0
    if mode == 'ls':
        return ((x - t) ** 2).mean()
    if mode == 'original':
        return (x.clamp_min(0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean()
    if mode == 'w':
        return -x.mean() if real else x.mean()
    raise ValueError(mode)


def torch_fp32(x, real, mode):
    """what the reference computes: torch's own fp32 operators"""
    t = torch.full_like(x, 1.0 if real else 0.0)
    if mode == 'ls':
        return F.mse_loss(x, t)
    if mode == 'original':
        return F.binary_cross_entropy_with_logits(x, t)
    return -x.mean() if real else x.mean()


def _ulp32(v):
    """spacing of fp32 numbers at |v|"""
    return float(np.spacing(np.float32(abs(v)))) if v != 0.0 else float(np.spacing(np.float32(0)))


G_UP = 0.75          # the upstream scalar g of the backward pass (exact in fp32)


def check_kernel(device, x, real, mode, ref_device='cpu'):
    """ops.gan_loss on `device` against the float64 formula: error at most twice that of torch's fp32 operators on the same inputs,
    floor 4 fp32 ulps of the float64 value (value) / of the largest float64 gradient entry (dx, element-wise maximum); all finite"""
    ops = _ops()
    xd = x.to(device).detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    out = ops.gan_loss(xd, real, mode)
    assert out.shape == (1,) and out.dtype == torch.float32
    out.backward(torch.full((1,), G_UP, device=device))
    x64 = x.to(ref_device).double().detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    r64 = formula(x64, real, mode)
    r64.backward(torch.tensor(G_UP, dtype=torch.float64, device=ref_device))
    x32 = x.to(ref_device).detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    r32 = torch_fp32(x32, real, mode)
    r32.backward(torch.tensor(G_UP, device=ref_device))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(xd.grad).all())
    assert xd.grad.shape == x.shape
    v64 = float(r64)
    e_k, e_t = abs(float(out.double().cpu()) - v64), abs(float(r32.double()) - v64)
    bar = max(2.0 * e_t, 4.0 * _ulp32(v64))
    d64 = x64.grad
    g_k = float((xd.grad.double().to(ref_device) - d64).abs().max())
    g_t = float((x32.grad.double() - d64).abs().max())
    g_bar = max(2.0 * g_t, 4.0 * _ulp32(float(d64.abs().max())))
    print('gan_loss', mode, 'real' if real else 'fake', tuple(x.shape), 'value: kernel %.3e torch fp32 %.3e bar %.3e' % (e_k, e_t, bar),
          '| dx: kernel %.3e torch fp32 %.3e bar %.3e' % (g_k, g_t, g_bar))
    assert e_k <= bar, (mode, real, tuple(x.shape), e_k, e_t, bar)
    assert g_k <= g_bar, (mode, real, tuple(x.shape), g_k, g_t, g_bar)
    return (e_k, e_t), (g_k, g_t)


def check_hinge_untouched(device, n):
    """ops.gan_loss(.., 'hinge') IS ops.hinge_loss: value and gradient bit-equal for both targets"""
    ops = _ops()
    x = inputs((n,), 40 + n % 7)
    for real in (True, False):
        res = []
        for fn in (lambda t: ops.gan_loss(t, real, 'hinge'), lambda t: ops.hinge_loss(t, real)):
            xd = x.to(device).detach().clone().requires_grad_(True)
            out = fn(xd)
            out.backward(torch.full((1,), G_UP, device=device))
            res.append((out.detach().cpu(), xd.grad.detach().cpu()))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (n, real)
        want = -torch.minimum((1.0 if real else -1.0) * x.double() - 1.0, torch.zeros((), dtype=torch.float64)).mean()
        assert abs(float(res[0][0]) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))


def check_bad_arguments(device, count_launches=None):
    """an unknown mode string raises like GANLoss.__init__; an unknown mode code is FSV_ERR_BAD_ARG with nothing launched"""
    import pytest
    ops, lib = _ops(), _lib()
    x = torch.randn(2, 1, 3, 5).to(device)
    for bad in ('lsgan', 'Hinge', '', None):
        with pytest.raises(ValueError, match='Unexpected gan_mode'):
            ops.gan_loss(x, True, bad)
    part = torch.zeros(512, dtype=torch.float64, device=device)
    loss = torch.full((1,), -7.0, device=device)
    dx = torch.full_like(x, -7.0)
    g = torch.ones(1, device=device)
    c0 = count_launches() if count_launches else 0
    for mode in (7, -1, 4):
        assert lib.call_status('fsv_hinge_fwd', lib.ptr(x), x.numel(), 1.0, mode, lib.ptr(part), lib.ptr(loss),
                               lib.stream_ptr()) == lib.ENUMS['FSV_ERR_BAD_ARG']
        assert lib.call_status('fsv_hinge_bwd', lib.ptr(x), x.numel(), 1.0, mode, lib.ptr(g), lib.ptr(dx),
                               lib.stream_ptr()) == lib.ENUMS['FSV_ERR_BAD_ARG']
    if count_launches:
        assert count_launches() == c0
    assert float(loss) == -7.0 and bool((dx == -7.0).all()) and float(part.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ reference fixtures
def check_step(device, case):
    """adaptive_conv_checks.check_step (losses 1e-3, gradient norms and sketches as there) on a --gan_mode fixture"""
    with _gan_mode_flags():
        ac.check_step(device, case)


def product_two_frames(device, opt):
    """two consecutive frames of the product with the previous-frame branch and the temporal discriminator, learning rate 0, in the
    shape tests/model_checks._oracle_two_frames returns: (d_losses, gD, g_losses by name, gG, generated, gDT) of the second frame"""
    M = mc._model()
    model = M.create_model(opt)
    mc.fill_state(model.netD)
    model = model.to(device).train()
    model.build_optimizers()
    model.init_temporal_model()
    mc.fill_state(model.netG)
    if opt.lambda_temp > 0:
        mc.fill_state(model.netDT)
    opt_G, opt_D = model.optimizer_G, model.optimizer_D
    opt_G.set_lr(0.0); opt_D.set_lr(0.0)
    frames = [mc.synth_pose_inputs(1, 64, 64, 777 + t, 6) for t in range(2)]
    frames[1] = (frames[1][0], frames[1][1], frames[0][2], frames[0][3])
    prevs = [None, None, None]
    for data in frames:
        tl, ti, rl, ri = [x.to(device) for x in data]
        data_list = [tl, ti, [None, None], [None, None], rl, ri] + prevs
        d_losses = M.loss_backward(opt, model(data_list, mode='discriminator'), opt_D, 1)
        gD = {k: p.grad.detach().clone().cpu() for k, p in model.netD.named_parameters() if p.grad is not None}
        gDT = {k: p.grad.detach().clone().cpu() for k, p in model.netDT.named_parameters() if p.grad is not None} \
            if opt.lambda_temp > 0 else {}
        g_losses, generated, prevs = model(data_list, save_images=True, mode='generator')
        g_losses = M.loss_backward(opt, g_losses, opt_G, 0)
    gG = {}
    for k, p in model.netG.named_parameters():
        if p.grad is None:
            continue
        gG[k] = p.grad.detach().clone().cpu()
        for a, b in (('flow_network_temp.', 'flow_network_ref.'), ('flow_network_ref.', 'flow_network_temp.')):
            if k.startswith(a):                   # one shared module, two names
                gG.setdefault(b + k[len(a):], gG[k])
    gen = dict(fake=generated[0].detach().cpu(), warp=[None if t is None else t.detach().cpu() for t in generated[2]],
               flow=[None if t is None else t.detach().cpu() for t in generated[3]],
               mask=[None if t is None else t.detach().cpu() for t in generated[4]])
    return ([x.detach().cpu() for x in d_losses], gD, {k: g_losses[i].detach().cpu() for i, k in enumerate(M.LOSS_NAMES_G)},
            gG, gen, gDT)


def temporal_figures(device, case=TEMPORAL_CASE):
    """the product's second temporal frame next to the fixture: the quantities test_golden.test_oracle_reproduces_reference_second_frame
    compares, each relative to the denominator that function uses"""
    from test_golden import _rel
    g = torch.load(os.path.join(GOLD, 'temporal_%s.pt' % case), weights_only=False)
    opt = opt_from_flags(g['flags'])
    d, _, gl, gG, gen, gDT = product_two_frames(device, opt)
    names = g['loss_names']
    assert opt.lambda_temp > 0 and len(d) == 6 and g['g_losses'][names.index('GT_GAN_Feat')] > 0 and g['grad_norm_DT']
    fig = dict(d=max(abs(float(d[i]) - r) / max(1.0, abs(r)) for i, r in enumerate(g['d_losses'])),
               g=max(abs(float(v) - g['g_losses'][names.index(k)]) / max(1.0, abs(g['g_losses'][names.index(k)])) for k, v in gl.items()),
               fake=_rel(gen['fake'], g['fake']), warp1=_rel(gen['warp'][1], g['warp'][1]), flow1=_rel(gen['flow'][1], g['flow'][1]),
               gDT=max(abs(float(gDT[k].norm()) - r) / max(r, 1e-6) for k, r in g['grad_norm_DT'].items()))
    med = sorted(g['grad_norm_G'].values())[len(g['grad_norm_G']) // 2]
    fig['gG'] = max(abs(float(gG[k].norm()) - r) / max(r, 5e-2 * med) for k, r in g['grad_norm_G'].items())
    return fig


def check_temporal(device, case=TEMPORAL_CASE):
    """Two frames of the PRODUCT, the second with the previous-frame branch and the temporal discriminator, against the reference
    fixture.  tests/test_golden.py compares temporal_pose_combine_dt.pt in test_oracle_reproduces_reference_second_frame only - a
    check of oracle/fsv_oracle.py, which restates the reference operator by operator in torch, knows the hinge objective alone and
    is not edited: neither that function nor its bars (1e-5 on losses and images, 1e-4 / 1e-3 on gradient norms: two torch programs
    that differ in nothing but structure) apply to the HIP kernels.  What is kept from it: the quantities (all six D losses, every
    G loss, image, previous-frame warp and flow, the gradient norm of every netDT and netG parameter) and its denominators.  The
    bars are the ones this suite holds the product to against a reference fixture in check_step / test_golden: 1e-3 on losses and
    outputs, 1e-2 on gradient norms (test_golden._check_grad_norms).  Emulator figures when written: losses 5.2e-6 / 4.4e-6, image
    2.0e-4, warp 5.7e-5, flow 9.0e-6, netDT norms 7.4e-6, netG norms 3.5e-3."""
    fig = temporal_figures(device, case)
    print('temporal', case, {k: '%.2e' % v for k, v in fig.items()})
    for k in ('d', 'g', 'fake', 'warp1', 'flow1'):
        assert fig[k] <= 1e-3, (k, fig)
    for k in ('gDT', 'gG'):
        assert fig[k] <= 1e-2, (k, fig)
