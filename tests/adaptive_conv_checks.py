"""Shared checks of --use_label_ref concat and --adaptive_conv: the pooled-row kernel (csrc/pool_rows.hip) against torch's
adaptive_avg_pool2d and a float64 evaluation, the step / inference against fixtures minted from the unmodified reference
(`python tests/test_adaptive_conv_emu.py`).  Used by tests/test_adaptive_conv_emu.py (emulator) and tests/test_adaptive_conv_gpu.py
(hardware)."""
import os

import torch
import torch.nn.functional as F

import model_checks as mc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STEP_CASES = ['face_concat', 'face_aconv_concat', 'face_aconv_only_concat', 'pose_combine_aconv_concat']
INFERENCE_CASE = 'pose_combine_aconv_concat'
POOL = 32            # generator.py:54 sh_fix = sw_fix


def opt_from_flags(flags):
    """test_golden._opt_from_flags plus the two options of this feature (it rejects flags it does not know)"""
    from test_golden import _opt_from_flags
    toks, extra = flags.split(), {}
    rest, i = [], 0
    while i < len(toks):
        if toks[i] == '--use_label_ref':
            extra['use_label_ref'] = toks[i + 1]; i += 2
        elif toks[i] == '--adaptive_conv':
            extra['adaptive_conv'] = True; i += 1
        else:
            rest.append(toks[i]); i += 1
    opt = _opt_from_flags(' '.join(rest))
    opt.adaptive_spade = '--adaptive_spade' in toks          # (a store_true flag of the reference; the product namespace defaults to on)
    for k, v in extra.items():
        setattr(opt, k, v)
    return opt


def load_step(case):
    return torch.load(os.path.join(GOLD, 'step_%s.pt' % case), weights_only=False)


def _ops():
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.ops')


# ------------------------------------------------------------------------------------------------ the pooled-row kernel
def pool_product(device, x, drows):
    """ops.pool_rows on `device`: rows [B * C, 1024] and the gradient of x under `drows`"""
    ops = _ops()
    xd = x.to(device).detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    rows = ops.pool_rows(xd, POOL, POOL)
    rows.backward(drows.to(device))
    return rows.detach(), xd.grad.detach()


def pool_torch(x, drows, dtype, device='cpu'):
    """F.adaptive_avg_pool2d + autograd in `dtype`, reshaped the way generator.py:169-174 reshapes it"""
    xr = x.to(device=device, dtype=dtype).detach().clone().requires_grad_(True)
    b, c = x.shape[:2]
    rows = F.adaptive_avg_pool2d(xr, (POOL, POOL)).reshape(b * c, POOL * POOL)
    rows.backward(drows.to(device=device, dtype=dtype))
    return rows.detach(), xr.grad.detach()


def ulps(a, b):
    """largest |a - b| in units of the spacing of b's fp32 values (a, b fp32)"""
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    sp = torch.from_numpy(__import__('numpy').spacing(b.abs().clamp_min(1e-30).numpy()))
    return float(((a - b).abs() / sp).max())


def check_pool_windows(device, b, c, h, w, seed=5):
    """(a) window indices: small integers, sums exact in fp32 - forward and backward within 1 ulp of torch's fp32 result"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (b, c, h, w), generator=g).float()
    drows = torch.randint(-8, 9, (b * c, POOL * POOL), generator=g).float()
    rows, dx = pool_product(device, x, drows)
    rows_t, dx_t = pool_torch(x, drows, torch.float32)
    assert rows.shape == rows_t.shape and dx.shape == dx_t.shape
    uf, ub = ulps(rows, rows_t), ulps(dx, dx_t)
    print('pool_rows windows', (b, c, h, w), 'forward ulps', uf, 'backward ulps', ub)
    assert uf <= 1.0, ('forward', uf)
    assert ub <= 1.0, ('backward', ub)


def check_pool_random(device, b, c, h, w, seed=6, ref_device='cpu'):
    """(b) / (c) random inputs against float64: at most 4 x the error of torch's own fp32 adaptive_avg_pool2d against the same
    float64 result on the same inputs (the summation order differs), with a floor of 1e-6 of the output's absmax.  Returns
    (error of the kernel, error of torch fp32) per direction, each relative to the float64 result's absmax."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, h, w, generator=g) + 0.25
    drows = torch.randn(b * c, POOL * POOL, generator=g)
    rows, dx = pool_product(device, x, drows)
    r64, d64 = pool_torch(x, drows, torch.float64, ref_device)
    r32, d32 = pool_torch(x, drows, torch.float32, ref_device)
    out = []
    for name, got, t32, t64 in (('forward', rows, r32, r64), ('backward', dx, d32, d64)):
        top = float(t64.abs().max())
        e_k = float((got.double().to(t64.device) - t64).abs().max()) / top
        e_t = float((t32.double() - t64).abs().max()) / top
        print('pool_rows random', (b, c, h, w), name, 'kernel %.3e' % e_k, 'torch fp32 %.3e' % e_t)
        assert e_k <= max(4.0 * e_t, 1e-6), (name, e_k, e_t)
        out.append((e_k, e_t))
    return out


# ------------------------------------------------------------------------------------------------ reference fixtures
def check_step(device, case, grad_tol=1e-2):
    """one D + G iteration of the product on the fixture's inputs and key-derived weights against the unmodified reference's: the
    bars of test_golden.test_product_reproduces_reference_iteration_on_gpu; every parameter of the fixture is seen"""
    from test_golden import _check_grad_norms, _check_grad_sketches, _inputs, _rel
    g = load_step(case)
    opt = opt_from_flags(g['flags'])
    M = mc._model()
    model = M.create_model(opt)
    mc.fill_state(model.netG); mc.fill_state(model.netD)
    model = model.to(device).train()
    opt_G, opt_D = model.build_optimizers()
    opt_G.set_lr(0.0); opt_D.set_lr(0.0)
    tl, ti, rl, ri = [t.to(device) for t in _inputs(g, opt)]
    data = [tl, ti, [None, None], [None, None], rl, ri, None, None, None]
    d = M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
    _check_grad_norms(model.netD, g['grad_norm_D'], 'netD', tol=grad_tol)
    _check_grad_sketches(model.netD, g['grad_sketch_D'], g['grad_norm_D'], 'netD')
    gl, generated, _ = model(data, save_images=True, mode='generator')
    gl = M.loss_backward(opt, gl, opt_G, 0)
    # every parameter of the fixture is seen; a parameter the reference left without a gradient (an encoder level whose feature
    # map no weight generator reads) has none here either - a zero slice of the optimiser's flat gradient buffer
    mine = {k: p for k, p in model.netG.named_parameters() if p.grad is not None}
    assert set(g['grad_norm_G']) <= set(mine), sorted(set(g['grad_norm_G']) - set(mine))[:10]
    for k in set(mine) - set(g['grad_norm_G']):
        assert float(mine[k].grad.abs().max()) == 0.0, k
    if getattr(opt, 'adaptive_conv', False):
        assert any(k.startswith('fc_conv_') and v > 0 for k, v in g['grad_norm_G'].items())
    _check_grad_norms(model.netG, g['grad_norm_G'], 'netG', tol=grad_tol)
    _check_grad_sketches(model.netG, g['grad_sketch_G'], g['grad_norm_G'], 'netG')
    for i in range(len(d)):
        assert abs(float(d[i]) - g['d_losses'][i]) <= 1e-3 * max(1.0, abs(g['d_losses'][i])), i
    for i, ref in enumerate(g['g_losses']):
        assert abs(float(gl[i]) - ref) <= 1e-3 * max(1.0, abs(ref)), (g['loss_names'][i], float(gl[i]), ref)
    assert _rel(generated[0].cpu(), g['fake']) <= 1e-3
    if g['flow'][0] is not None:
        assert _rel(generated[3][0].cpu(), g['flow'][0]) <= 1e-3
        assert _rel(generated[4][0].cpu(), g['mask'][0]) <= 1e-3
        assert _rel(generated[2][0].cpu(), g['warp'][0]) <= 1e-3


def check_inference(dev):
    """test.py path on the fixture (bars of test_golden._check_product_inference): frames after the first re-use the cached SPADE,
    embedding AND convolution weights - the weight generators and the pooled-row kernel do not run again"""
    from importlib import import_module
    from test_golden import _rel
    lib = import_module('few-shot-vid2vid_amd.lib')
    g = torch.load(os.path.join(GOLD, 'inference_%s.pt' % INFERENCE_CASE), weights_only=False)
    opt = opt_from_flags(g['flags'])
    M = mc._model()
    model = M.create_model(opt)
    model.netG.init_temporal_network()
    mc.fill_state(model.netG)
    sd = model.netG.state_dict()
    for k, v in g['buffers'].items():
        sd[k].copy_(v)
    frames = [mc.synth_pose_inputs(g['batch'], g['size'], g['size'], g['seed'] + t, 6) for t in range(3)]
    model = model.to(dev).eval()
    opt.isTrain = False
    ref_label, ref_image = frames[0][2].to(dev), frames[0][3].to(dev)
    real, pools = lib.call, []
    for t, (f, ref) in enumerate(zip(frames, g['fakes'])):
        seen = []
        lib.call = lambda name, *a: (seen.append(name), real(name, *a))[1]
        try:
            fake = model([f[0].to(dev), None, None, None, ref_label, ref_image, None, None, None])[0]
        finally:
            lib.call = real
        pools.append(seen.count('fsv_pool_rows_fwd'))
        if t == 0:
            cached = model.netG._cached_weights
            assert len(cached) == 3 and len(cached[2]) == model.netG.n_adaptive_layers
            ids = [id(w) for lvl in cached[2] for pair in lvl for w in pair]
        assert _rel(fake.cpu(), ref) <= 1e-3, t
    assert pools[0] > 0 and pools[1] == 0 and pools[2] == 0, pools
    assert [id(w) for lvl in model.netG._cached_weights[2] for pair in lvl for w in pair] == ids
    assert model.t == 2
