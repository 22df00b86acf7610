"""Shared checks of the 3x3 SPADE (--spade_ks 3, csrc/spade_k3.hip) and the 3x3 embedding (--embed_ks 3): the op against a float64
restatement written here (F.batch_norm statistics, per-sample F.conv2d with padding 1, the modulation, LeakyReLU), the step against
fixtures minted from the unmodified reference (`python tests/test_spade_k3_emu.py`).  Used by tests/test_spade_k3_emu.py (emulator)
and tests/test_spade_k3_gpu.py (hardware)."""
import os

import torch
import torch.nn.functional as F

import model_checks as mc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STEP_CASES = ['pose_combine_ks3', 'face_sks3', 'face_eks3']


def opt_from_flags(flags):
    """test_golden._opt_from_flags plus the two kernel-size options (it rejects flags it does not know)"""
    from test_golden import _opt_from_flags
    toks, ks = flags.split(), {}
    rest, i = [], 0
    while i < len(toks):
        if toks[i] in ('--spade_ks', '--embed_ks'):
            ks[toks[i][2:]] = int(toks[i + 1]); i += 2
        else:
            rest.append(toks[i]); i += 1
    opt = _opt_from_flags(' '.join(rest))
    for k, v in ks.items():
        setattr(opt, k, v)
    return opt


def load_step(case):
    return torch.load(os.path.join(GOLD, 'step_%s.pt' % case), weights_only=False)


def spade_ref(x, maps, weights, act, up):
    """normalization.py:37-52 with ks = 3 (+ leaky_relu) as a float64 autograd restatement.  weights[k] = (wg, wb, bg, bb), wg / wb
    [C, Ch, 3, 3] (shared) or [B, C, Ch, 3, 3] (per sample)"""
    if up:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    out = F.batch_norm(x, None, None, training=True, eps=1e-5)
    for m, (wg, wb, bg, bb) in zip(maps, weights):
        if wg.dim() == 5:
            g = torch.cat([F.conv2d(m[i:i + 1], wg[i], bg[i], padding=1) for i in range(m.shape[0])])
            b = torch.cat([F.conv2d(m[i:i + 1], wb[i], bb[i], padding=1) for i in range(m.shape[0])])
        else:
            g, b = F.conv2d(m, wg, bg, padding=1), F.conv2d(m, wb, bb, padding=1)
        out = out * (1 + g) + b
    return F.leaky_relu(out, 0.2) if act else out


def make_case(n, c, chs, h, w, per_sample0, up, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, c, h // 2 if up else h, w // 2 if up else w, generator=g) + 0.3
    maps = [torch.randn(n, ch, h, w, generator=g) for ch in chs]
    ws = []
    for k, ch in enumerate(chs):
        s = 0.6 / (9 * ch) ** 0.5
        lead = (n,) if (k == 0 and per_sample0) else ()
        ws.append((torch.randn(*lead, c, ch, 3, 3, generator=g) * s, torch.randn(*lead, c, ch, 3, 3, generator=g) * s,
                   torch.randn(*lead, c, generator=g) * 0.3, torch.randn(*lead, c, generator=g) * 0.3))
    dy = torch.randn(n, c, h, w, generator=g)
    return x, maps, ws, dy


def run_product(device, x, maps, ws, dy, act, up):
    """ops.spade_mod on `device`: (h, [dx, d(map_k)..., d(wg, wb, bg, bb)_k...], running mean, running var)"""
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    ops = import_module('few-shot-vid2vid_amd.ops')
    conv = import_module('few-shot-vid2vid_amd.conv')
    cl = lambda t: t.to(device).detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    xd = cl(x)
    md = [cl(m) for m in maps]
    wd = [tuple(t.to(device).detach().clone().requires_grad_(True) for t in wt) for wt in ws]
    c = x.shape[1]
    rm, rv = torch.zeros(c, device=device), torch.ones(c, device=device)
    y = ops.spade_mod(xd, md, wd, rm, rv, act=conv.ACT_LRELU if act else conv.ACT_NONE, up=up)
    y.backward(dy.to(device))
    grads = [xd.grad] + [m.grad for m in md] + [t.grad for wt in wd for t in wt]
    return y.detach(), grads, rm, rv


def reference(x, maps, ws, dy, act, up, device='cpu'):
    """float64 reference of run_product's outputs, computed on `device`"""
    leaf = lambda t: t.to(device=device, dtype=torch.float64).detach().clone().requires_grad_(True)
    xr = leaf(x)
    mr = [leaf(m) for m in maps]
    wr = [tuple(leaf(t) for t in wt) for wt in ws]
    y = spade_ref(xr, mr, wr, act, up)
    y.backward(dy.to(device=device, dtype=torch.float64))
    xin = F.interpolate(x.double(), scale_factor=2, mode='nearest') if up else x.double()
    rm, rv = torch.zeros(x.shape[1], dtype=torch.float64), torch.ones(x.shape[1], dtype=torch.float64)
    F.batch_norm(xin, rm, rv, training=True, momentum=0.1, eps=1e-5)
    grads = [xr.grad] + [m.grad for m in mr] + [t.grad for wt in wr for t in wt]
    return y.detach(), grads, rm, rv


def band_rows(h):
    """rows the CPU comparison of a large case covers: both borders and one interior pair"""
    return sorted(set([0, 1, h // 2, h // 2 + 1, h - 2, h - 1]))


def spade_band_ref(x, maps, ws, act, up, rows):
    """h of spade_ref on the given rows only, in float64 on the CPU: BatchNorm statistics over the whole tensor, the 3x3 convolutions
    of each row from its three source rows (zero rows beyond the image)"""
    x = x.double()
    if up:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    mean = x.mean((0, 2, 3), keepdim=True)
    var = x.var((0, 2, 3), unbiased=False, keepdim=True)
    out = ((x[:, :, rows] - mean) / torch.sqrt(var + 1e-5))
    for m, (wg, wb, bg, bb) in zip(maps, ws):
        mp = F.pad(m.double(), (1, 1, 1, 1))
        strip = torch.stack([mp[:, :, r:r + 3] for r in rows], 2)            # [N, Ch, R, 3, W + 2]
        n, ch, nr, _, wp = strip.shape
        s2 = strip.permute(0, 2, 1, 3, 4).reshape(n * nr, ch, 3, wp)
        outs = []
        for wt, bt in ((wg, bg), (wb, bb)):
            wt, bt = wt.double(), bt.double()
            if wt.dim() == 5:
                r = torch.stack([F.conv2d(s2[i * nr:(i + 1) * nr], wt[i], bt[i]) for i in range(n)])
            else:
                r = F.conv2d(s2, wt, bt).view(n, nr, -1, 1, wp - 2)
            outs.append(r.view(n, nr, -1, wp - 2).permute(0, 2, 1, 3))
        out = out * (1 + outs[0]) + outs[1]
    return F.leaky_relu(out, 0.2) if act else out


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


GRAD_NAMES = ('dwg', 'dwb', 'dbg', 'dbb')


def check_op(device, n, c, chs, h, w, per_sample0=True, up=False, act=True, seed=3, h_tol=1e-4, g_tol=1e-3, ref_device='cpu',
             band=False):
    """h within h_tol of the reference's absmax, every gradient within g_tol relative L2, the running statistics.  band: the
    float64 reference of h on the CPU over band_rows only (large cases); the gradients against the float64 reference on
    ref_device"""
    x, maps, ws, dy = make_case(n, c, chs, h, w, per_sample0, up, seed)
    y, grads, rm, rv = run_product(device, x, maps, ws, dy, act, up)
    if band:
        rows = band_rows(h)
        yb = spade_band_ref(x, maps, ws, act, up, rows)
        err = float((y[:, :, rows].double().cpu() - yb).abs().max()) / max(float(yb.abs().max()), 1e-30)
        assert err <= h_tol, ('h band', err)
    yr, gr, rmr, rvr = reference(x, maps, ws, dy, act, up, ref_device)
    err_all = float((y.double().cpu() - yr.cpu()).abs().max()) / max(float(yr.abs().max()), 1e-30)
    assert err_all <= h_tol, ('h', err_all)
    names = ['dx'] + ['dmap%d' % k for k in range(len(chs))] + ['%s%d' % (p, k) for k in range(len(chs)) for p in GRAD_NAMES]
    worst = 0.0
    for name, a, b in zip(names, grads, gr):
        assert a is not None, name
        e = rel_l2(a, b)
        worst = max(worst, e)
        assert e <= g_tol, (name, e)
    assert rel_l2(rm, rmr) <= 1e-5 and rel_l2(rv, rvr) <= 1e-5
    return err_all, worst


def check_step(device, case, grad_tol=1e-2):
    """one D + G iteration of the product on the fixture's inputs and key-derived weights against the unmodified reference's: the
    bars of test_golden.test_product_reproduces_reference_iteration_on_gpu"""
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
