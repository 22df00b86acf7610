"""Checks of the y-free normalisation backward (fsv_norm_bwd_fused with y = NULL and the forward's bias) and of the Adam kernel's
beta1 == 0 / 16-byte form, shared by the emulated (`not gpu`) and the real-hardware (`gpu`) test modules.

The y-free mode recomputes the pre-activation v = ((x - mean) * rstd) * w + b by the expression the forward evaluates and takes the
slope of LeakyReLU(0.2) / LeakyReLU(0.1) / ReLU from v > 0 where the y mode takes it from y > 0.  y > 0 exactly when v > 0, so the
two modes must agree in every BIT of s1, s2, dw, db and dx - also on inputs built to sit on the kink, where a forward and a backward
that contract a * b + c differently would pick different slopes.  Values against fp64 PyTorch use the helpers and the `bounded` rule
of small_op_checks.check_sync_bn.
"""
import ctypes

import torch

import small_op_checks as sc
from op_checks import _dev, pkg
from small_op_checks import bits, bounded, f32, lib, same_bits

ACTS = {'lrelu': 1, 'relu': 4, 'lrelu01': 5}
NOY_SHAPES = ((1, 37, 6),        # scalar kernels (C % 4 != 0), ragged rows
              (2, 100, 32),      # InstanceNorm groups
              (1, 1000, 40),     # float4, two channel slabs
              (1, 4100, 64))     # 1.05 MB: the two-launch sums above the ticket threshold
NOY_EPS = 1e-5


def _backward_both(device, x, mean, rstd, w, b, dy, G, P, C, act, fixed_stats):
    """forward by fsv_norm_apply, then fsv_norm_bwd_fused with y and with (y = NULL, b): {name: (with y, without y)} and y"""
    ops, _ = pkg()
    L = lib()
    st = L.stream_ptr()
    xd, dyd, md, rd = (_dev(t.contiguous(), device) for t in (x, dy, mean, rstd))
    wd = _dev(w, device) if w is not None else None
    bd = _dev(b, device) if b is not None else None
    y = torch.empty_like(xd)
    L.call('fsv_norm_apply', L.ptr(xd), L.ptr(md), L.ptr(rd), L.ptr(wd), L.ptr(bd), L.ptr(y), G, P, C, act, None, st)
    ws = ops._ws(G, P, C, xd)
    ticket = ops._ticket(xd)
    res = []
    for yy, bb in ((y, None), (None, bd)):
        s1 = torch.full((G * C,), float('nan'), device=device)
        s2, dx = torch.full_like(s1, float('nan')), torch.full_like(xd, float('nan'))
        dw = torch.full((C,), float('nan'), device=device) if w is not None else None
        db = torch.full_like(dw, float('nan')) if w is not None else None
        L.call('fsv_norm_bwd_fused', L.ptr(dyd), L.ptr(yy), L.ptr(xd), L.ptr(md), L.ptr(rd), L.ptr(wd), L.ptr(bb), L.ptr(ws),
               L.ptr(s1), L.ptr(s2), L.ptr(dx), L.ptr(dw), L.ptr(db), G, P, C, act, fixed_stats, ticket, None, st)
        res.append(dict(s1=s1, s2=s2, dx=dx, dw=dw, db=db))
    return {k: (res[0][k], res[1][k]) for k in res[0]}, y


def _assert_modes_equal(tag, pair):
    for name, (a, b) in pair.items():
        if a is None:
            assert b is None
            continue
        assert bool(torch.isfinite(a).all()), '%s %s: not finite' % (tag, name)
        assert torch.equal(a, b), '%s %s: the two modes differ' % (tag, name)
        same_bits('%s %s' % (tag, name), b, a)


def _stats(device, x, G, P, C):
    ops, _ = pkg()
    mean, rstd = ops.norm_stats(_dev(x.contiguous(), device), G, P, C, NOY_EPS)
    return mean.cpu(), rstd.cpu()


def check_modes_bit_equal(device, shape, act, affine, fixed_stats, seed=201):
    """1. s1, s2, dw, db, dx of the y mode and of the y-free mode, bit for bit"""
    G, P, C = shape
    g = torch.Generator().manual_seed(seed + 13 * P + C + 7 * ACTS[act] + (1 if affine else 0))
    x = torch.randn(G * P, C, generator=g) * 1.5 + 0.25
    dy = torch.randn(G * P, C, generator=g)
    w = ((0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)) if affine else None
    b = 0.2 * torch.randn(C, generator=g) if affine else None
    if fixed_stats:            # eval mode: running statistics, unrelated to the batch
        mean, rstd = 0.3 * torch.randn(G * C, generator=g), 0.5 + torch.rand(G * C, generator=g)
    else:
        mean, rstd = _stats(device, x, G, P, C)
    tag = 'noy %s %s affine=%d fixed=%d' % (shape, act, affine, fixed_stats)
    pair, y = _backward_both(device, x, mean, rstd, w, b, dy, G, P, C, ACTS[act], fixed_stats)
    frac = float((y > 0).float().mean())
    assert 0.05 < frac < 0.95, '%s: %.2f of the outputs positive - the case does not exercise both slopes' % (tag, frac)
    _assert_modes_equal(tag, pair)


def kink_inputs(P, C, seed=203, steps=3):
    """2. mean = 0, rstd = 1, random w; in every channel one pixel at x0 with b[c] = -fl(x0 * w[c]) - multiply-then-add gives exactly
    0 there, a fused multiply-add the rounding residual of x0 * w[c], of either sign - and 2 * steps more pixels at
    nextafter(x0, +-inf) repeated.  Returns x [P][C], w, b and the mask of the planted elements."""
    assert P >= 2 * steps + 2
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, generator=g)
    w = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    x0 = 0.5 + torch.rand(C, generator=g)
    b = -(x0 * w)                                     # fp32 product, rounded once: fl(x0 * w)
    planted = torch.zeros(P, C, dtype=torch.bool)
    rows = torch.randperm(P, generator=g)[:2 * steps + 1]
    x[rows[0]] = x0
    planted[rows[0]] = True
    up, down = x0.clone(), x0.clone()
    for k in range(steps):
        up = torch.nextafter(up, torch.full_like(up, float('inf')))
        down = torch.nextafter(down, torch.full_like(down, -float('inf')))
        x[rows[1 + 2 * k]], x[rows[2 + 2 * k]] = up, down
        planted[rows[1 + 2 * k]] = True
        planted[rows[2 + 2 * k]] = True
    return x, w, b, planted


def check_kink(device, P, C, act):
    """the bit equality of check 1 on elements planted on the kink; at least C of them (the exact zeros alone are C) must have
    |v| < 2^-20 |b|.  Returns that count."""
    x, w, b, planted = kink_inputs(P, C)
    g = torch.Generator().manual_seed(204)
    dy = torch.randn(P, C, generator=g)
    mean, rstd = torch.zeros(C), torch.ones(C)
    v = x * w + b                                    # the forward's arithmetic: multiply, then add, each rounded to fp32
    near = (v.abs() < 2.0 ** -20 * b.abs()) & planted
    count = int(near.sum())
    exact = int(((v == 0) & planted).sum())
    fused = torch.addcmul(b.double(), x.double(), w.double())          # what one fused multiply-add would have kept (exact in fp64)
    flips = int((((fused > 0) != (v > 0)) & planted).sum())
    print('kink %s P=%d C=%d: %d planted elements with |v| < 2^-20 |b| (%d exact zeros), %d of them change sign under a fused '
          'multiply-add' % (act, P, C, count, exact, flips))
    assert count >= C, 'only %d elements on the kink, %d wanted' % (count, C)
    for fixed_stats in (0, 1):
        pair, y = _backward_both(device, x, mean, rstd, w, b, dy, 1, P, C, ACTS[act], fixed_stats)
        _assert_modes_equal('noy kink %s C=%d fixed=%d' % (act, C, fixed_stats), pair)
        # the forward itself sits where the construction says: the planted exact zeros come out as zeros
        assert int(((y.cpu() == 0) & planted).sum()) >= exact
    return count


def check_values(device, P, C, seed=205):
    """3. dx, dw, db of the y-free mode against fp64 autograd through batch_norm(training) + LeakyReLU: `bounded`, inputs and
    references of small_op_checks.check_sync_bn"""
    ops, _ = pkg()
    x, w, b, dy, _, _ = sc._draw_bn_input(P, C, 1, 'lrelu', seed + 7 * P + C)
    ref, base = (sc._bn_backward(x, w, b, dy, 'lrelu', 1, dt) for dt in (torch.float64, torch.float32))
    xd, dyd, wd, bd = (_dev(t, device) for t in (x, dy, w, b))
    mean, rstd = ops.norm_stats(xd, 1, P, C, sc.BN_EPS)
    assert ops.norm_bwd_from_x
    dx, dw, db = ops.bn_backward(dyd, None, xd, mean, rstd, wd, 1, P, C, ACTS['lrelu'], False, True, b=bd)
    tag = 'noy values P=%d C=%d ' % (P, C)
    bounded(tag + 'dx', dx, ref[0], base[0])
    bounded(tag + 'dw', dw.view(1, C), ref[1], base[1])
    bounded(tag + 'db', db.view(1, C), ref[2], base[2])


def check_bad_args(device):
    """y == NULL: tanh / sigmoid, and an affine pair with only one half, are refused; nothing is written"""
    L = lib()
    ops, _ = pkg()
    G, P, C = 1, 8, 4
    x = _dev(torch.randn(P, C), device)
    one = _dev(torch.ones(C), device)
    ws, s = ops._ws(G, P, C, x), torch.zeros(C, device=device)
    dx = torch.zeros_like(x)

    def status(act, w, b):
        return L.call_status('fsv_norm_bwd_fused', L.ptr(x), None, L.ptr(x), L.ptr(one), L.ptr(one), L.ptr(w), L.ptr(b), L.ptr(ws),
                             L.ptr(s), L.ptr(s), L.ptr(dx), None, None, G, P, C, act, 0, ops._ticket(x), None, L.stream_ptr())
    assert status(2, None, None) != 0 and status(3, one, one) != 0          # tanh, sigmoid
    assert status(1, one, None) != 0 and status(1, None, one) != 0
    assert status(1, one, one) == 0 and status(4, None, None) == 0 and status(0, None, None) == 0


# ---------------------------------------------------------------------------------------------------------------- Adam
ADAM_NS = (1, 5, 1027, 4096 + 3)
GUARD = 8


def _adam_one(p, grad, m, v, beta1, beta2, gscale, t, dtype):
    """one step of small_op_checks._adam_ref's formula from given moments, every operation in `dtype`"""
    t_ = lambda s: torch.tensor(s, dtype=dtype)                                    # noqa: E731
    b1, b2, eps, lr, gs = t_(f32(beta1)), t_(f32(beta2)), t_(f32(sc.ADAM_EPS)), t_(f32(sc.LR)), t_(f32(gscale))
    one = t_(1.0)
    bc1, bc2 = one - torch.pow(b1, t_(float(t))), one - torch.pow(b2, t_(float(t)))
    g = grad.to(dtype) * gs
    mn = b1 * m.to(dtype) + (one - b1) * g
    vn = b2 * v.to(dtype) + (one - b2) * g * g
    step_size, rbc2 = lr / bc1, one / torch.sqrt(bc2)
    pn = p.to(dtype) - step_size * (mn / (torch.sqrt(vn) * rbc2 + eps))
    return pn - p.to(dtype), mn, vn            # the update as the stored parameter shows it (check_adam_fp64)


def check_adam_range(device, n, beta1, offset, tick, beta2=0.999, gscale=0.25, seed=207):
    """4. one fsv_adam_step_range on [offset, offset + n) of 16-byte-aligned buffers with GUARD elements on either side, against
    the fp64 step (`bounded`, as check_adam_fp64: the update, m, v); the guard bands keep their bits; at beta1 == 0 the stored m is
    the scaled gradient and an arbitrary finite m before the step changes neither param nor v"""
    L = lib()
    g = torch.Generator().manual_seed(seed + 31 * n + 5 * offset + tick)
    total = GUARD + offset + n + GUARD + 3
    lo = GUARD + offset                                # GUARD is a multiple of 4: the range starts `offset` elements off alignment
    p0, grad = torch.randn(total, generator=g), torch.randn(total, generator=g) * 0.7
    m0 = torch.randn(total, generator=g) * 0.3
    v0 = torch.rand(total, generator=g) * 0.2
    t0 = 3.0                                           # the step count before the call

    def state_for(step):
        b1, b2 = torch.tensor(f32(beta1)), torch.tensor(f32(beta2))
        return torch.tensor([step, float(1 - torch.pow(b1, torch.tensor(step))), float(1 - torch.pow(b2, torch.tensor(step))), sc.LR])

    def run(m_init):
        bufs = [_dev(t.clone(), device) for t in (p0, grad, m_init, v0)]
        assert all(t.data_ptr() % 16 == 0 for t in bufs)
        # tick = 1: the call advances t0 -> t0 + 1 itself; tick = 0: the caller's earlier piece did
        state = _dev(state_for(t0) if tick else state_for(t0 + 1), device)
        at = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * lo)                      # noqa: E731
        L.call('fsv_adam_step_range', at(bufs[0]), at(bufs[1]), at(bufs[2]), at(bufs[3]), L.ptr(state), n, beta1, beta2, sc.ADAM_EPS,
               gscale, tick, L.stream_ptr())
        assert float(state.cpu()[0]) == t0 + 1
        return [t.cpu() for t in bufs]

    got = run(m0)
    tag = 'adam range n=%d beta1=%g offset=%d tick=%d ' % (n, beta1, offset, tick)
    for name, t, t_before in zip(('param', 'grad', 'm', 'v'), got, (p0, grad, m0, v0)):
        same_bits(tag + name + ' guard below', t[:lo], t_before[:lo])
        same_bits(tag + name + ' guard above', t[lo + n:], t_before[lo + n:])
    same_bits(tag + 'grad', got[1], grad)
    sl = slice(lo, lo + n)
    ref = _adam_one(p0[sl], grad[sl], m0[sl], v0[sl], beta1, beta2, gscale, t0 + 1, torch.float64)
    base = _adam_one(p0[sl], grad[sl], m0[sl], v0[sl], beta1, beta2, gscale, t0 + 1, torch.float32)
    bounded(tag + 'update', got[0][sl].double() - p0[sl].double(), ref[0], base[0])
    bounded(tag + 'm', got[2][sl], ref[1], base[1])
    bounded(tag + 'v', got[3][sl], ref[2], base[2])
    if beta1 == 0.0:
        assert torch.equal(got[2][sl], grad[sl] * torch.tensor(f32(gscale))), tag + 'm is not the scaled gradient'
        other = run(torch.randn(total, generator=g) * 50.0)
        same_bits(tag + 'param under another m', other[0], got[0])
        same_bits(tag + 'v under another m', other[3], got[3])
        assert torch.equal(other[2][sl], got[2][sl])


# ------------------------------------------------------------------------------------------------------------- model level
def _one_step(device, opt, b, seed):
    """one D step + one G step of the small fixture of tests/test_model_emu.py: the losses and every parameter gradient"""
    import model_checks as mc
    M = mc._model()
    model = M.create_model(opt)
    mc.fill_state(model.netG), mc.fill_state(model.netD)
    model = model.to(device).train()
    opt_G, opt_D = model.build_optimizers(split_backward=False)
    opt_G.set_lr(0.0); opt_D.set_lr(0.0)
    h, w = int(opt.fineSize / opt.aspect_ratio), opt.fineSize
    tl, ti, rl, ri = [t.to(device) for t in mc.synth_pose_inputs(b, h, w, seed, opt.input_nc)]
    data_list = [tl, ti, [None, None], [None, None], rl, ri, None, None, None]
    d_losses = M.loss_backward(opt, model(data_list, mode='discriminator'), opt_D, 1)
    out = {'loss D %d' % i: v.detach().cpu().clone() for i, v in enumerate(d_losses)}
    grads = {'netD.' + k: p.grad.detach().cpu().clone() for k, p in model.netD.named_parameters() if p.grad is not None}
    g_losses, _, _ = model(data_list, save_images=True, mode='generator')
    g_losses = M.loss_backward(opt, g_losses, opt_G, 0)
    out.update({'loss G %d' % i: v.detach().cpu().clone() for i, v in enumerate(g_losses) if torch.is_tensor(v)})
    grads.update({'netG.' + k: p.grad.detach().cpu().clone() for k, p in model.netG.named_parameters() if p.grad is not None})
    return out, grads


def check_model_step(device, b=2, seed=21):
    """5. ops.norm_bwd_from_x on and off: bit-equal losses and parameter gradients.  Returns (number of y-free backward calls,
    number of compared gradients)."""
    import model_checks as mc
    ops, _ = pkg()
    L = lib()
    seen, real_call = [], L.call

    def recording_call(name, *a):
        if name == 'fsv_norm_bwd_fused':
            seen.append(a[1] is None and a[16] != 0)          # y absent at a site with an activation
        return real_call(name, *a)

    kept = ops.norm_bwd_from_x
    res = {}
    try:
        L.call = recording_call
        for flag in (True, False):
            ops.norm_bwd_from_x = flag
            seen.clear()
            res[flag] = _one_step(device, mc.tiny_opt(warp_ref=True, spade_combine=True, remove_face_labels=True), b, seed)
            res[flag] += (sum(seen),)
    finally:
        L.call = real_call
        ops.norm_bwd_from_x = kept
    (loss_a, grad_a, n_a), (loss_b, grad_b, n_b) = res[True], res[False]
    assert n_a > 0 and n_b == 0, 'y-free backward calls: %d with the flag, %d without' % (n_a, n_b)
    assert loss_a.keys() == loss_b.keys() and grad_a.keys() == grad_b.keys() and len(grad_a) > 20
    for k in loss_a:
        same_bits('model step ' + k, loss_a[k], loss_b[k])
    for k in grad_a:
        same_bits('model step grad ' + k, grad_a[k], grad_b[k])
    print('model step: %d y-free normalisation backward calls, %d losses and %d gradients bit-equal' % (n_a, len(loss_a), len(grad_a)))
    return n_a, len(grad_a)
