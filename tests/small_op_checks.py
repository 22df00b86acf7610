"""Direct checks of the optimiser, loss-scale, cross-replica BatchNorm, max-pool and table-helper entry points, shared by the
emulated (`not gpu`) and the real-hardware (`gpu`) test modules.

Every entry point is driven through the C ABI at the smallest shapes that still cross each of its code paths and compared with
plain PyTorch in fp64 on the CPU, computed from the same seeded fp32 inputs (scalar arguments that travel as `float` - betas,
eps, momentum - enter the reference as their fp32 value).  Where the operation rounds, the tolerance is not a constant: it is
the error of an fp32 PyTorch restatement of the same formula against the fp64 reference, times MARGIN, plus a floor of two fp32
ulp of the compared quantity (`bounded`).  Where it does not round (routing, copies, fixed-order fp32 sums), the comparison is
bit for bit.
"""
import ctypes
import os
import re

import torch
import torch.nn.functional as F

from op_checks import ROOT, _dev, pkg
from oracle.np_oracle import LossScaler

MARGIN = 4.0                                   # the kernel may be this much worse than the fp32 restatement
EPS32 = float(torch.finfo(torch.float32).eps)  # one ulp of a value in [1, 2)
FLT_MAX = float(torch.finfo(torch.float32).max)
ratios = {}                                    # name -> kernel error / restatement error of the last run (`bounded` prints each)


def lib():
    from importlib import import_module
    pkg()
    return import_module('few-shot-vid2vid_amd.lib')


def f32(v):
    """the value a `float` argument of the C ABI carries"""
    return float(torch.tensor(v, dtype=torch.float32))


def bits(t):
    """the tensor's bytes, for comparisons that -0.0 / nan must not blur"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(name, got, ref):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, '%s: %s %s vs %s %s' % (name, got.dtype, tuple(got.shape), ref.dtype,
                                                                                     tuple(ref.shape))
    bad = int((bits(got) != bits(ref)).sum())
    assert bad == 0, '%s: %d of %d elements differ in their bits' % (name, bad, got.numel())


def bounded(name, got, ref64, base32, scale=None):
    """max|got - ref| <= MARGIN * max|base - ref| + 2 ulp, the ulp taken at max|ref| (or at `scale`).  Returns and records
    kernel error / restatement error."""
    got, base = got.detach().cpu().double(), base32.detach().cpu().double()
    ref64 = ref64.detach().cpu()
    assert ref64.dtype == torch.float64 and got.shape == ref64.shape == base.shape, name
    assert bool(torch.isfinite(got).all()), '%s: not finite' % name
    err, berr = float((got - ref64).abs().max()), float((base - ref64).abs().max())
    floor = 2.0 * EPS32 * (float(ref64.abs().max()) if scale is None else scale)
    ratio = err / berr if berr > 0 else (0.0 if err == 0 else float('inf'))
    ratios[name] = ratio
    print('%-58s kernel %.3e  fp32 restatement %.3e  ratio %.2f  floor %.1e' % (name, err, berr, ratio, floor))
    assert err <= MARGIN * berr + floor, '%s: kernel error %.3e > %g * %.3e + %.1e' % (name, err, MARGIN, berr, floor)
    return ratio


# ------------------------------------------------------------------------------------------------------------ Adam family
ADAM_SIZES = (1, 3, 1027, 100003)              # below one float4, a ragged tail, four passes of the grid-stride loop
ADAM_BETAS = ((0.5, 0.999), (0.0, 0.9), (0.9, 0.999))
ADAM_GSCALES = (1.0, 0.25)
LR, ADAM_EPS = 2e-4, 1e-8


def _adam_ref(p0, grads, beta1, beta2, eps, lr, gscale, dtype):
    """the formula of csrc/elementwise.hip (torch.optim.Adam without weight decay / amsgrad), every operation in `dtype`;
    returns the trajectories of p - p0, m, v ([steps][n]) and of state[0..2] ([steps][3])"""
    t_ = lambda s: torch.tensor(s, dtype=dtype)                                    # noqa: E731
    b1, b2, eps, lr, gs = t_(f32(beta1)), t_(f32(beta2)), t_(f32(eps)), t_(f32(lr)), t_(f32(gscale))
    p, m, v = p0.to(dtype), torch.zeros_like(p0, dtype=dtype), torch.zeros_like(p0, dtype=dtype)
    one = t_(1.0)
    up, ms, vs, st = [], [], [], []
    for t, grad in enumerate(grads, 1):
        bc1, bc2 = one - torch.pow(b1, t_(float(t))), one - torch.pow(b2, t_(float(t)))
        step_size, rbc2 = lr / bc1, one / torch.sqrt(bc2)
        g = grad.to(dtype) * gs
        m = b1 * m + (one - b1) * g
        v = b2 * v + (one - b2) * g * g
        p = p - step_size * (m / (torch.sqrt(v) * rbc2 + eps))
        up.append(p - p0.to(dtype)), ms.append(m), vs.append(v), st.append(torch.stack([t_(float(t)), bc1, bc2]))
    return torch.stack(up), torch.stack(ms), torch.stack(vs), torch.stack(st)


def check_adam_fp64(device, betas, gscale, sizes=ADAM_SIZES, steps=24, seed=109):
    """fsv_adam_step over 24 steps against fp64: the whole trajectories of the UPDATE p_t - p_0 (not the parameter: max|p| is
    a thousand updates), of m, of v and of state[0..2] = (t, 1 - beta1^t, 1 - beta2^t).  Tolerance: `bounded`, the update's ulp
    floor taken at max|update|.

    Measured kernel error / restatement error, worst over betas, gscale and n (emulator | MI355X): update 1.00 | 1.00,
    m 1.00 | 1.00, v 1.00 | 1.00, 1 - beta1^t 1.00 | 0.99, 1 - beta2^t 1.00 | 1.00."""
    ops, _ = pkg()
    beta1, beta2 = betas
    for n in sizes:
        g = torch.Generator().manual_seed(seed + n)
        p0 = torch.randn(n, generator=g)
        grads = [torch.randn(n, generator=g) * (0.1 + 2.0 * torch.rand(1, generator=g)) for _ in range(steps)]
        ref = _adam_ref(p0, grads, beta1, beta2, ADAM_EPS, LR, gscale, torch.float64)
        base = _adam_ref(p0, grads, beta1, beta2, ADAM_EPS, LR, gscale, torch.float32)
        pd = _dev(p0.clone(), device)
        m, v = torch.zeros_like(pd), torch.zeros_like(pd)
        state = _dev(torch.tensor([0.0, 0.0, 0.0, LR]), device)
        up, ms, vs, st = [], [], [], []
        for grad in grads:
            ops.adam_step(pd, _dev(grad, device), m, v, state, beta1, beta2, ADAM_EPS, gscale)
            up.append(pd.cpu().double() - p0.double()), ms.append(m.cpu().clone()), vs.append(v.cpu().clone())
            st.append(state.cpu()[:3].clone())
        tag = 'adam betas=%s gscale=%g n=%d ' % (betas, gscale, n)
        assert float(ref[0].abs().max()) < 0.02 * float(p0.abs().max()) or n < 4     # the update IS small next to the parameter
        bounded(tag + 'update', torch.stack(up), ref[0], base[0])
        bounded(tag + 'm', torch.stack(ms), ref[1], base[1])
        bounded(tag + 'v', torch.stack(vs), ref[2], base[2])
        got_st = torch.stack(st)
        same_bits(tag + 'state[0]', got_st[:, 0], torch.arange(1, steps + 1, dtype=torch.float32))
        bounded(tag + 'state[1]', got_st[:, 1], ref[3][:, 1], base[3][:, 1])
        bounded(tag + 'state[2]', got_st[:, 2], ref[3][:, 2], base[3][:, 2])
        assert float(state.cpu()[3]) == f32(LR)


def _adam_buffers(n, seed, steps):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(steps)]
    return p0, grads


def _adam_set(device, p0, warm=0.0):
    pd = _dev(p0.clone(), device)
    return [pd, torch.full_like(pd, warm), torch.full_like(pd, warm * warm), _dev(torch.tensor([0.0, 0.0, 0.0, LR]), device)]


def check_adam_ranges(device, n=5000, cuts=(1027, 1027), betas=(0.5, 0.999), gscale=0.25, steps=3, seed=110):
    """fsv_adam_step_range over three ranges of the flat buffers - [0, 1027) with n % 4 == 3, an EMPTY one, the rest - with the
    tick on the first only == one fsv_adam_step over the whole buffer, bit for bit in param, m, v and state; a further pass
    with tick = 0 everywhere leaves `state` untouched (and steps with the old bias corrections)."""
    ops, _ = pkg()
    p0, grads = _adam_buffers(n, seed, steps + 1)
    whole, parts = _adam_set(device, p0), _adam_set(device, p0)
    edges = [0] + list(cuts) + [n]
    assert edges[1] % 4 != 0 and edges[1] == edges[2] and len(edges) == 4

    L = lib()

    def at(t, a):                              # base + offset, as a C caller would pass it (an empty view has no address)
        return ctypes.c_void_p(t.data_ptr() + 4 * a)

    def ranged(grad, first_tick):
        for k in range(3):
            a, b = edges[k], edges[k + 1]
            L.call('fsv_adam_step_range', at(parts[0], a), at(grad, a), at(parts[1], a), at(parts[2], a), L.ptr(parts[3]), b - a,
                   betas[0], betas[1], ADAM_EPS, gscale, 1 if first_tick and k == 0 else 0, L.stream_ptr())

    for it in range(steps):
        grad = _dev(grads[it], device)
        ops.adam_step(whole[0], grad, whole[1], whole[2], whole[3], betas[0], betas[1], ADAM_EPS, gscale)
        ranged(grad, True)
        for name, a, b in zip(('param', 'm', 'v', 'state'), parts, whole):
            same_bits('adam ranges step %d %s' % (it + 1, name), a, b)
    assert float(parts[3].cpu()[0]) == steps
    before = [t.clone() for t in parts]
    ranged(_dev(grads[steps], device), False)
    same_bits('adam ranges: state after a pass without tick', parts[3], before[3])
    assert int((bits(parts[0]) != bits(before[0])).sum()) > n // 2, 'the pass without tick did not step'


def check_amp_adam(device, n=1027, betas=(0.5, 0.999), gscale=0.25, scale=1024.0, steps=3, seed=111):
    """fsv_amp_adam with found_inf = 0 and a power-of-two scale == fsv_adam_step with gscale / scale on the same (scaled)
    gradients, bit for bit; with found_inf = 1 it leaves param, m, v and state (step count included) byte for byte as they were,
    also when the gradient holds the inf that raised the flag."""
    ops, _ = pkg()
    L = lib()
    p0, grads = _adam_buffers(n, seed, steps + 1)
    plain, amp = _adam_set(device, p0), _adam_set(device, p0)
    scaler = _dev(torch.tensor([scale, 5.0, 0.0, 2000.0, 2.0 ** 24, 1.0]), device)
    words = scaler.clone()

    def amp_adam(grad):
        L.call('fsv_amp_adam', L.ptr(amp[0]), L.ptr(grad), L.ptr(amp[1]), L.ptr(amp[2]), L.ptr(amp[3]), L.ptr(scaler), n,
               betas[0], betas[1], ADAM_EPS, gscale, L.stream_ptr())

    for it in range(steps):
        grad = _dev(grads[it] * scale, device)
        ops.adam_step(plain[0], grad, plain[1], plain[2], plain[3], betas[0], betas[1], ADAM_EPS, gscale / scale)
        amp_adam(grad)
        for name, a, b in zip(('param', 'm', 'v', 'state'), amp, plain):
            same_bits('amp adam step %d %s' % (it + 1, name), a, b)
    same_bits('amp adam: scaler', scaler, words)                 # the step itself never writes the scaler
    before = [t.clone() for t in amp]
    scaler[2] = 1.0
    bad = grads[steps] * scale
    bad[0], bad[n // 2], bad[n - 1] = float('inf'), float('nan'), -float('inf')
    amp_adam(_dev(bad, device))
    for name, a, b in zip(('param', 'm', 'v', 'state'), amp, before):
        same_bits('amp adam skipped step: %s' % name, a, b)
    assert float(scaler.cpu()[2]) == 1.0


# ------------------------------------------------------------------------------------------------------ loss-scale kernels
AMP_CHECK_SIZES = (1, 255, 5000, 3_000_000)
SCALER_WORDS = (1024.0, 7.0, 0.0, 3.0, 65536.0, 0.5)


def amp_check_threads(n):
    """work-items fsv_amp_check launches for n values (csrc/amp.hip fsv_amp_grid: 8 values per work-item, at most 4096 workgroups
    of 256); indices from here on are only reached by a later pass of the grid-stride loop"""
    return min(max((n + 2047) // 2048, 1), 4096) * 256


def check_amp_check(device, n, seed=112):
    """fsv_amp_check: ONE +inf / -inf / nan at index 0, at n - 1 and (where work-items stride: 8 values each at 5000, the capped grid at 3,000,000) at an index
    only the second and only the last pass reach sets found_inf; finite data holding +-FLT_MAX, denormals and -0.0 does not; a
    flag that is set stays set; the other five words of the scaler are never written."""
    L = lib()
    g = torch.Generator().manual_seed(seed)
    host = torch.randn(n, generator=g) * 100.0
    edge = torch.tensor([FLT_MAX, -FLT_MAX, 1e-45, -1e-45, 1.1754942e-38, -1e-40, -0.0, 0.0])
    assert bool(torch.isfinite(edge).all()) and float(edge[2]) > 0 and bits(edge)[6] != bits(edge)[7]
    k = min(n, edge.numel())
    host[torch.arange(k) * (n // k)] = edge[:k]                 # spread over the buffer
    if n >= 2:
        host[0], host[n - 1] = FLT_MAX, -FLT_MAX
    assert bool(torch.isfinite(host).all())
    grad = _dev(host, device)
    threads = amp_check_threads(n)
    spots = [0, n - 1]
    if n > threads:
        spots += [threads + 17, n - 1 - 17]
        assert threads + 17 < n and (n - 1 - 17) // threads == (n - 1) // threads >= 2
    else:
        assert n <= 256                        # one pass: 1 and 255; 5000 and 3,000,000 take the branch above
    spots = sorted(set(spots))

    def run(flag):
        scaler = _dev(torch.tensor(SCALER_WORDS), device)
        scaler[2] = flag
        L.call('fsv_amp_check', L.ptr(grad), n, L.ptr(scaler), L.stream_ptr())
        got = scaler.cpu()
        keep = [0, 1, 3, 4, 5]
        same_bits('amp check n=%d: the other scaler words' % n, got[keep], torch.tensor(SCALER_WORDS)[keep])
        return float(got[2])

    assert run(0.0) == 0.0, 'n=%d: finite gradients (FLT_MAX, denormals, -0.0) were flagged' % n
    assert run(1.0) == 1.0, 'n=%d: a set flag was cleared' % n
    for bad in (float('inf'), -float('inf'), float('nan')):
        for i in spots:
            old = grad[i].clone()
            grad[i] = bad
            assert run(0.0) == 1.0, 'n=%d: %r at index %d was not found' % (n, bad, i)
            grad[i] = old
    assert run(0.0) == 0.0


def check_amp_update(device):
    """fsv_amp_update against oracle/np_oracle.LossScaler (apex's rule) over scripted good (0) / bad (1) steps with window 3:
    halving down to min_scale and staying there, the good-step counter reset by an overflow one step before the window closes,
    doubling every third good step up to max_scale and staying there; after every step scale and counter agree bit for bit,
    found_inf is cleared and window / max_scale / min_scale are as they were."""
    L = lib()
    for init, lo, hi, script in [(4.0, 1.0, 16.0, [1, 1, 1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0] + [0] * 12 + [1, 0, 0, 0]),
                                 (2.0 ** 16, 2.0 ** 15, 2.0 ** 17, [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0])]:
        ref = LossScaler(init_scale=init, window=3, max_scale=hi, min_scale=lo)
        scaler = _dev(torch.tensor([init, 0.0, 0.0, 3.0, hi, lo]), device)
        seen = set()
        for k, found in enumerate(script):
            if found:
                scaler[2] = 1.0
            L.call('fsv_amp_update', L.ptr(scaler), L.stream_ptr())
            old = (ref.scale, ref.good)
            ref.update(bool(found))
            want = torch.tensor([ref.scale, float(ref.good), 0.0, 3.0, hi, lo])
            same_bits('amp update step %d of %s' % (k, script), scaler, want)
            seen.add(('halved' if ref.scale < old[0] else 'floor') if found else
                     ('doubled' if ref.scale > old[0] else 'cap' if ref.good == 0 else 'counted'))
            if found and old[1] == 2:
                seen.add('reset before the window closed')
        assert seen == {'halved', 'floor', 'doubled', 'cap', 'counted', 'reset before the window closed'}, seen


# ------------------------------------------------------------------------------- cross-replica BatchNorm on one device
SYNC_BN_SHAPES = ((35, 10), (1000, 7), (4096, 64), (300, 260))     # odd P, C % 4 != 0 (scalar kernels), C above one channel slab
BN_EPS, BN_MOMENTUM, KINK = 1e-5, 0.1, 1e-4
_ACT = {'none': 0, 'lrelu': 1}


def _bn_forward(x, w, b, rm0, rv0, dtype):
    """batch statistics of [n][C] and the nn.BatchNorm2d running-statistics rule, every operation in `dtype`"""
    x, n = x.to(dtype), x.shape[0]
    eps, mom = torch.tensor(f32(BN_EPS), dtype=dtype), torch.tensor(f32(BN_MOMENTUM), dtype=dtype)
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    rm = (1 - mom) * rm0.to(dtype) + mom * mean
    rv = (1 - mom) * rv0.to(dtype) + mom * (var * (n / (n - 1.0)))
    pre = (x - mean) * rstd * w.to(dtype) + b.to(dtype)
    return mean, rstd, rm, rv, pre


def _bn_backward(x, w, b, dy, act, world, dtype):
    """autograd through F.batch_norm(training) + activation on the concatenated tensor -> dx; every shard's share of dw / db"""
    xr, wr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    pre = F.batch_norm(xr, None, None, wr, br, True, 0.0, f32(BN_EPS))
    y = F.leaky_relu(pre, 0.2) if act == 'lrelu' else pre
    y.backward(dy.to(dtype))
    with torch.no_grad():
        slope = torch.where(pre > 0, torch.ones((), dtype=dtype), torch.full((), 0.2, dtype=dtype)) if act == 'lrelu' else 1.0
        d = dy.to(dtype) * slope
        xhat = (xr - xr.mean(0)) / torch.sqrt(xr.var(0, unbiased=False) + f32(BN_EPS))
        C = x.shape[1]
        dw = (d * xhat).view(world, -1, C).sum(1)
        db = d.view(world, -1, C).sum(1)
    if dtype == torch.float64:
        assert torch.allclose(dw.sum(0), wr.grad, rtol=1e-9, atol=1e-12) and torch.allclose(db.sum(0), br.grad, rtol=1e-9, atol=1e-12)
    return xr.grad, dw, db


def _draw_bn_input(P, C, world, act, seed, offset=0.25, spread=1.5):
    """seeded inputs with no pre-activation within KINK of the LeakyReLU kink: the few values that land there (about one in
    ten thousand) are moved half a per-mille of a standard deviation away from it, then the condition is asserted"""
    g = torch.Generator().manual_seed(seed)
    n = P * world
    x = torch.randn(n, C, generator=g) * spread + offset
    w = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)    # some negative
    b = 0.2 * torch.randn(C, generator=g)
    dy = torch.randn(n, C, generator=g)
    rm0, rv0 = 0.5 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    for _ in range(8):
        pre = _bn_forward(x, w, b, rm0, rv0, torch.float64)[4]
        close = pre.abs() < 4 * KINK
        if act != 'lrelu' or not bool(close.any()):
            break
        away = torch.where(pre >= 0, 1.0, -1.0) * torch.sign(w).double() * (spread * 5e-3)
        x = torch.where(close, (x.double() + away).float(), x)
    pre = _bn_forward(x, w, b, rm0, rv0, torch.float64)[4]
    assert act != 'lrelu' or float(pre.abs().min()) >= KINK, 'a pre-activation lies within %g of the kink' % KINK
    assert act != 'lrelu' or (bool((pre > 0).any()) and bool((pre < 0).any()))
    return x, w, b, dy, rm0, rv0


def _sync_bn_kernels(device, x, w, b, dy, rm0, rv0, P, C, world, act):
    """what ops.norm_stats / ops.bn_backward do around their two all-reduces, the all-reduce being torch.add over the shards"""
    ops, _ = pkg()
    L = lib()
    st = L.stream_ptr()
    xs = [_dev(x[r * P:(r + 1) * P].contiguous(), device) for r in range(world)]
    dys = [_dev(dy[r * P:(r + 1) * P].contiguous(), device) for r in range(world)] if dy is not None else None
    wd, bd = _dev(w, device), _dev(b, device)
    ws = ops._ws(1, P, C, xs[0])
    total = None
    for r in range(world):
        sums = torch.empty(2 * C, dtype=torch.float64, device=device)
        L.call('fsv_norm_sums', L.ptr(xs[r]), L.ptr(ws), L.ptr(sums), P, C, st)
        total = sums if total is None else torch.add(total, sums)
    mean, rstd = torch.empty(C, device=device), torch.empty(C, device=device)
    rm, rv = _dev(rm0.clone(), device), _dev(rv0.clone(), device)
    L.call('fsv_norm_stats_from_sums', L.ptr(total), float(P) * world, L.ptr(mean), L.ptr(rstd), C, BN_EPS, L.ptr(rm), L.ptr(rv),
           BN_MOMENTUM, st)
    out = dict(mean=mean, rstd=rstd, rm=rm, rv=rv)
    if dy is None:
        return out
    ys, local = [], []
    for r in range(world):
        y = torch.empty_like(xs[r])
        L.call('fsv_norm_apply', L.ptr(xs[r]), L.ptr(mean), L.ptr(rstd), L.ptr(wd), L.ptr(bd), L.ptr(y), 1, P, C, _ACT[act], None, st)
        ys.append(y)
        sums = torch.empty(2 * C, dtype=torch.float64, device=device)
        L.call('fsv_norm_bwd_sums', L.ptr(dys[r]), L.ptr(y), L.ptr(xs[r]), L.ptr(mean), L.ptr(rstd), L.ptr(ws), L.ptr(sums), P, C,
               _ACT[act], st)
        local.append(sums)
    total = local[0]
    for s in local[1:]:
        total = torch.add(total, s)
    s = total.float()
    s1, s2 = s[:C].contiguous(), s[C:].contiguous()
    dxs = []
    for r in range(world):
        dx = torch.full_like(xs[r], float('nan'))
        L.call('fsv_norm_bwd_apply', L.ptr(dys[r]), L.ptr(ys[r]), L.ptr(xs[r]), L.ptr(mean), L.ptr(rstd), L.ptr(wd), L.ptr(s1),
               L.ptr(s2), L.ptr(dx), P, C, P * world, _ACT[act], None, st)
        dxs.append(dx)
    # the parameter gradients are the LOCAL sums (ops.bn_backward: they are averaged over the replicas with every other gradient)
    out.update(dx=torch.cat(dxs), db=torch.stack([t[:C].float() for t in local]), dw=torch.stack([t[C:].float() for t in local]))
    if world == 1:
        out['dx_fused'] = ops.bn_backward(dys[0], ys[0], xs[0], mean, rstd, wd, 1, P, C, _ACT[act], False, True)[0]
    return out


def check_sync_bn(device, P, C, world, act, seed=113):
    """fsv_norm_sums -> (sum over the shards) -> fsv_norm_stats_from_sums(count = P * world) and fsv_norm_bwd_sums -> (sum) ->
    fsv_norm_bwd_apply(count = P * world) on `world` equal shards of one [P * world][C] tensor, against fp64 batch statistics /
    fp64 autograd through batch_norm(training) + activation of the WHOLE tensor: mean, rstd, running mean and (unbiased, n = P *
    world) variance, dx, and every shard's LOCAL sums against that shard's share of dw / db.  world == 1: dx also agrees with
    fsv_norm_bwd_fused within the same bound.  Tolerance per quantity: `bounded`.

    Measured kernel error / restatement error, worst over shapes, worlds and activations (emulator | MI355X):
    mean 0.83 | 0.83, rstd 0.99 | 0.94, running mean 1.00 | 1.00, running var 1.34 | 1.34, dx 1.30 | 1.15, dw 1.21 | 1.01,
    db 0.83 | 0.83; world == 1: |dx - fused dx| / restatement error 0.46 | 0.46."""
    x, w, b, dy, rm0, rv0 = _draw_bn_input(P, C, world, act, seed + 7 * P + C + world)
    got = _sync_bn_kernels(device, x, w, b, dy, rm0, rv0, P, C, world, act)
    ref, base = (_bn_forward(x, w, b, rm0, rv0, dt) for dt in (torch.float64, torch.float32))
    tag = 'sync bn P=%d C=%d world=%d %s ' % (P, C, world, act)
    for k, name in enumerate(('mean', 'rstd', 'rm', 'rv')):
        bounded(tag + name, got[name], ref[k], base[k])
    ref, base = (_bn_backward(x, w, b, dy, act, world, dt) for dt in (torch.float64, torch.float32))
    for k, name in enumerate(('dx', 'dw', 'db')):
        bounded(tag + name, got[name], ref[k], base[k])
    if world == 1:
        err_b = float((base[0].double() - ref[0]).abs().max())
        floor = 2.0 * EPS32 * float(ref[0].abs().max())
        gap = float((got['dx'].cpu().double() - got['dx_fused'].cpu().double()).abs().max())
        ratios[tag + 'dx vs fused'] = gap / err_b
        print('%-58s gap %.3e  ratio %.2f' % (tag + 'dx vs fused', gap, gap / err_b))
        assert gap <= MARGIN * err_b + floor, '%s: split and fused dx differ by %.3e' % (tag, gap)


def check_sync_bn_cancellation(device, P=1000, C=7, world=2, seed=114):
    """x = 100 + 0.01 * randn: fp32 sums lose the variance (E[x^2] - mean^2 cancels eight digits; the fp32 restatement is not
    a usable baseline here), the kernels' fp64 sums of the fp32 data do not: relative cancellation loss 1e4 / 1e-4 * 2^-53 ~ 1e-8,
    the rest is the fp32 rounding of the result -> rstd within 1e-5 relative of fp64; the mean within two ulp.  Measured:
    3.8e-8 (emulator and MI355X) - and 0.80 while fsv_norm_sums still summed fp32 products in fp32 within a work-item."""
    g = torch.Generator().manual_seed(seed)
    x = 100.0 + 0.01 * torch.randn(P * world, C, generator=g)
    one, zero = torch.ones(C), torch.zeros(C)
    got = _sync_bn_kernels(device, x, one, zero, None, zero, one, P, C, world, 'none')
    mean, rstd, rm, rv, _ = _bn_forward(x, one, zero, zero, one, torch.float64)
    rel = float(((got['rstd'].cpu().double() - rstd) / rstd).abs().max())
    print('sync bn cancellation: rstd relative error %.3e' % rel)
    assert rel <= 1e-5, 'rstd relative error %.3e' % rel
    assert float((got['mean'].cpu().double() - mean).abs().max()) <= 2 * EPS32 * 100.0
    assert float(((got['rv'].cpu().double() - rv) / rv).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------ max pooling
MAXPOOL_SHAPES = ((1, 2, 2, 1), (2, 7, 5, 3), (1, 6, 9, 64), (2, 16, 16, 130))     # (N, H, W, C)
_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))                           # positions (0,0),(0,1),(1,0),(1,1) = 0..3


def _windows(x):
    """[N][C][H/2][W/2][4]: the four values of every pooling window in the order (0,0),(0,1),(1,0),(1,1)"""
    n, c, h, w = x.shape
    v = x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(n, c, h // 2, 2, w // 2, 2)
    return v.permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)


def _tie_input(n, h, w, c, g):
    """relu(randn) with about 40 % of the windows all zero and 6 x 5 % holding a two-way tie of their maximum, one share per
    position pair; asserts that every kind is there (as many kinds as there are windows, for the one-window shape)"""
    x = torch.relu(torch.randn(n, c, h, w, generator=g))
    win = _windows(x).clone()
    nwin = win[..., 0].numel()
    kind = torch.full((nwin,), -1, dtype=torch.long)
    order = torch.randperm(nwin, generator=g)
    n_zero, n_pair = max(int(0.4 * nwin), 1), max(int(0.05 * nwin), 1)
    kind[order[:n_zero]] = 0
    for k in range(6):
        kind[order[n_zero + k * n_pair:n_zero + (k + 1) * n_pair]] = 1 + k
    flat = win.view(nwin, 4)
    flat[kind == 0] = 0.0
    top = flat.max(dim=1).values + 1.0
    for k, (i, j) in enumerate(_PAIRS):
        sel = kind == 1 + k
        flat[sel, i] = top[sel]
        flat[sel, j] = top[sel]
    x[:, :, :h // 2 * 2, :w // 2 * 2] = flat.view(n, c, h // 2, w // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2 * 2, w // 2 * 2)
    win = _windows(x).reshape(nwin, 4)
    is_max = win == win.max(dim=1, keepdim=True).values
    present = int((is_max.all(dim=1) & (win == 0).all(dim=1)).sum() > 0)
    for i, j in _PAIRS:
        only = torch.zeros(4, dtype=torch.bool)
        only[[i, j]] = True
        present += int((is_max == only).all(dim=1).sum() > 0)
    assert present == min(nwin, 7), 'only %d of the 7 kinds of tie are in the input' % present
    return x


def check_maxpool2(device, shape, seed=115):
    """ops.maxpool2 (fsv_maxpool2_fwd / _bwd) == F.max_pool2d(2, 2) and its autograd, bit for bit (max and routing do not round):
    randn, relu(randn) with all-zero windows and two-way ties in each of the six position pairs (the gradient goes to the FIRST
    maximum in (0,0),(0,1),(1,0),(1,1) order), and all-negative values; the row / column an odd H / W drops gets gradient 0."""
    ops, _ = pkg()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    inputs = [('randn', torch.randn(n, c, h, w, generator=g)), ('ties', _tie_input(n, h, w, c, g)),
              ('negative', -(torch.randn(n, c, h, w, generator=g).abs() + 0.1))]
    for name, x in inputs:
        xr = x.double().requires_grad_(True)
        ref = F.max_pool2d(xr, 2, 2)
        dy = torch.randn(ref.shape, generator=g) + 3.0          # no zero: a mis-routed gradient cannot hide
        ref.backward(dy.double())
        xd = _dev(x, device).requires_grad_(True)
        y = ops.maxpool2(xd)
        y.backward(_dev(dy, device))
        assert tuple(y.shape) == (n, c, h // 2, w // 2)
        same_bits('maxpool %s %s y' % (shape, name), y.contiguous(), ref.detach().float())
        dx = xd.grad.cpu().contiguous()
        same_bits('maxpool %s %s dx' % (shape, name), dx, xr.grad.float())
        assert int((dx != 0).sum()) == ref.numel()              # one receiver per window
        if h % 2:
            assert not bool(dx[:, :, h - 1, :].any()), 'gradient in the dropped row'
        if w % 2:
            assert not bool(dx[:, :, :, w - 1].any()), 'gradient in the dropped column'


# ---------------------------------------------------------------------------------------------------------- table helpers
def _guarded(n, device, g, pad=4):
    """(buffer, view of n floats inside it): `pad` guard words on either side (pad = 4 keeps the view 16-byte aligned)"""
    buf = _dev(torch.randn(n + 2 * pad, generator=g) * 3.0 + 10.0, device)
    return buf, buf[pad:pad + n]


def _guards_untouched(name, buf, before, n, pad=4):
    same_bits(name + ': guard words in front', buf[:pad], before[:pad])
    same_bits(name + ': guard words behind', buf[pad + n:], before[pad + n:])


def check_sum_terms(device, nsrcs, counts, seed=116):
    """fsv_sum_terms over len(nsrcs) jobs == the left-to-right fp32 sum ((a + b) + c) + d of PyTorch, bit for bit, with terms of
    mixed magnitude for which the right-to-left sum has other bits (asserted); nothing is written outside dst."""
    L = lib()
    g = torch.Generator().manual_seed(seed)
    njobs = len(nsrcs)
    mags = (1e4, 1.0, 1e-3, 1e-3)          # the small terms decide how round(1e4 + 1) falls only when they are added first
    dsts, srcs, want, bufs = [], [], [], []
    for ns, cnt in zip(nsrcs, counts):
        terms = [torch.randn(cnt, generator=g) * mags[t] for t in range(ns)]
        for t, planted in enumerate((16384.0, 1.0006, 0.0006, 0.0006)[:ns]):      # half an ulp of 16385 is 0.00098: left to right
            terms[t][:4] = planted                                                 # drops both small terms, right to left keeps them
        left = terms[0].clone()
        for t in terms[1:]:
            left = left + t
        if ns >= 3:
            right = terms[-1].clone()
            for t in reversed(terms[:-1]):
                right = t + right
            assert int((bits(left) != bits(right)).sum()) >= max(cnt // 8, 4), 'the order of summation would not show'
        buf, dst = _guarded(cnt, device, g)
        bufs.append((buf, buf.clone(), cnt))
        dsts.append(dst)
        srcs.append([_dev(t, device) for t in terms])
        want.append(left)
    dptr = (ctypes.c_void_p * njobs)(*[d.data_ptr() for d in dsts])
    sptr = (ctypes.c_void_p * (4 * njobs))()
    for j, ts in enumerate(srcs):
        for t, s in enumerate(ts):
            assert s.data_ptr() % 16 == 0 and dsts[j].data_ptr() % 16 == 0
            sptr[4 * j + t] = s.data_ptr()
    L.check_device(*dsts)
    L.call('fsv_sum_terms', dptr, sptr, L.int_array(nsrcs), (ctypes.c_longlong * njobs)(*counts), njobs, L.stream_ptr())
    for j in range(njobs):
        name = 'sum_terms job %d of %d (%d terms, %d values)' % (j, njobs, nsrcs[j], counts[j])
        same_bits(name, dsts[j], want[j])
        _guards_untouched(name, *bufs[j])


def check_gather_add(device, sizes, seed=117):
    """fsv_gather_add over len(sizes) jobs: dst (non-zero before) == dst + src in fp32, bit for bit; one guard word before and
    behind every dst is untouched (sizes straddle the 4096-element chunk of the block map)."""
    L = lib()
    g = torch.Generator().manual_seed(seed)
    jobs, words, tmap = [], [], []
    for j, n in enumerate(sizes):
        buf, dst = _guarded(n, device, g, pad=1)
        src = _dev(torch.randn(n, generator=g), device)
        jobs.append((buf, buf.clone(), dst, src, n))
        words += [src.data_ptr(), dst.data_ptr(), n]
        tmap += [v for chunk in range((n + 4095) // 4096) for v in (j, chunk)]
    table = torch.tensor(words, dtype=torch.int64, device=device)
    tm = torch.tensor(tmap, dtype=torch.int32, device=device)
    L.call('fsv_gather_add', L.ptr(table), len(sizes), L.ptr(tm), len(tmap) // 2, L.stream_ptr())
    for j, (buf, before, dst, src, n) in enumerate(jobs):
        name = 'gather_add job %d of %s' % (j, list(sizes))
        same_bits(name, dst, before[1:1 + n] + src)
        _guards_untouched(name, buf, before, n, pad=1)


def upload_words_per_launch():
    """FSV_UPLOAD_WORDS of csrc/wgrad_finalize.hip: the 64-bit words one launch of fsv_upload_i64 carries in its kernel
    arguments.  The entry point has no upper limit on n - it issues one launch per that many words"""
    src = open(os.path.join(ROOT, 'few-shot-vid2vid_amd', 'csrc', 'wgrad_finalize.hip')).read()
    return int(re.search(r'#define\s+FSV_UPLOAD_WORDS\s+(\d+)', src).group(1))


def check_upload_i64(device, n, seed=118):
    """fsv_upload_i64: n host words arrive exactly - every one of the 64 bits significant - and the words behind them keep
    their contents."""
    L = lib()
    g = torch.Generator().manual_seed(seed + n)
    hi = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64)
    lo = torch.randint(0, 2 ** 32, (n,), generator=g, dtype=torch.int64)
    vals = (hi << 32) | lo
    special = [-1, -2 ** 63, 2 ** 63 - 1, 0x0123456789ABCDEF, 0, 1 << 32, -(1 << 32) - 1]
    vals[torch.arange(min(n, len(special))) * max(n // len(special), 1) % n] = torch.tensor(special[:n])
    vals[n - 1] = -0x0123456789ABCDF0
    assert n < 3 or (bool((vals < 0).any()) and bool((vals >> 32 != 0).any()) and bool((vals & 0xFFFFFFFF != 0).any()))
    sentinel = 0x5A5A5A5A5A5A5A5A
    dst = torch.full((n + 8,), sentinel, dtype=torch.int64, device=device)
    host = (ctypes.c_longlong * n)(*vals.tolist())
    L.call('fsv_upload_i64', L.ptr(dst), host, n, L.stream_ptr())
    got = dst.cpu()
    assert torch.equal(got[:n], vals), 'upload of %d words: %d differ' % (n, int((got[:n] != vals).sum()))
    assert bool((got[n:] == sentinel).all()), 'upload of %d words wrote behind them' % n


# ------------------------------------------------------------------------- two-launch forms of the column reductions
def check_two_launch_reductions(device, P, C, act='lrelu', seed=119):
    """fsv_norm_stats, fsv_norm_stats_rep (rep = 4: only the unbiased running-variance factor counts 4 P values), fsv_colsum and
    fsv_norm_bwd called as entry points (the suite otherwise reaches them only from inside their fused forms, above the
    fused-size threshold) against the fp64 references of check_sync_bn with world = 1; tolerance `bounded`.

    Measured kernel error / restatement error, worst over the shapes and quantities: 1.10 (running variance) on the emulator
    and on an MI355X alike; every other quantity is at or below 1.00."""
    ops, _ = pkg()
    L = lib()
    st = L.stream_ptr()
    x, w, b, dy, rm0, rv0 = _draw_bn_input(P, C, 1, act, seed + P + C)
    xd, dyd, wd, bd = (_dev(t, device) for t in (x, dy, w, b))
    ws = ops._ws(1, P, C, xd)
    ref, base = (_bn_forward(x, w, b, rm0, rv0, dt) for dt in (torch.float64, torch.float32))
    tag = 'two-launch P=%d C=%d ' % (P, C)
    for rep in (1, 4):
        mean, rstd = torch.empty(C, device=device), torch.empty(C, device=device)
        rm, rv = _dev(rm0.clone(), device), _dev(rv0.clone(), device)
        if rep == 1:
            L.call('fsv_norm_stats', L.ptr(xd), L.ptr(ws), L.ptr(mean), L.ptr(rstd), 1, P, C, BN_EPS, L.ptr(rm), L.ptr(rv), BN_MOMENTUM, st)
        else:
            L.call('fsv_norm_stats_rep', L.ptr(xd), L.ptr(ws), L.ptr(mean), L.ptr(rstd), 1, P, C, BN_EPS, L.ptr(rm), L.ptr(rv),
                   BN_MOMENTUM, rep, st)
        n = float(P * rep)
        # the running variance with the factor n / (n - 1) of the repeated tensor, from the same biased variance
        rv_ref, rv_base = ((1 - torch.tensor(f32(BN_MOMENTUM), dtype=dt)) * rv0.to(dt) + torch.tensor(f32(BN_MOMENTUM), dtype=dt)
                           * (x.to(dt).var(0, unbiased=False) * (n / (n - 1.0))) for dt in (torch.float64, torch.float32))
        for name, got, r, bs in (('mean', mean, ref[0], base[0]), ('rstd', rstd, ref[1], base[1]), ('rm', rm, ref[2], base[2]),
                                 ('rv', rv, rv_ref, rv_base)):
            bounded(tag + 'rep=%d %s' % (rep, name), got, r, bs)
    out = _dev(torch.ones(C), device)
    L.call('fsv_colsum', L.ptr(xd), L.ptr(ws), L.ptr(out), 1, P, C, 1, st)
    bounded(tag + 'colsum (accumulating)', out, 1.0 + x.double().sum(0), 1.0 + x.sum(0))
    y = torch.empty_like(xd)
    L.call('fsv_norm_apply', L.ptr(xd), L.ptr(mean), L.ptr(rstd), L.ptr(wd), L.ptr(bd), L.ptr(y), 1, P, C, _ACT[act], None, st)
    s1, s2, dw, db = (torch.empty(C, device=device) for _ in range(4))
    dx = torch.full_like(xd, float('nan'))
    L.call('fsv_norm_bwd', L.ptr(dyd), L.ptr(y), L.ptr(xd), L.ptr(mean), L.ptr(rstd), L.ptr(wd), L.ptr(ws), L.ptr(s1), L.ptr(s2),
           L.ptr(dx), L.ptr(dw), L.ptr(db), 1, P, C, _ACT[act], 0, None, st)
    ref, base = (_bn_backward(x, w, b, dy, act, 1, dt) for dt in (torch.float64, torch.float32))
    for name, got, r, bs in (('dx', dx, ref[0], base[0]), ('dw', dw, ref[1][0], base[1][0]), ('db', db, ref[2][0], base[2][0])):
        bounded(tag + name, got, r, bs)


# ------------------------------------------------------------------------------------------------------ fsv_act_fwd
ACT_SIZES = (1, 3, 1027, 4096, 100003)         # below four values, total % 4 != 0 and == 0, four passes of the grid-stride loop
ACT_CODES = (('none', 0), ('lrelu', 1), ('tanh', 2), ('sigmoid', 3), ('relu', 4), ('lrelu01', 5))


def check_act_fwd(device, total, seed=120):
    """fsv_act_fwd for every activation code of the element-wise kernel (FSV_ACT_DLRELU exists in the GEMM epilogue only), on
    3 * randn with +-0.0, +-50 and +-1e-30 planted.  none / relu route (bit for bit, relu(-0.0) = +0.0 as `v > 0 ? v : 0`); the
    leaky forms are ONE fp32 product with the fp32 slope, so they equal the rounded exact product bit for bit; tanh / sigmoid are
    compared element by element in ulp of the fp64 value: at most MARGIN times the worst ulp error of torch's own fp32
    tanh / sigmoid on the same values, plus 2 ulp.

    Measured worst ulp error, kernel | torch fp32: tanh 1.26 | 0.52 on the emulator, 1.19 | 0.50 on an MI355X; sigmoid
    0.97 | 0.97 and 1.02 | 0.97."""
    L = lib()
    g = torch.Generator().manual_seed(seed + total)
    x = torch.randn(total, generator=g) * 3.0
    edge = torch.tensor([0.0, -0.0, 50.0, -50.0, 1e-30, -1e-30])
    k = min(total, edge.numel())
    x[torch.arange(k) * (total // k)] = edge[:k]
    xd = _dev(x, device)
    x64 = x.double()
    for name, code in ACT_CODES:
        y = torch.full_like(xd, float('nan'))
        L.call('fsv_act_fwd', L.ptr(xd), L.ptr(y), total, code, L.stream_ptr())
        tag = 'act_fwd %s total=%d' % (name, total)
        if name == 'none':
            same_bits(tag, y, x)
        elif name == 'relu':
            same_bits(tag, y, torch.where(x > 0, x, torch.zeros(())))
        elif name in ('lrelu', 'lrelu01'):
            slope = f32(0.2 if name == 'lrelu' else 0.1)
            same_bits(tag, y, torch.where(x > 0, x, (x64 * slope).float()))      # the fp64 product of two floats is exact
        else:
            ref = torch.tanh(x64) if name == 'tanh' else torch.sigmoid(x64)
            base = torch.tanh(x) if name == 'tanh' else torch.sigmoid(x)
            assert float(ref.abs().min()) == 0.0 or float(ref.abs()[ref != 0].min()) > 1e-37        # no denormal results
            ulp = EPS32 * ref.abs().clamp_min(1e-37)
            err = float(((y.cpu().double() - ref).abs() / ulp).max())
            berr = float(((base.double() - ref).abs() / ulp).max())
            print('%-40s kernel %.2f ulp  torch fp32 %.2f ulp' % (tag, err, berr))
            assert bool(torch.isfinite(y).all()) and err <= MARGIN * berr + 2.0, '%s: %.2f ulp against %.2f ulp' % (tag, err, berr)


# ------------------------------------------------------------------------------------------------------ fsv_bias_act
BIAS_ACT_TOTALS = (1, 7, 4099)                 # one value, below two float4, two passes of the grid-stride loop ending inside a pixel
BIAS_ACT_CHANNELS = (1, 3, 64)


def check_bias_act(device, seed=121):
    """fsv_bias_act, in place: x = act(x + bias[i % C]) over `total` values of an NHWC tensor, every total of BIAS_ACT_TOTALS with
    every C of BIAS_ACT_CHANNELS and every activation code of ACT_CODES (those of the convolution epilogue, and 5 = leaky 0.1).
    The sum is ONE fp32 addition, so it equals the rounded fp64 sum bit for bit; none / relu route it, the leaky forms are one
    more exact-product rounding (all four: bit for bit); tanh / sigmoid are compared with the fp64 function of that fp32 sum in
    ulp of the result: at most MARGIN times the worst ulp error of torch's own fp32 tanh / sigmoid on the same sums, plus 2 ulp.
    Guard words around x keep their bits.  Returns the number of launches.

    Measured worst ulp error, kernel | torch fp32: tanh 1.28 | 0.49 on the emulator, 1.01 | 0.49 on an MI355X; sigmoid
    0.97 | 0.94 and 1.04 | 0.94."""
    L = lib()
    ran = 0
    for total in BIAS_ACT_TOTALS:
        for C in BIAS_ACT_CHANNELS:
            g = torch.Generator().manual_seed(seed + 100 * total + C)
            x = torch.randn(total, generator=g) * 3.0
            bias = torch.randn(C, generator=g)
            edge = torch.tensor([0.0, -0.0, 50.0, -50.0])
            k = min(total, edge.numel())
            x[torch.arange(k) * (total // k)] = edge[:k]
            s64 = x.double() + bias.double()[torch.arange(total) % C]
            s = s64.float()                                            # the fp32 sum (the fp64 sum of two floats of like size is exact)
            s64 = s.double()
            bd = _dev(bias, device)
            for name, code in ACT_CODES:
                buf = _dev(torch.cat([torch.full((4,), 7.5), x, torch.full((4,), 7.5)]), device)
                before = buf.clone()
                y = buf[4:4 + total]
                L.check_device(buf, bd)
                L.call('fsv_bias_act', L.ptr(y), L.ptr(bd), total, C, code, L.stream_ptr())
                ran += 1
                tag = 'bias_act %s total=%d C=%d' % (name, total, C)
                _guards_untouched(tag, buf, before, total)
                if name == 'none':
                    same_bits(tag, y, s)
                elif name == 'relu':
                    same_bits(tag, y, torch.where(s > 0, s, torch.zeros(())))
                elif name in ('lrelu', 'lrelu01'):
                    same_bits(tag, y, torch.where(s > 0, s, (s64 * f32(0.2 if name == 'lrelu' else 0.1)).float()))
                else:
                    ref = torch.tanh(s64) if name == 'tanh' else torch.sigmoid(s64)
                    base = torch.tanh(s) if name == 'tanh' else torch.sigmoid(s)
                    ulp = EPS32 * ref.abs().clamp_min(1e-37)
                    err = float(((y.cpu().double() - ref).abs() / ulp).max())
                    berr = float(((base.double() - ref).abs() / ulp).max())
                    print('%-40s kernel %.2f ulp  torch fp32 %.2f ulp' % (tag, err, berr))
                    assert bool(torch.isfinite(y).all()) and err <= MARGIN * berr + 2.0, '%s: %.2f ulp against %.2f ulp' % (tag, err, berr)
    return ran


# ------------------------------------------------------------------------------------------------------ fsv_blend_bwd
def _ncp(t, layout, device):
    """device copy of t [N][C][P] in `layout` -> (tensor that owns the storage, address of element (0, 0, 0), (batch, channel,
    pixel) strides in elements)"""
    n, c, p = t.shape
    if layout == 'nchw':
        d = _dev(t.contiguous(), device)
        return d, d.data_ptr(), (c * p, p, 1)
    if layout == 'nhwc':
        d = _dev(t.permute(0, 2, 1).contiguous(), device)
        return d, d.data_ptr(), (p * c, 1, c)
    assert layout == 'slice'                   # channels 1 .. C of a wider NCHW tensor, as the generator passes image slices
    wide = torch.full((n, c + 2, p), 1e6)
    wide[:, 1:c + 1] = t
    d = _dev(wide, device)
    return d, d.data_ptr() + 4 * p, ((c + 2) * p, p, 1)


BLEND_LAYOUTS = (('nchw', 'nhwc', 'slice'), ('nhwc', 'slice', 'nhwc'))      # of a, b and the upstream gradient g


def check_blend_bwd(device, n=2, p=37, seed=122):
    """fsv_blend_bwd: da, db, dm of out = a * m + b * (1 - m) (m broadcast over the channels) for an upstream gradient g, against
    float64 autograd of that expression; C = 1 and C = 5, P = 37, a / b / g each in another memory layout (dense NCHW, dense
    NHWC, a channel slice of a wider NCHW tensor), with all three outputs and with dm alone (da / db are nullable).  da = g * m is
    one fp32 product: bit-equal to the rounded exact product; db and dm: `bounded` against fp32 autograd.  Returns the number of
    launches."""
    L = lib()
    ll = lambda v: (ctypes.c_longlong * 3)(*v)                                  # noqa: E731
    ran = 0
    for c in (1, 5):
        for la, lb, lg in BLEND_LAYOUTS:
            g_ = torch.Generator().manual_seed(seed + c)
            a, b, g = (torch.randn(n, c, p, generator=g_) for _ in range(3))
            m = torch.rand(n, 1, p, generator=g_)
            grads = {}
            for dt in (torch.float64, torch.float32):
                ar, br, mr = (t.to(dt).requires_grad_(True) for t in (a, b, m))
                (ar * mr + br * (1 - mr)).backward(g.to(dt))
                grads[dt] = (ar.grad, br.grad, mr.grad)
            (ka, pa, sa), (kb, pb, sb), (kg, pg, sg) = _ncp(a, la, device), _ncp(b, lb, device), _ncp(g, lg, device)
            md = _dev(m.reshape(n, p).contiguous(), device)
            tag = 'blend_bwd C=%d a %s b %s g %s ' % (c, la, lb, lg)
            for only_dm in (False, True):
                da, db = (None, None) if only_dm else (torch.full((n, c, p), float('nan'), device=device) for _ in range(2))
                dm = torch.full((n, 1, p), float('nan'), device=device)
                L.check_device(ka, kb, kg, md, dm)
                L.call('fsv_blend_bwd', ctypes.c_void_p(pa), ctypes.c_void_p(pb), L.ptr(md), ctypes.c_void_p(pg), L.ptr(da), L.ptr(db),
                       L.ptr(dm), n, c, p, ll(sa), ll(sb), ll(sg), L.stream_ptr())
                ran += 1
                if not only_dm:
                    same_bits(tag + 'da', da, (g.double() * m.double()).float())
                    bounded(tag + 'db', db, grads[torch.float64][1], grads[torch.float32][1])
                bounded(tag + ('dm alone' if only_dm else 'dm'), dm, grads[torch.float64][2], grads[torch.float32][2])
    return ran
