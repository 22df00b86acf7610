"""Shared checks of --norm_G spectralspadeinstance / --norm_F spectralinstance / spectralnone: the SPADE kernels with per-sample
statistics (stat_bstride = C) against a float64 evaluation of normalization.py:37-52, the grouped statistics epilogue of
csrc/spade_conv3.hip, one D + G iteration / three inference frames of the product against fixtures minted from the unmodified
reference (`python tests/test_norm_instance_emu.py`), the state_dict layout, and the options.  Used by
tests/test_norm_instance_emu.py (emulator) and tests/test_norm_instance_gpu.py (hardware)."""
import contextlib
import json
import os
from importlib import import_module

import torch
import torch.nn.functional as F

import adaptive_conv_checks as ac
import model_checks as mc
import op_checks as oc

GOLD = ac.GOLD
# fixture -> (oracle.make_golden.CONFIGS key, flags appended)
STEP_FLAGS = {
    'face_inorm': ('face', ' --norm_G spectralspadeinstance'),
    'pose_combine_inorm': ('pose_combine', ' --norm_G spectralspadeinstance --norm_F spectralinstance'),
    'pose_blend_inormF': ('pose_blend', ' --norm_F spectralinstance'),
    # (the unmodified reference cannot build `pose_combine --norm_F spectralnone`: generalNorm('spectralnone') of the flow network's
    # residual blocks derives a class from None, architecture.py:42-50 - TypeError at construction.  Without those blocks it runs.)
    'pose_combine_noneF_nb0': ('pose_combine', ' --norm_F spectralnone --n_blocks_F 0'),
    'face_inorm_k3': ('face', ' --norm_G spectralspadeinstance --spade_ks 3 --embed_ks 3'),
    'face_nshot2_inorm': ('face_nshot2', ' --norm_G spectralspadeinstance'),
}
STEP_CASES = list(STEP_FLAGS)
INFERENCE_CASE = 'pose_combine_inorm'
LAYOUT_FLAGS = {'face_inorm': STEP_FLAGS['face_inorm'], 'pose_combine_inorm': STEP_FLAGS['pose_combine_inorm'],
                'pose_combine_noneF_nb0': STEP_FLAGS['pose_combine_noneF_nb0']}
LAYOUT_FILE = os.path.join(GOLD, 'ref_state_layout_norm.json')
KW = dict(norm_G='spectralspadeinstance', norm_F='spectralinstance', fineSize=32, loadSize=32, n_downsample_G=3, n_adaptive_layers=2)


def _ops():
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.ops')


def _conv():
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.conv')


def _lib():
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.lib')


_ac_opt_from_flags = ac.opt_from_flags


def opt_from_flags(flags):
    """adaptive_conv_checks.opt_from_flags plus the options of this feature and of the 3x3 SPADE (it rejects flags it does not know)"""
    toks, extra, rest, i = flags.split(), {}, [], 0
    while i < len(toks):
        if toks[i] in ('--norm_G', '--norm_F'):
            extra[toks[i][2:]] = toks[i + 1]; i += 2
        elif toks[i] in ('--spade_ks', '--embed_ks', '--n_blocks_F'):
            extra[toks[i][2:]] = int(toks[i + 1]); i += 2
        else:
            rest.append(toks[i]); i += 1
    opt = _ac_opt_from_flags(' '.join(rest))
    for k, v in extra.items():
        setattr(opt, k, v)
    return opt


@contextlib.contextmanager
def _norm_flags():
    """adaptive_conv_checks.check_step reads its fixture's flags with a parser that stops at --norm_G: lend it the one above"""
    saved = ac.opt_from_flags
    ac.opt_from_flags = opt_from_flags
    try:
        yield
    finally:
        ac.opt_from_flags = saved


# ------------------------------------------------------------------------------------------------ reference fixtures
def check_step(device, case):
    """adaptive_conv_checks.check_step (losses and outputs 1e-3, gradient norms 1e-2, sketches as there) on a --norm_* fixture"""
    with _norm_flags():
        ac.check_step(device, case)


def check_inference(device):
    """test.py path (bars of test_golden._check_product_inference) on the instance-normalised fixture: eval() networks, no running
    buffers to load but the spectral-norm vectors"""
    from test_golden import _rel
    g = torch.load(os.path.join(GOLD, 'inference_%s.pt' % INFERENCE_CASE), weights_only=False)
    opt = opt_from_flags(g['flags'])
    M = mc._model()
    model = M.create_model(opt)
    model.netG.init_temporal_network()
    mc.fill_state(model.netG)
    sd = model.netG.state_dict()
    assert not any(k.endswith(('running_mean', 'running_var')) for k in g['buffers']), 'an instance-normalised generator has no running buffers'
    for k, v in g['buffers'].items():
        sd[k].copy_(v)
    frames = [mc.synth_pose_inputs(g['batch'], g['size'], g['size'], g['seed'] + t, 6) for t in range(3)]
    model = model.to(device).eval()
    opt.isTrain = False
    ref_label, ref_image = frames[0][2].to(device), frames[0][3].to(device)
    for t, (f, ref) in enumerate(zip(frames, g['fakes'])):
        fake = model([f[0].to(device), None, None, None, ref_label, ref_image, None, None, None])[0]
        r = _rel(fake.cpu(), ref)
        print('inference', INFERENCE_CASE, 'frame', t, '%.2e' % r)
        assert r <= 1e-3, (t, r)
    assert model.t == 2


def check_layout():
    """state_dict keys and shapes of the product's generator == the reference's, key for key, under the three flag sets"""
    with open(LAYOUT_FILE) as f:
        layout = json.load(f)
    assert set(layout) == set(LAYOUT_FLAGS)
    for name, rec in layout.items():
        opt = opt_from_flags(rec['flags'])
        with torch.device('meta'):
            net = mc._net().define_G(opt)
        mine = {k: list(v.shape) for k, v in net.state_dict().items()}
        ref = rec['netG']
        assert sorted(set(ref) - set(mine)) == [] and sorted(set(mine) - set(ref)) == [], \
            (name, sorted(set(ref) - set(mine))[:8], sorted(set(mine) - set(ref))[:8])
        for k, shp in ref.items():
            assert mine[k] == shp, (name, k, mine[k], shp)
        if 'inorm' in name:
            assert not any('running_' in k or 'num_batches_tracked' in k or '.bn.' in k for k in mine
                           if not k.startswith(('flow_network', 'img_ref_embedding')) or 'norm_F' in rec['flags']), name


# ------------------------------------------------------------------------------------------------ the kernels, per-sample statistics
OFFSETS = (0.0, 3.0, -5.0)
SCALES = (1.0, 0.1, 10.0)
EPS = 0.1


def _inputs(n, c, h, w, up, chs, per_sample, k, seed):
    """x with per-sample offsets (0, +3, -5) and scales (1, 0.1, 10): any other sample's statistics miss by orders of magnitude"""
    assert n == len(OFFSETS)
    g = torch.Generator().manual_seed(seed)
    xs = (h // 2, w // 2) if up else (h, w)
    x = torch.randn(n, c, *xs, generator=g)
    x = x * torch.tensor(SCALES).view(n, 1, 1, 1) + torch.tensor(OFFSETS).view(n, 1, 1, 1)
    maps = [torch.randn(n, ch, h, w, generator=g) for ch in chs]
    wts = []
    for i, ch in enumerate(chs):
        lead = (n,) if (per_sample and i == 0) else ()
        wts.append((torch.randn(*lead, c, ch, k, k, generator=g) * (0.3 / k), torch.randn(*lead, c, ch, k, k, generator=g) * (0.3 / k),
                    torch.randn(*lead, c, generator=g) * 0.3, torch.randn(*lead, c, generator=g) * 0.3))
    dy = torch.randn(n, c, h, w, generator=g)
    return x, maps, wts, dy


def _conv_any(m, w, b):
    """conv2d with shared [C, Ch, k, k] or per-sample [N, C, Ch, k, k] weights (batch_conv, base_network.py:56-71), padding k // 2"""
    pad = w.shape[-1] // 2
    if w.dim() == 4:
        return F.conv2d(m, w, b, padding=pad)
    return torch.cat([F.conv2d(m[i:i + 1], w[i], b[i], padding=pad) for i in range(m.shape[0])], 0)


def spade_instance_ref(x, maps, wts, act, up, dtype=torch.float64):
    """normalization.py:37-52 with self.norm = nn.InstanceNorm2d(C, affine=False, eps=0.1), restated in torch at `dtype`: returns
    (h, leaves) with leaves = [x, maps.., (wg, wb, bg, bb)..] requiring gradients"""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    xr, mr = leaf(x), [leaf(m) for m in maps]
    wr = [tuple(leaf(t) for t in ws) for ws in wts]
    xin = F.interpolate(xr, scale_factor=2, mode='nearest') if up else xr
    out = F.instance_norm(xin, eps=EPS)
    for m, (wg, wb, bg, bb) in zip(mr, wr):
        out = out * (1 + _conv_any(m, wg, bg)) + _conv_any(m, wb, bb)
    if act:
        out = F.leaky_relu(out, 0.2)
    return out, [xr] + mr + [t for ws in wr for t in ws]


def _close_per_sample(name, got, ref, tol):
    """op_checks.assert_close, sample by sample where the tensor has a batch axis of the test's N (the x gradients of the three samples
    differ by the ratio of their scales: one bar over the whole tensor would be 30 x looser for the smallest)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    if got.dim() >= 2 and got.shape[0] == len(OFFSETS):
        for i in range(got.shape[0]):
            oc.assert_close('%s [sample %d]' % (name, i), got[i], ref[i], tol=tol)
    else:
        oc.assert_close(name, got, ref, tol=tol)


@contextlib.contextmanager
def _env(**kw):
    saved = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _recorded():
    lib = _lib()
    seen, real = [], lib.call

    def rec(name, *a):
        seen.append((name, a))
        return real(name, *a)
    lib.call = rec
    try:
        yield seen
    finally:
        lib.call = real


def check_spade_instance(device, c=16, chs=(4,), per_sample=True, h=9, w=7, up=False, act=True, k=1, bwd='twin', max_gx=None, seed=31):
    """ops.spade_mod(instance=True) on `device` against the float64 reference: output and the gradients of x, of every map and of every
    weight / bias, at the bar of tests/test_ops_gpu.py::test_spade (op_checks.REL_TOL, here per sample).  bwd: 'twin' (the fused
    backward twin fsv_spade_mod_bwd; c % 16 == 0) or 'elem' (gamma | beta materialised + fsv_spade_bwd_elem)"""
    ops, conv = _ops(), _conv()
    n = len(OFFSETS)
    x, maps, wts, dy = _inputs(n, c, h, w, up, chs, per_sample, k, seed)
    ref, leaves_r = spade_instance_ref(x, maps, wts, act, up)
    ref.backward(dy.double())
    dev = lambda t: t.to(device).detach().clone().requires_grad_(True)
    xd, md = dev(x), [dev(m) for m in maps]
    wd = [tuple(dev(t) for t in ws) for ws in wts]
    with _env(FSV_SPADE_FUSED_BWD='1' if bwd == 'twin' else '0', FSV_SPADE_MAX_GX=max_gx), _recorded() as seen:
        y = ops.spade_mod(xd, md, wd, None, None, act=conv.ACT_LRELU if act else conv.ACT_NONE, eps=EPS, up=up, instance=True)
        y.backward(dy.to(device))
    names = [nm for nm, _ in seen]
    fast = c % 16 == 0 and k == 1
    if k == 3:
        assert 'fsv_spade_k3_fwd' in names and 'fsv_spade_bwd_elem' in names, names
    else:
        assert 'fsv_spade_mod_fwd' in names, names
        assert ('fsv_spade_mod_bwd' in names) == (fast and bwd == 'twin') and ('fsv_spade_bwd_elem' in names) != (fast and bwd == 'twin'), names
    # every launch that takes the statistics indexes them per sample, and the statistics are N groups of H W pixels
    for nm, a in seen:
        if nm == 'fsv_norm_stats_fused':
            assert a[4:7] == (n, (h // 2) * (w // 2) if up else h * w, c), a[4:7]
    _close_per_sample('spade(instance) h', y, ref, oc.REL_TOL)
    leaves_d = [xd] + md + [t for ws in wd for t in ws]
    for i, (a, b) in enumerate(zip(leaves_r, leaves_d)):
        _close_per_sample('spade(instance) grad %d' % i, b.grad, a.grad, oc.REL_TOL)


def check_spade_instance_eval_and_buffers(device):
    """instance=True ignores `training` and running buffers: same bits either way, buffers untouched"""
    ops, conv = _ops(), _conv()
    x, maps, wts, _ = _inputs(3, 16, 9, 7, False, (4,), True, 1, 33)
    d = lambda t: t.to(device)
    rm, rv = d(torch.full((16,), 7.0)), d(torch.full((16,), 9.0))
    a = ops.spade_mod(d(x), [d(m) for m in maps], [tuple(d(t) for t in ws) for ws in wts], None, None, eps=EPS, instance=True)
    b = ops.spade_mod(d(x), [d(m) for m in maps], [tuple(d(t) for t in ws) for ws in wts], rm, rv, training=False, eps=EPS, instance=True)
    assert torch.equal(a, b) and float(rm.min()) == 7.0 and float(rv.max()) == 9.0


def _block_inputs(c, cout, chs, h, w, up, kconv, seed):
    n = len(OFFSETS)
    x, maps, wts, _ = _inputs(n, c, h, w, up, chs, True, 1, seed)
    g = torch.Generator().manual_seed(seed + 1)
    wconv = torch.randn(cout, c, kconv, kconv, generator=g) * (1.0 / (kconv * kconv * c) ** 0.5)
    bconv = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(n, cout, h, w, generator=g)
    return x, maps, wts, wconv, bconv, dy


def _run_fused(device, x, maps, wts, wconv, bconv, dy, act, up, conv3, fused, stats):
    ops, conv = _ops(), _conv()
    cl = lambda t: t.to(device).detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    pl = lambda t: t.to(device).detach().clone().requires_grad_(True)
    xd, md = cl(x), [cl(m) for m in maps]
    wd = [tuple(pl(t) for t in ws) for ws in wts]
    wc, bc = pl(wconv), (pl(bconv) if conv3 else None)
    env = dict(FSV_SPADE_CONV3='1' if (conv3 and fused) else '0', FSV_SPADE_CONV_S='1' if (fused and not conv3) else '0')
    with _env(**env), _recorded() as seen:
        with ops.spade_into_conv(conv3=conv3):
            hm = ops.spade_mod(xd, md, wd, None, None, act=conv.ACT_LRELU if act else conv.ACT_NONE, eps=EPS, up=up, instance=True)
            y = ops.conv2d(hm, wc, bc, 1, 1 if conv3 else 0, stats_groups=stats)
        (y * dy.to(device)).sum().backward()
    grads = [xd.grad] + [m.grad for m in md] + [t.grad for ws in wd for t in ws] + [wc.grad] + ([bc.grad] if conv3 else [])
    return y, grads, seen


def _fused_ref(x, maps, wts, wconv, bconv, dy, act, up, conv3):
    h, leaves = spade_instance_ref(x, maps, wts, act, up)
    wc = wconv.double().clone().requires_grad_(True)
    bc = bconv.double().clone().requires_grad_(True) if conv3 else None
    y = F.conv2d(h, wc, bc, padding=1 if conv3 else 0)
    (y * dy.double()).sum().backward()
    return y, [l.grad for l in leaves] + [wc.grad] + ([bc.grad] if conv3 else [])


def check_spade_conv_s_instance(device, c=64, cout=32, chs=(8, 4), h=9, w=7, up=False, seed=41):
    """bn_s -> conv_s as one kernel (csrc/spade_conv.hip) with per-sample statistics against float64, at the bars
    op_checks._check_spade_conv_s holds the batch-statistics form to against the oracle (2e-5 output, 4e-5 gradients on the exact-fp32
    kernels), and against the two launches (2e-5)"""
    data = _block_inputs(c, cout, chs, h, w, up, 1, seed)
    y_ref, g_ref = _fused_ref(*data, act=False, up=up, conv3=False)
    y1, g1, seen1 = _run_fused(device, *data, act=False, up=up, conv3=False, fused=False, stats=0)
    y2, g2, seen2 = _run_fused(device, *data, act=False, up=up, conv3=False, fused=True, stats=0)
    n1, n2 = [s[0] for s in seen1], [s[0] for s in seen2]
    assert 'fsv_spade_conv_s_fwd' in n2 and 'fsv_spade_mod_fwd' not in n2 and 'fsv_spade_conv_s_fwd' not in n1, (n1, n2)
    _close_per_sample('bn_s -> conv_s (instance) vs two launches', y2, y1, 2e-5)
    _close_per_sample('bn_s -> conv_s (instance) vs float64', y2, y_ref, 2e-5)
    for i, (a, b, r) in enumerate(zip(g1, g2, g_ref)):
        _close_per_sample('bn_s -> conv_s (instance) grad %d vs two launches' % i, b, a, 2e-5)
        _close_per_sample('bn_s -> conv_s (instance) grad %d vs float64' % i, b, r, 4e-5)


def check_spade_conv3_instance(device, c=64, cout=32, chs=(8, 4), h=12, w=10, up=False, seed=43):
    """actvn(bn) -> conv3x3 as one kernel (csrc/spade_conv3.hip) with per-sample statistics against float64 at the bars of
    op_checks.check_spade_conv3 (2e-5 output, 4e-5 gradients), and its statistics epilogue with one group per sample against a float64
    reduction of its own output (1e-5 of the largest sum, as check_spade_conv3 holds the one-group form)"""
    conv = _conv()
    n = len(OFFSETS)
    data = _block_inputs(c, cout, chs, h, w, up, 3, seed)
    y_ref, g_ref = _fused_ref(*data, act=True, up=up, conv3=True)
    y2, g2, seen2 = _run_fused(device, *data, act=True, up=up, conv3=True, fused=True, stats=-1)
    n2 = [s[0] for s in seen2]
    assert 'fsv_spade_conv3_fwd' in n2 and 'fsv_spade_mod_fwd' not in n2, n2
    _close_per_sample('bn -> actvn -> conv3x3 (instance) vs float64', y2, y_ref, 2e-5)
    for i, (b, r) in enumerate(zip(g2, g_ref)):
        _close_per_sample('bn -> actvn -> conv3x3 (instance) grad %d vs float64' % i, b, r, 4e-5)
    if conv.stats_enabled():
        ys = getattr(y2, '_fsv_stats', None)
        assert ys is not None, 'the fused launch leaves the per-sample statistics of its output'
        part, groups, slots, px, ch_ = ys
        assert (groups, px, ch_) == (n, h * w, cout), (groups, px, ch_)
        got = part.view(n, slots, cout, 2).sum(1).cpu()
        yd = y2.detach().double().cpu()
        want = torch.stack([yd.sum(dim=(2, 3)), (yd * yd).sum(dim=(2, 3))], dim=2)
        for i in range(n):
            assert float((got[i] - want[i]).abs().max()) <= 1e-5 * float(want[i].abs().max()), (i, got[i], want[i])
        # ... and the normalisation that follows takes them: no reduction launch of its own
        ops = _ops()
        with _recorded() as seen, torch.no_grad():
            z = ops.norm_act(y2, None, None, None, None, instance=True, eps=EPS)
        names = [s[0] for s in seen]
        assert 'fsv_norm_stats_finish' in names and 'fsv_norm_stats_fused' not in names, names
        oc.assert_close('instance norm from the grouped epilogue', z, F.instance_norm(yd, eps=EPS), tol=2e-5)


# ------------------------------------------------------------------------------------------------ behaviour
def check_unknown_norms():
    import pytest
    net = mc._net()
    for bad in ('spectralinstance', 'spectralspadegroup', 'spadeinstance', ''):
        with torch.device('meta'):
            with pytest.raises(NotImplementedError, match=repr(bad)):
                net.define_G(mc.tiny_opt(norm_G=bad))
    for bad, word in (('spectralgroup', 'group'), ('spectrallayer', 'layer')):
        with torch.device('meta'):
            with pytest.raises(ValueError, match='normalization layer %s is not recognized' % word):
                net.define_G(mc.tiny_opt(norm_F=bad, warp_ref=True))
    with torch.device('meta'):
        for ok in ('spectralspadesyncbatch', 'spectralspadebatch', 'spectralspadeinstance'):
            net.define_G(mc.tiny_opt(norm_G=ok))
        for ok in ('spectralsyncbatch', 'spectralbatch', 'spectralinstance', 'spectralnone'):
            net.define_G(mc.tiny_opt(norm_F=ok, warp_ref=True, n_blocks_F=0))
        with pytest.raises(NotImplementedError):
            net.define_D(mc.tiny_opt(), 9, 8, 3, 'spectralbatch')


def check_amp_raises():
    import pytest
    net = mc._net()
    for amp in ('O1', 'bf16x3'):
        for kw in (dict(norm_G='spectralspadeinstance'), dict(norm_F='spectralinstance'), dict(norm_F='spectralnone'),
                   dict(norm_G='spectralspadebatch')):
            with torch.device('meta'):
                with pytest.raises(NotImplementedError, match='norm_G'):
                    net.define_G(mc.tiny_opt(amp=amp, **kw))
        with torch.device('meta'):
            net.define_G(mc.tiny_opt(amp=amp))


def check_eval_equals_train(device):
    """an instance-normalised generator has no normalisation mode: its output with every normalisation-carrying module in train()
    equals its eval() output bit for bit in the fixed-order arithmetic.  What legitimately differs between the modes, here as in the
    reference, is the spectral-norm power iteration (train() advances u / v before it forms sigma): the spectral layers and the
    generator that batches their iteration are therefore held in eval() in both passes, everything else is switched."""
    net_mod = mc._net()
    with _env(FSV_DETERMINISTIC='1'):
        opt = mc.tiny_opt(**KW, warp_ref=True, spade_combine=True)
        net = net_mod.define_G(opt)
        mc.fill_state(net)
        net = net.to(device)
        assert not any('running' in k or 'num_batches' in k for k in net.state_dict())
        tl, ti, rl, ri = [t.to(device) for t in mc.synth_pose_inputs(2, 32, 32, 77, 6)]
        net.eval()
        with torch.no_grad():
            b = net(tl[:, 0], rl, ri)
            switched = 0
            for m in net.modules():
                if m is not net and not isinstance(m, (net_mod.Conv2d, net_mod.Linear)):
                    m.training = True
                    switched += 1
            assert switched > 50 and net.up_0.bn_0.training and net.ref_img_first.training and net.flow_network_ref.training
            a = net(tl[:, 0], rl, ri)
        assert torch.equal(a[0], b[0]), float((a[0] - b[0]).abs().max())          # the image
        for k in (1, 2, 4):       # flow, mask, warp of the reference branch
            assert torch.equal(a[k][0], b[k][0]), k
        # (the batch-normalised generator does have a mode: the same switch changes its output)
        net2 = net_mod.define_G(mc.tiny_opt(**dict(KW, norm_G='spectralspadesyncbatch', norm_F='spectralsyncbatch'), warp_ref=True,
                                            spade_combine=True))
        mc.fill_state(net2)
        net2 = net2.to(device).eval()
        with torch.no_grad():
            b2 = net2(tl[:, 0], rl, ri)[0].clone()
            for m in net2.modules():
                if m is not net2 and not isinstance(m, (net_mod.Conv2d, net_mod.Linear)):
                    m.training = True
            a2 = net2(tl[:, 0], rl, ri)[0]
        assert not torch.equal(a2, b2)


def _torch_ops(device, **kw):
    """torch operators (aten overload packets, with counts) of one steady-state D + G iteration: the loop of
    tests/test_launch_count_emu.py under a dispatch mode"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Seen(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.ops = {}

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func.overloadpacket)
            self.ops[name] = self.ops.get(name, 0) + 1
            return func(*args, **(kwargs or {}))
    M = mc._model()
    opt = mc.tiny_opt(warp_ref=True, spade_combine=True, remove_face_labels=True, **kw)
    model = M.create_model(opt)
    mc.fill_state(model.netG); mc.fill_state(model.netD)
    model = model.to(device).train()
    opt_G, opt_D = model.build_optimizers()
    tl, ti, rl, ri = [t.to(device) for t in mc.synth_pose_inputs(2, 64, 64, 900, opt.input_nc)]
    data = [tl, ti, [None, None], [None, None], rl, ri, None, None, None]
    seen = None
    for it in range(2):
        seen = Seen()
        with seen:
            M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
            g, _, _ = model(data, mode='generator')
            M.loss_backward(opt, g, opt_G, 0)
    return seen.ops


def check_no_new_torch_operator(device):
    """the instance-normalised iteration issues no torch operator the default iteration does not: all of its arithmetic is in the
    library.  (Counts may differ - there are fewer parameters and buffers - the set may not grow.)"""
    base = _torch_ops(device)
    for kw in (dict(norm_G='spectralspadeinstance', norm_F='spectralinstance'), dict(norm_F='spectralnone', n_blocks_F=0)):
        ops = _torch_ops(device, **kw)
        new = sorted(set(ops) - set(base))
        print(kw, 'operators', len(ops), 'of the default', len(base), 'new', new)
        assert not new, (kw, new)
