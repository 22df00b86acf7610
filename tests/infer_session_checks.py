"""Shared checks of frozen-weight inference (few-shot-vid2vid_amd/infer.py): the `col_scale` layouts of fsv_prep_weight and the uint8
frames of fsv_cast_half dir 2 against torch / numpy bit for bit, the folded convolution -> BatchNorm -> LeakyReLU launch against
float64, and `InferenceSession` against the eager `Vid2VidModel.inference` of a twin model in the same state (same bits), the
reference fixtures (their 1e-3 bar) and the emulator's launch counters.  Used by tests/test_infer_session_emu.py (emulator) and
tests/test_infer_session_gpu.py (hardware: real captures)."""
import ctypes
import os
from importlib import import_module

import numpy as np
import torch
import torch.nn.functional as F

import model_checks as mc
import norm_instance_checks as ni

GOLD = ni.GOLD
FIXTURES = ('pose_combine', 'pose_combine_inorm', 'pose_combine_aconv_concat')
FROZEN_KERNELS = ('fsv_prep_weight', 'fsv_sn_', 'fsv_spade_prep')
# (Cout, Cin, k) of the col_scale layouts; the last one as a per-sample batch of 2
COL_SCALE_SHAPES = [(8, 6, 3, 0), (40, 12, 3, 0), (33, 4, 1, 0), (64, 32, 3, 0), (8, 8, 3, 2)]
# (Cout, stride, spectral, bias) of the folded launch: N = 2, Cin = 8, H x W = 9 x 7
FOLD_CASES = [(co, st, sp, bi) for co in (12, 40) for st in (1, 2) for sp in (True, False) for bi in (True, False)]


def _mod(name):
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.' + name)


def emu_report(reset=True):
    """{kernel name: launches since the last reset} from the emulator's counter"""
    h = _mod('lib').get_lib()
    buf = ctypes.create_string_buffer(1 << 16)
    h.fsv_emu_launch_report(buf, len(buf), 1 if reset else 0)
    return {l.rsplit(' ', 1)[0]: int(l.rsplit(' ', 1)[1]) for l in buf.value.decode().splitlines()}


def _count(rep, prefixes):
    return sum(v for k, v in rep.items() if k.lstrip('(').startswith(tuple(prefixes)))


# ------------------------------------------------------------------------------------------------ 1: col_scale layouts
def check_col_scale(device, cout, cin, k, nbatch, seed=3):
    """mode 0 with col_scale == (w * cs[:, None, None, None]) re-arranged in torch, bit for bit; padding exactly zero"""
    conv = _mod('conv')
    g = torch.Generator().manual_seed(seed + cout)
    shape = ((nbatch,) if nbatch else ()) + (cout, cin, k, k)
    w = torch.randn(shape, generator=g)
    cs = torch.randn(cout, generator=g) * 3
    geom = conv.Geom(k, k, 1, k // 2)
    kpad, ldw = (len(geom.khs) * cin + 31) // 32 * 32, (cout + 31) // 32 * 32
    out = torch.full((max(nbatch, 1), kpad, ldw), 7.0, device=device)       # the kernel has to write the padding itself
    wt, kp, ld = conv.prep_weight(w.to(device), 0, geom, col_scale=cs.to(device), out=out)
    assert (kp, ld) == (kpad, ldw) and wt is out
    ws = (w * cs[:, None, None, None]).reshape((max(nbatch, 1), cout, cin, k, k))
    want = torch.zeros(max(nbatch, 1), kpad, ldw)
    rows = torch.stack([ws[:, :, :, a, b] for a, b in zip(geom.khs, geom.kws)], dim=1)          # [z, tap, co, ci]
    want[:, :len(geom.khs) * cin, :cout] = rows.permute(0, 1, 3, 2).reshape(max(nbatch, 1), -1, cout)
    got = wt.cpu()
    assert torch.equal(got, want), float((got - want).abs().max())
    assert float(got[:, len(geom.khs) * cin:].abs().max() if kpad > len(geom.khs) * cin else 0.0) == 0.0
    assert float(got[:, :, cout:].abs().max() if ldw > cout else 0.0) == 0.0


def check_col_scale_bad_args(device, launches=None):
    """col_scale with scale_ptr, or with a mode other than 0: FSV_ERR_BAD_ARG and no launch"""
    lib, conv = _mod('lib'), _mod('conv')
    bad = lib.ENUMS['FSV_ERR_BAD_ARG']
    w = torch.randn(8, 8, 3, 3).to(device)
    cs, sc = torch.ones(8, device=device), torch.ones(1, device=device)
    geom = conv.Geom(3, 3, 1, 1)
    out = torch.zeros(1, 96, 32, device=device)

    def call(scale, mode):
        return lib.call_status("fsv_prep_weight", lib.ptr(w), lib.ptr(out), lib.ptr(scale), mode, 1, 8, 8, 3, 3, 9,
                               lib.int_array(geom.khs), lib.int_array(geom.kws), 96, 32, 8 * 8 * 9, 96 * 32, lib.ptr(cs),
                               lib.stream_ptr())
    n0 = launches() if launches else 0
    assert call(sc, 0) == bad
    for mode in (1, 2, 3):
        assert call(None, mode) == bad, mode
    if launches:
        assert launches() == n0
    assert float(out.abs().max()) == 0.0
    assert call(None, 0) == 0 and float(out.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 2: uint8 frames
def tensor2im_np(x):
    """util/util.py:63,66,70 of the reference (normalised form) on a float32 array, as numpy evaluates it"""
    assert x.dtype == np.float32
    return np.clip((x + 1) / 2.0 * 255.0, 0, 255).astype(np.uint8)


def _u8_values(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) * 3.2 - 1.6).numpy()
    special = np.array([-1.0, 1.0, -1.5, 1.2, 0.0, -0.0], dtype=np.float32)
    # values whose scaled result sits next to an integer boundary: the fp32 neighbours of 2 k / 255 - 1
    ks = np.arange(0, 257, dtype=np.float64)
    edge = (2.0 * ks / 255.0 - 1.0).astype(np.float32)
    edge = np.concatenate([edge, np.nextafter(edge, np.float32(-4)), np.nextafter(edge, np.float32(4))])
    fill = np.concatenate([special, edge])
    m = min(n, fill.shape[0])
    x[:m] = fill[:m]
    return x.astype(np.float32)


def check_image_u8(device):
    ops = _mod('ops')
    for n in (1, 7, 4099):
        x = _u8_values(n, 70 + n)
        assert not np.isnan(x).any()
        got = ops.image_u8(torch.from_numpy(x).to(device))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n,)
        want = tensor2im_np(x)
        assert np.array_equal(got.cpu().numpy(), want), (n, int(np.abs(got.cpu().numpy().astype(int) - want.astype(int)).max()))
    # a channels-last [2, 3, 5, 7] image comes back as [2, 5, 7, 3]
    x = torch.from_numpy(_u8_values(2 * 3 * 5 * 7, 99)).view(2, 3, 5, 7)
    img = x.to(device).contiguous(memory_format=torch.channels_last)
    got = ops.image_u8(img)
    assert tuple(got.shape) == (2, 5, 7, 3)
    assert np.array_equal(got.cpu().numpy(), tensor2im_np(x.permute(0, 2, 3, 1).contiguous().numpy()))


# ------------------------------------------------------------------------------------------------ 3: the folded launch
def _fold_layers(device, cout, stride, spectral, bias, seed):
    net = mc._net()
    g = torch.Generator().manual_seed(seed)
    cv = net.Conv2d(8, cout, 3, stride=stride, padding=1, bias=bias, spectral=spectral)
    bn = net.BatchNorm(cout)
    with torch.no_grad():
        (cv.weight_orig if spectral else cv.weight).copy_(torch.randn(cout, 8, 3, 3, generator=g) * 0.2)
        if bias:
            cv.bias.copy_(torch.randn(cout, generator=g) * 0.3)
        if spectral:
            # (u / v as training leaves them - a few power iterations: sigma = u . (W v) of random vectors is a random small
            # number that only measures how badly the division is conditioned)
            w2, u = cv.weight_orig.detach().reshape(cout, -1), F.normalize(torch.randn(cout, generator=g), dim=0)
            for _ in range(20):
                v = F.normalize(w2.t() @ u, dim=0)
                u = F.normalize(w2 @ v, dim=0)
            cv.weight_u.copy_(u); cv.weight_v.copy_(v)
        bn.weight.copy_(1.0 + 0.3 * torch.randn(cout, generator=g))
        bn.bias.copy_(0.2 * torch.randn(cout, generator=g))
        bn.running_mean.copy_(0.5 * torch.randn(cout, generator=g))            # running statistics that are not the defaults
        bn.running_var.copy_(0.3 + torch.rand(cout, generator=g) * 2)
    x = torch.randn(2, 8, 9, 7, generator=g)
    return cv.to(device).eval(), bn.to(device).eval(), x


def _fold_ref64(cv, bn, x):
    w = (cv.weight_orig if cv.spectral else cv.weight).detach().double().cpu()
    if cv.spectral:
        u, v = cv.weight_u.double().cpu(), cv.weight_v.double().cpu()
        w = w / torch.dot(u, w.reshape(w.shape[0], -1) @ v)                  # eval-mode sigma = u . (W v)
    y = F.conv2d(x.double(), w, cv.bias.detach().double().cpu() if cv.bias is not None else None, stride=cv.stride, padding=1)
    y = F.batch_norm(y, bn.running_mean.double().cpu(), bn.running_var.double().cpu(), bn.weight.detach().double().cpu(),
                     bn.bias.detach().double().cpu(), False, 0.0, 1e-5)
    return F.leaky_relu(y, 0.2)


def check_fold_launch(device, cout, stride, spectral, bias, report=None):
    """ONE folded launch against float64 conv -> eval-BN -> LeakyReLU: at most 4 x the max-abs error of the existing two-launch
    path against the same float64 values (the fold re-associates one multiply per weight and one add per output: an error of the
    same order, the factor absorbs the different rounding points).  Returns (error of the fold, error of the two launches)."""
    infer, ops, conv = _mod('infer'), _mod('ops'), _mod('conv')
    cv, bn, x = _fold_layers(device, cout, stride, spectral, bias, 11 + cout + 2 * stride)
    ref = _fold_ref64(cv, bn, x)
    xd = x.to(device).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        two = bn(cv(xd), act=conv.ACT_LRELU)
        fz = infer.FrozenWeights()
        w = cv.weight_orig if spectral else cv.weight
        w._fsv_frozen = fz
        if spectral:
            cv._sig_frozen = ops.SpectralState.update(cv.weight_orig, cv.weight_u, cv.weight_v, False)
        infer.fold_conv_bn(fz, cv, bn)
        if report:
            report()
        one = bn(cv(xd), act=conv.ACT_LRELU)
        if report:
            rep = report()
            assert _count(rep, ['fsv_norm_apply']) == 0 and _count(rep, ['fsv_sn_']) == 0, rep
            assert _count(rep, ['fsv_prep_weight']) == 1, rep        # the re-arrangement, once
            again = bn(cv(xd), act=conv.ACT_LRELU)
            rep = report()
            assert _count(rep, ['fsv_prep_weight', 'fsv_norm_apply', 'fsv_sn_']) == 0 and torch.equal(again, one), rep
    assert one.shape == two.shape == ref.shape
    e_one = float((one.double().cpu() - ref).abs().max())
    e_two = float((two.double().cpu() - ref).abs().max())
    print('fold Cout %d stride %d spectral %d bias %d: folded %.3e two launches %.3e ratio %.2f'
          % (cout, stride, spectral, bias, e_one, e_two, e_one / e_two))
    assert e_two > 0 and e_one <= 4.0 * e_two, (e_one, e_two)
    return e_one, e_two


# ------------------------------------------------------------------------------------------------ session scenarios
def settle_buffers(net, seed):
    """eval-mode BatchNorm statistics that are not the defaults (fill_state writes zeros and ones), and spectral-norm vectors that a
    training run would have left: thirty power iterations from the key-derived ones (eval() forms sigma = u . (W v) from the
    buffers as they are; with random u / v it is a random small number and a deep generator overflows)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in mc._net().spectral_layers(net):
            w = m.weight_orig.detach().reshape(m.weight_orig.shape[0], -1).double()
            u, v = m.weight_u.double(), m.weight_v.double()
            for _ in range(30):
                v = F.normalize(w.t() @ u, dim=0, eps=1e-12)
                u = F.normalize(w @ v, dim=0, eps=1e-12)
            m.weight_u.copy_(u.float()); m.weight_v.copy_(v.float())
        for k, v in net.state_dict().items():
            if k.endswith('running_mean'):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith('running_var'):
                v.copy_(0.6 + torch.rand(v.shape, generator=g))


def fixture_setup(case, device, finetune=False):
    """(opt, model in eval() on `device`, fixture): the product model in the fixture's state, as the golden tests build it"""
    M = mc._model()
    if finetune:
        from test_golden import _finetune_setup
        g = torch.load(os.path.join(GOLD, 'finetune_%s.pt' % case), weights_only=False)
        opt, model, _ = _finetune_setup(g)
    else:
        g = torch.load(os.path.join(GOLD, 'inference_%s.pt' % case), weights_only=False)
        opt = ni.opt_from_flags(g['flags'])
        model = M.create_model(opt)
        model.netG.init_temporal_network()
        mc.fill_state(model.netG)
        sd = model.netG.state_dict()
        for k, v in g['buffers'].items():
            sd[k].copy_(v)
    model = model.to(device).eval()
    opt.isTrain = False
    model.isTrain = False
    return opt, model, g


def fixture_sequence(g, opt, n, device, ref_seed=None):
    """n frames of the fixture's seeded inputs: ([encoded target labels], encoded reference labels, reference images)"""
    M = mc._model()
    frames = [mc.synth_pose_inputs(g['batch'], g['size'], g['size'], g['seed'] + t, 6) for t in range(n)]
    ref = frames[0] if ref_seed is None else mc.synth_pose_inputs(g['batch'], g['size'], g['size'], ref_seed, 6)
    return ([M.encode_label(opt, f[0].to(device)) for f in frames], M.encode_label(opt, ref[2].to(device)), ref[3].to(device))


def tiny_setup(device, seed=77, temporal=True, scale=1.0, **kw):
    """scale: of the key-derived generator weights (eval-mode BatchNorm does not re-normalise: a deep stack of them must not overflow)"""
    M = mc._model()
    opt = mc.tiny_opt(**kw)
    opt.isTrain = False
    model = M.create_model(opt)
    if temporal:
        model.netG.init_temporal_network()
    mc.fill_state(model.netG, scale); mc.fill_state(model.netD)
    settle_buffers(model.netG, seed)
    model = model.to(device).eval()
    model.isTrain = False
    return opt, model


def tiny_sequence(opt, n, device, seed, b=1):
    M = mc._model()
    h, w = int(opt.fineSize / opt.aspect_ratio), opt.fineSize
    nl = opt.label_nc if opt.label_nc != 0 else opt.input_nc
    frames = [mc.synth_pose_inputs(b, h, w, seed + t, nl) for t in range(n)]
    _, _, rl, ri = mc.with_n_shot(frames[0], opt.n_shot, b, h, w, seed, nl)
    return ([M.encode_label(opt, f[0].to(device)) for f in frames], M.encode_label(opt, rl.to(device)), ri.to(device))


def _keep(out):
    """a frame's outputs, detached from the static buffers a replay writes them into"""
    def cp(o):
        if torch.is_tensor(o):
            return o.detach().clone()
        if isinstance(o, (list, tuple)):
            return [cp(x) for x in o]
        return o
    kept = [cp(o) for o in out]
    u8 = getattr(out, 'image_u8', None)
    return kept, (u8.clone() if u8 is not None else None)


def _flat(o, out=None):
    out = [] if out is None else out
    if isinstance(o, (list, tuple)):
        for x in o:
            _flat(x, out)
    else:
        out.append(o)
    return out


def same_bits(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb), (len(fa), len(fb))
    bad = []
    for i, (x, y) in enumerate(zip(fa, fb)):
        if x is None or y is None:
            if not (x is None and y is None):
                bad.append(i)
        elif x.shape != y.shape or not torch.equal(x, y):
            bad.append(i)
    return bad


def run_eager(model, seq, report=None):
    labels, rl, ri = seq
    model.reset_inference()
    outs, reps = [], []
    for lab in labels:
        if report:
            report()
        outs.append(_keep(model.inference(lab, rl, ri))[0])
        reps.append(report() if report else None)
    return outs, reps


def run_session(sess, seq, report=None):
    labels, rl, ri = seq
    sess.reset()
    outs, u8s, reps = [], [], []
    for lab in labels:
        if report:
            report()
        kept, u8 = _keep(sess(lab, rl, ri))
        reps.append(report() if report else None)
        outs.append(kept)
        u8s.append(u8)
    return outs, u8s, reps


def assert_same_frames(eager, got, what):
    assert len(eager) == len(got)
    for t, (a, b) in enumerate(zip(eager, got)):
        assert len(a) == len(b) == 6
        bad = same_bits(a, b)
        assert not bad, '%s: frame %d, outputs %s differ from the eager path' % (what, t, bad)


def assert_captured(sess, device, captures=1):
    if device.type == 'cuda':
        assert sess.capture_failures == [], sess.capture_failures
        assert sess.n_captures == captures and sess.launch_mode() == 'hipgraph', (sess.n_captures, sess.launch_mode())


def _rel(a, b):
    from test_golden import _rel as rel
    return rel(a, b)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------------------------------------ 4, 5, 6: fixtures
_scenarios = {}


def fixture_scenario(case, device, report=None, second=False):
    """ONE run shared by the tests of a fixture (fold_norms=False, frames_u8=True): four frames eager on a twin and four through a
    session; with second=True also - same session, same graph - a second sequence of two frames on other references after reset()"""
    key = (case, str(device))
    r = _scenarios.get(key)
    if r is None:
        infer = _mod('infer')
        opt, twin, g = fixture_setup(case, device)
        _, model, _ = fixture_setup(case, device)
        seq1 = fixture_sequence(g, opt, 4, device)
        sess = infer.InferenceSession(model, opt, fold_norms=False, frames_u8=True, warmup=1)
        e1, er1 = run_eager(twin, seq1, report)
        s1, u1, sr1 = run_session(sess, seq1, report)
        r = _scenarios[key] = dict(opt=opt, g=g, sess=sess, model=model, twin=twin, seq1=seq1, e1=e1, s1=s1, u1=u1, er1=er1, sr1=sr1,
                                   caps=sess.n_captures)
    if second and 'e2' not in r:
        seq2 = fixture_sequence(r['g'], r['opt'], 2, device, ref_seed=r['g']['seed'] + 40)
        seq2 = (r['seq1'][0][2:], seq2[1], seq2[2])
        r['e2'], _ = run_eager(r['twin'], seq2, report)
        r['s2'], _, _ = run_session(r['sess'], seq2, report)
    return r


def check_fixture_bits(case, device, report=None):
    """4: four session frames == model.inference() on a twin, all six outputs; the fixture's own 1e-3 bar; a graph was captured"""
    r = fixture_scenario(case, device, report)
    assert r['sess'].folded_sites == []
    assert_same_frames(r['e1'], r['s1'], case)
    for t, ref in enumerate(r['g']['fakes']):
        rel = _rel(r['s1'][t][0].cpu(), ref)
        print('session', case, 'frame', t, 'against the reference %.2e' % rel)
        assert rel <= 1e-3, (t, rel)
    for t, (out, u8) in enumerate(zip(r['s1'], r['u1'])):
        img = out[0].permute(0, 2, 3, 1).contiguous().cpu().numpy()
        assert np.array_equal(u8.cpu().numpy(), tensor2im_np(img)), t
    assert_captured(r['sess'], device, r['sess'].n_captures)
    if device.type == 'cuda':
        assert r['caps'] == 1


def check_two_sequences(case, device, report=None):
    """5: reset(), other references: the second sequence == eager after reset_inference(); no new capture"""
    r = fixture_scenario(case, device, report, second=True)
    assert_same_frames(r['e2'], r['s2'], case + ' (second sequence)')
    assert same_bits(r['e1'][0], r['e2'][0]), 'the second sequence must differ from the first (other references)'
    if device.type == 'cuda':
        assert r['sess'].n_captures == r['caps'] == 1 and r['sess'].capture_failures == []


def check_launch_accounting(device, report):
    """6 (emulator): a steady session frame launches no constant-recomputing kernel and at most the eager frame's launches minus the
    eager frame's count of those kernels.  Frame 3 is steady in both runs (frame 1 of the session still builds layouts)."""
    r = fixture_scenario('pose_combine', device, report)
    eager, sess = r['er1'][3], r['sr1'][3]
    assert r['er1'][2] == r['er1'][3], 'the eager frame is not steady'
    frozen_eager = _count(eager, FROZEN_KERNELS)
    assert frozen_eager > 0
    offenders = {k: v for k, v in sess.items() if k.lstrip('(').startswith(FROZEN_KERNELS)}
    assert offenders == {}, offenders
    u8 = _count(sess, ['fsv_cast_f2u8'])            # (frames_u8 is on in the shared run: its one launch is not the frame's)
    print('launches per steady frame: eager %d (constants %d), session %d' % (sum(eager.values()), frozen_eager,
                                                                               sum(sess.values()) - u8))
    assert sum(sess.values()) - u8 <= sum(eager.values()) - frozen_eager
    return r


# ------------------------------------------------------------------------------------------------ 7: fold_norms at model level
def check_fold_model(device, report=None):
    """7 / 6: fold_norms=True on the default fixture: three frames within the fixture's 1e-3 bar; fsv_norm_apply* launches drop by
    exactly len(folded_sites) on frame 0, the frame on which every folded layer runs exactly once (reference encoders once per
    sequence, flow network once: there is no previous frame yet), and by the folded layers a steady frame runs otherwise.  Returns
    the relative L2 distances to the eager frames."""
    infer = _mod('infer')
    base = fixture_scenario('pose_combine', device, report)
    opt, model, g = fixture_setup('pose_combine', device)
    sess = infer.InferenceSession(model, opt, fold_norms=True, warmup=1)
    n = len(sess.folded_sites)
    assert n > 0
    outs, _, reps = run_session(sess, fixture_sequence(g, opt, 4, device), report)
    dist = []
    for t, ref in enumerate(g['fakes']):
        rel = _rel(outs[t][0].cpu(), ref)
        dist.append(rel_l2(outs[t][0], base['e1'][t][0]))
        print('fold_norms frame', t, 'against the reference %.2e, relative L2 to the eager frame %.2e' % (rel, dist[-1]))
        assert rel <= 1e-3, (t, rel)
    assert_captured(sess, device)
    if report:
        norm = lambda rep: _count(rep, ['fsv_norm_apply'])
        assert norm(base['er1'][0]) - norm(reps[0]) == n, (norm(base['er1'][0]), norm(reps[0]), n)
        netG = model.netG
        per_frame = sum((2 if netG.flow_network_temp is netG.flow_network_ref else 1) for s in sess.folded_sites
                        if s.startswith('flow_network_ref.')) + sum(1 for s in sess.folded_sites if s.startswith('flow_network_temp.'))
        assert norm(base['sr1'][3]) - norm(reps[3]) == per_frame > 0, (norm(base['sr1'][3]), norm(reps[3]), per_frame)
        assert _count(reps[3], FROZEN_KERNELS) == 0
    sess.close()
    return dist


def check_fold_nothing_to_fold(device):
    """7: on the instance-normalised fixture no layer is foldable (no BatchNorm behind a convolution): folded_sites is empty and
    the frames are bit-equal to eager"""
    infer = _mod('infer')
    base = fixture_scenario('pose_combine_inorm', device)
    opt, model, g = fixture_setup('pose_combine_inorm', device)
    sess = infer.InferenceSession(model, opt, fold_norms=True, warmup=1)
    assert sess.folded_sites == []
    outs, _, _ = run_session(sess, fixture_sequence(g, opt, 3, device))
    assert_same_frames(base['e1'][:3], outs, 'inorm with fold_norms')
    sess.close()


# ------------------------------------------------------------------------------------------------ 4: the tiny configurations
NSHOT2 = dict(dataset_mode='fewshot_face', input_nc=1, n_shot=2, warp_ref=True)
RING2 = dict(warp_ref=True, spade_combine=True, remove_face_labels=True, n_frames_G=3, fineSize=32, loadSize=32, n_downsample_G=3,
             n_adaptive_layers=2)


def check_tiny_bits(device, kw, seed, b=1, scale=1.0):
    """4: `--n_shot 2 --warp_ref` (reference encoding and attention stay per frame) / n_frames_G = 3 (ring depth 2)"""
    infer = _mod('infer')
    opt, twin = tiny_setup(device, scale=scale, **kw)
    _, model = tiny_setup(device, scale=scale, **kw)
    seq = tiny_sequence(opt, 4, device, seed, b)
    sess = infer.InferenceSession(model, opt, warmup=1)
    e, _ = run_eager(twin, seq)
    s, _, _ = run_session(sess, seq)
    assert all(bool(torch.isfinite(x).all()) for x in _flat(e) if x is not None)
    assert_same_frames(e, s, str(kw))
    if opt.n_frames_G > 2:
        assert sess._ring[0].shape[1] == opt.n_frames_G - 1
    assert_captured(sess, device)
    assert same_bits(e[2], e[3]), 'frames of the sequence must differ'
    sess.close()


# ------------------------------------------------------------------------------------------------ 8: nothing leaks
TINY = dict(warp_ref=True, spade_combine=True, remove_face_labels=True, fineSize=32, loadSize=32, n_downsample_G=3, n_adaptive_layers=2)


def _train_step(model, opt, device, seed):
    M = mc._model()
    opt.isTrain = True
    model.isTrain = True
    model.train()
    opt_G, opt_D = model.build_optimizers()
    h = opt.fineSize
    tl, ti, rl, ri = [t.to(device) for t in mc.synth_pose_inputs(1, h, h, seed, opt.input_nc)]
    data = [tl, ti, [None, None], [None, None], rl, ri, None, None, None]
    d = M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
    g, _, _ = model(data, mode='generator')
    g = M.loss_backward(opt, g, opt_G, 0)
    return ([float(x.detach()) for x in d], [float(x.detach()) for x in g if not isinstance(x, int)], opt_G.flat_p.detach().clone(),
            opt_D.flat_p.detach().clone())


def check_nothing_leaks(device):
    """8: build a session (with fold_norms), run it, close() it: an eager inference sequence and one D + G training step then give
    the bits of a model that never had a session"""
    infer = _mod('infer')
    opt, clean = tiny_setup(device, temporal=False, **TINY)
    opt2, model = tiny_setup(device, temporal=False, **TINY)
    seq = tiny_sequence(opt, 3, device, 300)
    sess = infer.InferenceSession(model, opt2, fold_norms=True, frames_u8=True, warmup=1)
    assert sess.folded_sites
    run_session(sess, seq)
    sess.close()
    for m in model.modules():
        assert getattr(m, '_sig_frozen', None) is None and getattr(m, '_fsv_fold', None) is None
    for t in list(model.parameters()) + list(model.buffers()):
        assert not hasattr(t, '_fsv_frozen') and not hasattr(t, '_fsv_frozen_stats')
    assert model.netG._frozen_x is None and model._infer_session is None
    e0, _ = run_eager(clean, seq)
    e1, _ = run_eager(model, seq)
    assert_same_frames(e0, e1, 'eager inference after close()')
    a, b = _train_step(clean, opt, device, 310), _train_step(model, opt2, device, 310)
    assert a[0] == b[0] and a[1] == b[1], (a[0], b[0], a[1], b[1])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------------ 9: refreeze
def check_refreeze(device):
    """9: load_state_dict of different weights + refreeze(): the session follows the new weights and equals eager (without the
    refreeze it would go on with the old layouts, sigmas and operands)"""
    infer = _mod('infer')
    opt, twin = tiny_setup(device, **TINY)
    _, model = tiny_setup(device, **TINY)
    seq = tiny_sequence(opt, 3, device, 320)
    sess = infer.InferenceSession(model, opt, warmup=1)
    old, _, _ = run_session(sess, seq)
    new_sd = {k: ((mc.fill_value(k, v.shape, 0.8) * (0.9 if v.dim() == 1 else 1.0)).to(v.dtype)
                  if k.endswith(('weight', 'weight_orig', 'bias')) else v.clone())
              for k, v in model.netG.state_dict().items()}
    for net in (twin.netG, model.netG):
        net.load_state_dict(new_sd)
    sess.refreeze()
    e, _ = run_eager(twin, seq)
    s, _, _ = run_session(sess, seq)
    assert_same_frames(e, s, 'after refreeze()')
    assert same_bits(old[0], s[0]), 'the new weights must change the frames'
    assert_captured(sess, device, 2)
    sess.close()


# ------------------------------------------------------------------------------------------------ 10: --finetune
def check_finetune(device):
    """10: the session over the finetune fixture meets the bars of tests/test_golden._check_product_finetune"""
    import random
    infer = _mod('infer')
    opt, model, g = fixture_setup('pose_combine', device, finetune=True)
    random.seed(g['rng_seed'])
    frames = [mc.synth_pose_inputs(g['batch'], g['size'], g['size'], g['seed'] + t, 6) for t in range(2)]
    sess = model.use_inference_session(True)
    assert isinstance(sess, infer.InferenceSession)
    rl, ri = frames[0][2].to(device), frames[0][3].to(device)
    for t, (f, ref) in enumerate(zip(frames, g['fakes'])):
        fake = model([f[0].to(device), None, None, None, rl, ri, None, None, None])[0]      # forward(mode='inference'), as test.py calls it
        assert _rel(fake.cpu(), ref) <= 1e-3, t
    assert sess.t == 1
    assert _rel(model.netG.conv_img.weight.detach().cpu(), g['conv_img_weight']) <= 1e-3
    dw = model.netD.discriminator_0.model0[0].weight.detach().cpu()
    assert float((dw - g['d_first_weight']).norm() / g['d_first_weight'].norm()) <= 2e-3
    # the finetuned parameters are the optimiser's: they keep its layout cache, everything else is the session's
    owned = [p for p in model.netG.parameters() if getattr(p, '_fsv_cache', None) is not None]
    assert owned and all(not hasattr(p, '_fsv_frozen') for p in owned)
    model.use_inference_session(False)
    assert model._infer_session is None


def check_refusals(device):
    infer = _mod('infer')
    import pytest
    opt, model = tiny_setup(device, temporal=False, **TINY)
    model.train()
    with pytest.raises(RuntimeError, match='eval'):
        infer.InferenceSession(model, opt)
    model.eval()
    opt.isTrain = True
    with pytest.raises(RuntimeError, match='isTrain'):
        infer.InferenceSession(model, opt)
    opt.isTrain = False
    sess = model.inference_session()
    sess.close()
    with pytest.raises(RuntimeError, match='closed'):
        sess(None, None, None)
