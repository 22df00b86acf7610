"""Shared checks of the attention of n_shot > 1 in query bands (few-shot-vid2vid_amd/networks.py attention_band_plan,
FewShotGenerator.attention_module / attention_module_kept): the operator against a float64 restatement of generator.py:298-316 under
forced band sizes, the untouched default path launch for launch, the step level (the reference's n_shot 2 fixture, a tiny n_shot 3
D + G step), the kept session, the sizes past 2 GiB that the unbanded code refuses, and the host-side bounds.  Used by
tests/test_attn_band_emu.py (emulator) and tests/test_attn_band_gpu.py (hardware)."""
import contextlib
import os

import torch

import infer_nshot_checks as nc
import infer_session_checks as ic
import model_checks as mc
import op_checks

_mod = ic._mod
U = 2.0 ** -24                    # fp32 unit roundoff
SWITCH = 'FSV_ATTN_BAND_MB'

# the smallest shapes where banding can go wrong: two samples, three references, an odd h x w grid (no multiple of any tile)
B, N, C, H, W = 2, 3, 8, 6, 5
# rows per band -> bands per sample (h = 6).  'uneven': 4 + 2; 'one_row': six bands of one row; 'sample': the band is exactly one
# sample, so every band ends on a sample boundary; 'mid_sample': 5 + 1, a one-row remainder; 'whole': one band through the band code
FORCED = {'uneven': 4, 'one_row': 1, 'sample': 6, 'mid_sample': 5, 'whole': 12}
BANDS = {'uneven': 4, 'one_row': 12, 'sample': 2, 'mid_sample': 4, 'whole': 1}


def band_mb(rows, n, hw, w):
    """the switch value whose cap is `rows` query rows (and one byte): exact, the factor is a power of two"""
    return repr((rows * n * hw * w * 4 + 1) / float(1 << 20))


@contextlib.contextmanager
def forced(value):
    """FSV_ATTN_BAND_MB = value (None: unset) for the block; the switch is read per call"""
    old = os.environ.pop(SWITCH, None)
    if value is not None:
        os.environ[SWITCH] = value
    try:
        yield
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


@contextlib.contextmanager
def recorded_plans():
    """[plan or None] of every attention_band_plan call inside the block"""
    net = _mod('networks')
    orig, log = net.attention_band_plan, []

    def wrapped(*a):
        log.append(orig(*a))
        return log[-1]
    net.attention_band_plan = wrapped
    try:
        yield log
    finally:
        net.attention_band_plan = orig


@contextlib.contextmanager
def recorded_calls():
    """[(entry point, the scalar arguments)] of every library call inside the block"""
    lib = _mod('lib')
    orig, log = lib.call, []

    def wrapped(name, *args):
        log.append((name, tuple(a for a in args if isinstance(a, (int, float)) and not isinstance(a, bool))))
        return orig(name, *args)
    lib.call = wrapped
    try:
        yield log
    finally:
        lib.call = orig


def _names(log, prefixes=('fsv_conv_gather_fwd', 'fsv_softmax')):
    return [n for n, _ in log if n.startswith(prefixes)]


# ------------------------------------------------------------------------------------------------ the operator
def stub_generator(n, key, query):
    """a FewShotGenerator that is nothing but its attention: the encoders hand out `key` / `query`"""
    net = _mod('networks')
    g = torch.nn.Module.__new__(net.FewShotGenerator)
    torch.nn.Module.__init__(g)
    g.n_shot = n
    g.attention_encode = lambda img, name: key if name == 'atn_key' else query
    return g


def attention_ref(key, query, x, xl, n):
    """generator.py:298-316 (and the ref_idx of generator.py:366) in the dtype of its inputs - float64 here"""
    bn, c, h, w = x.shape
    b = bn // n
    k = key.view(b, n, c, -1).permute(0, 1, 3, 2).contiguous().view(b, -1, c)           # B x NHW x C
    q = query.view(b, c, -1)                                                             # B x C x HW
    attention = torch.softmax(torch.bmm(k, q), dim=1)                                    # B x NHW x HW

    def attend(t):
        ct = t.shape[1]
        return torch.bmm(t.view(b, n, ct, h * w).permute(0, 2, 1, 3).contiguous().view(b, ct, -1), attention).view(b, ct, h, w)
    vis = attention.view(b, n, h * w, h * w).sum(2).view(b, n, h, w)
    mass = attention.view(b, n, -1).sum(2)
    return attend(x), attend(xl), vis[-1:, 0:1], mass


def operator_inputs(seed=5):
    g = torch.Generator().manual_seed(seed)
    t = [torch.randn(B * N, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g),
         torch.randn(B * N, C, H, W, generator=g), torch.randn(B * N, C + 4, H, W, generator=g),
         torch.randn(B, C, H, W, generator=g), torch.randn(B, C + 4, H, W, generator=g)]
    return t          # key, query, image features, label features (another channel count), the two cotangents


_ref = {}


def operator_reference():
    """computed once, shared, never written"""
    if not _ref:
        key, query, x, xl, g0, g1 = [t.double() for t in operator_inputs()]
        leaves = [t.clone().requires_grad_(True) for t in (key, query, x, xl)]
        out, outl, vis, mass = attention_ref(*leaves, N)
        ((out * g0).sum() + (outl * g1).sum()).backward()
        top = torch.sort(mass.detach(), dim=1, descending=True)[0]
        assert float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 1e-3, 'the references tie: choose another seed'
        _ref.update(out=out.detach(), outl=outl.detach(), vis=vis.detach(), idx=torch.argmax(mass.detach(), dim=1),
                    grads=[t.grad for t in leaves])
    return _ref


def run_operator(device, grad, announce=True):
    """the product's attention on the operator inputs, the way reference_encoding calls it (announce: the label features are handed
    over before the first call, so a banded pass attends them in the same band loop)"""
    key, query, x, xl, g0, g1 = [t.to(device) for t in operator_inputs()]
    leaves = [t.clone().requires_grad_(grad) for t in (key, query, x, xl)]
    net = stub_generator(N, leaves[0], leaves[1])
    with torch.set_grad_enabled(grad), recorded_plans() as plans:
        if announce:
            net._atn_second = leaves[3]
        out, atn, vis = net.attention_module(leaves[2], None, None)
        net.__dict__.pop('_atn_second', None)
        outl, atn2, vis2 = net.attention_module(leaves[3], None, None, atn)
        assert atn2 is atn and torch.equal(vis, vis2)
        if torch.is_tensor(atn):
            idx = torch.argmax(atn.reshape(B, N, -1).sum(2), dim=1)
        else:
            idx = atn.ref_idx()
        grads = None
        if grad:
            ((out * g0).sum() + (outl * g1).sum()).backward()
            grads = [t.grad for t in leaves]
    return dict(out=out.detach(), outl=outl.detach(), vis=vis.detach(), idx=idx, grads=grads, plan=plans[0], atn=atn)


def assert_operator(got, what):
    ref = operator_reference()
    worst = {}
    for k in ('out', 'outl', 'vis'):
        assert tuple(got[k].shape) == tuple(ref[k].shape), (what, k, got[k].shape)
        worst[k] = op_checks.assert_close('%s: %s' % (what, k), got[k], ref[k], op_checks.REL_TOL)
    assert torch.equal(got['idx'].cpu(), ref['idx']), (what, got['idx'], ref['idx'])
    if got['grads'] is not None:
        for name, a, r in zip(('d key', 'd query', 'd image features', 'd label features'), got['grads'], ref['grads']):
            assert a is not None, (what, name)
            worst[name] = op_checks.assert_close('%s: %s' % (what, name), a, r, op_checks.REL_TOL)
    print('%s: relative to float64 %s' % (what, {k: '%.1e' % v for k, v in worst.items()}))


def check_operator(device, mode, grad, announce=True):
    """1: banded (`mode` of FORCED) and unbanded on the same inputs through the same comparison against float64, bar
    op_checks.REL_TOL: out for both feature maps, atn_vis, ref_idx, and with `grad` the gradients w.r.t. the key features, the query
    features and the two reference features"""
    net = _mod('networks')
    with forced(None):
        plain = run_operator(device, grad, announce)
    assert plain['plan'] is None and torch.is_tensor(plain['atn'])
    assert_operator(plain, 'unbanded')
    with forced(band_mb(FORCED[mode], N, H * W, W)):
        got = run_operator(device, grad, announce)
    plan = got['plan']
    assert isinstance(got['atn'], net.AttentionBands) and plan is not None and len(plan) == BANDS[mode], plan
    # the bands tile [0, b) x [0, h) in memory order, each a whole-sample range or rows of one sample
    cover = torch.zeros(B, H, dtype=torch.int32)
    for s0, s1, r0, r1 in plan:
        assert 0 <= s0 < s1 <= B and 0 <= r0 < r1 <= H and (s1 - s0 == 1 or (r0, r1) == (0, H)), plan
        assert (s1 - s0) * (r1 - r0) <= FORCED[mode]
        cover[s0:s1, r0:r1] += 1
    assert bool((cover == 1).all()) and plan == sorted(plan), plan
    if mode == 'uneven':
        assert [r1 - r0 for _, _, r0, r1 in plan] == [4, 2, 4, 2]
    assert_operator(got, 'bands of %d rows (%s, grad %s, announced %s)' % (FORCED[mode], mode, grad, announce))
    if not grad:
        assert got['atn'].bands is None             # nothing band-sized outlives the loop


def parent_attention(net, x, label, label_ref, attention=None):
    """the attention_module of before the band code, statement for statement: the launches the default path must still issue"""
    ops = _mod('ops')
    bn, c, h, w = x.shape
    n = net.n_shot
    b = bn // n
    hw = h * w
    if attention is None:
        key = net.attention_encode(label_ref, 'atn_key')
        query = net.attention_encode(label, 'atn_query')
        kmat = key.reshape(b, n, c, hw).permute(0, 1, 3, 2).reshape(b, n * hw, c, 1, 1)
        energy_t = ops.batch_conv(query, kmat, allow_half=False)
        attention = ops.softmax_channels(energy_t)
    xmat = x.reshape(b, n, c, hw).permute(0, 2, 1, 3).reshape(b, c, n * hw, 1, 1)
    out = ops.batch_conv(attention, xmat, allow_half=False)
    atn_vis = attention.reshape(b, n, hw, h, w).sum(2)[-1:, 0:1]
    return out, attention, atn_vis


def check_default_path(device):
    """2: switch unset, sizes under the limit: two gather-GEMMs and one softmax for the first feature map, one gather-GEMM for the
    second - the whole recorded call sequence (entry points and scalar arguments) is that of the code without bands, the outputs
    are its bits; with and without autograd, announced second map or not"""
    key, query, x, xl = [t.to(device) for t in operator_inputs()[:4]]
    xl = xl[:, :C].contiguous()
    net = stub_generator(N, key, query)
    for grad in (False, True):
        with forced(None), torch.set_grad_enabled(grad):
            with recorded_calls() as want:
                o0, a0, v0 = parent_attention(net, x, None, None)
                cut = len(want)
                l0, _, _ = parent_attention(net, xl, None, None, a0)
            for announce in (False, True):
                with recorded_calls() as got:
                    if announce:
                        net._atn_second = xl
                    o1, a1, v1 = net.attention_module(x, None, None)
                    net.__dict__.pop('_atn_second', None)
                    cut1 = len(got)
                    l1, a2, _ = net.attention_module(xl, None, None, a1)
                assert got == want and cut1 == cut, (_names(got), _names(want))
                assert _names(got[:cut]) == ['fsv_conv_gather_fwd', 'fsv_softmax_rows_fwd', 'fsv_conv_gather_fwd']
                assert _names(got[cut:]) == ['fsv_conv_gather_fwd']
                assert torch.is_tensor(a1) and a2 is a1
                assert not ic.same_bits([o0, a0, v0, l0], [o1, a1, v1, l1])


# ------------------------------------------------------------------------------------------------ the band rule
def check_band_rule():
    """the automatic rule at the sizes of the pose configuration (hw = 128 x 128): exactly 2 GiB is one launch, anything more is
    split into the largest bands that fit - whole samples while a sample fits, rows of one sample otherwise"""
    net = _mod('networks')
    cap = net.ATTN_LAUNCH_MAX_BYTES
    assert cap == 1 << 31
    hw = 128 * 128
    with forced(None):
        assert net.attention_band_plan(1, 2, hw, 128, 128) is None                    # 2 GiB exactly: the unbanded code
        assert net.attention_band_plan(2, 2, hw, 128, 128) == [(0, 1, 0, 128), (1, 2, 0, 128)]
        assert net.attention_band_plan(1, 3, hw, 128, 128) == [(0, 1, 0, 85), (0, 1, 85, 128)]
        assert net.attention_band_plan(1, 4, hw, 128, 128) == [(0, 1, 0, 64), (0, 1, 64, 128)]
        assert net.attention_band_plan(4, 1, hw, 128, 128) == [(0, 2, 0, 128), (2, 4, 0, 128)]
        assert net.attention_band_plan(3, 1, hw, 128, 128) == [(0, 2, 0, 128), (2, 3, 0, 128)]
        assert net.attention_band_plan(1, 2, hw + 128, 129, 128) is not None           # one row more than 2 GiB
        for b, n in ((2, 2), (1, 3), (1, 4), (2, 3), (5, 1)):
            for s0, s1, r0, r1 in net.attention_band_plan(b, n, hw, 128, 128):
                assert (s1 - s0) * (r1 - r0) * 128 * n * hw * 4 <= cap
    with forced('1024'):
        assert net.attention_band_plan(1, 2, hw, 128, 128) == [(0, 1, 0, 64), (0, 1, 64, 128)]
        assert net.attention_band_plan(2, 1, hw, 128, 128) == [(0, 1, 0, 128), (1, 2, 0, 128)]
    with forced('4096'):             # never above the launch bound
        assert net.attention_band_plan(1, 2, hw, 128, 128) == [(0, 1, 0, 128)]
        assert len(net.attention_band_plan(1, 3, hw, 128, 128)) == 2
    import pytest
    with forced('0'), pytest.raises(ValueError):
        net.attention_band_plan(1, 2, 64, 8, 8)
    with forced(repr(1e-6)), pytest.raises(ValueError, match='one row'):
        net.attention_band_plan(1, 2, 64, 8, 8)


# ------------------------------------------------------------------------------------------------ 3: the step level
def check_fixture_step(device, case='face_nshot2', bands=3):
    """the reference's n_shot 2 iteration (tests/golden/step_face_nshot2.pt) with the attention forced into at least `bands` bands
    per sample: the comparison and the bars of test_golden.test_product_reproduces_reference_iteration_on_gpu"""
    from test_golden import _check_grad_norms, _check_grad_sketches, _inputs, _load, _opt_from_flags, _rel
    g = _load(case)
    opt = _opt_from_flags(g['flags'])
    M = mc._model()
    model = M.create_model(opt)
    mc.fill_state(model.netG); mc.fill_state(model.netD)
    assert model.netDf is None and model.netGf is None
    model = model.to(device).train()
    opt_G, opt_D = model.build_optimizers()
    opt_G.set_lr(0.0); opt_D.set_lr(0.0)
    tl, ti, rl, ri = [t.to(device) for t in _inputs(g, opt)]
    data = [tl, ti, [None, None], [None, None], rl, ri, None, None, None]
    side = g['size'] >> model.netG.n_downsample_A
    rows = max(1, side // bands)
    with forced(band_mb(rows, opt.n_shot, side * side, side)), recorded_plans() as plans:
        d = M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
        _check_grad_norms(model.netD, g['grad_norm_D'], 'netD')
        _check_grad_sketches(model.netD, g['grad_sketch_D'], g['grad_norm_D'], 'netD')
        gl, generated, _ = model(data, save_images=True, mode='generator')
        gl = M.loss_backward(opt, gl, opt_G, 0)
    assert len(plans) >= 2 and all(p is not None and len(p) >= bands * g['batch'] for p in plans), plans
    _check_grad_norms(model.netG, g['grad_norm_G'], 'netG')
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


def check_tiny_step(device, banded):
    """one D + G step of the `nshot3` tiny configuration of infer_nshot_checks (32 x 32 frames, attention at 8 x 8: hw = 64) through
    model_checks.check_train_step - losses, image and per-parameter gradient norms against the oracle pair at its bars - banded
    (3 + 3 + 2 rows per sample) and unbanded: the same comparison, the same bars, the same (shared) oracle"""
    kw = dict(nc.CONFIGS['nshot3'][0])
    opt = mc.tiny_opt(**kw)
    with forced(band_mb(3, 3, 64, 8) if banded else None), recorded_plans() as plans:
        mc.check_train_step(device, opt, b=1)
    assert len(plans) >= 2, plans
    if banded:
        assert all(p == [(0, 1, 0, 3), (0, 1, 3, 6), (0, 1, 6, 8)] for p in plans), plans
    else:
        assert all(p is None for p in plans), plans


# ------------------------------------------------------------------------------------------------ 4: the kept session
# What a band changes is the fp32 summation ORDER of the weighted-sum GEMM (K = n hw products per output; the split-K plan depends
# on the pixel count of a launch) - the energy GEMM (K = c, one chunk) and the softmax are per query pixel and keep their bits.  The
# attended feature of a band therefore differs from the unbanded one by at most 2 K u sum_k |a_k x_k| <= 2 K u max|x| (two orderings
# of the same K products, each within K u of the exact sum; the attention weights sum to 1).  The network behind it is held to the
# same relative bound on every output, 2 K u of the output's range, times SESSION_GAIN for its conditioning: the generator maps a
# relative perturbation of one encoder feature to a relative perturbation of its outputs of the same order (the step-level tests put
# the end-to-end gain of rounding-level perturbations at < 10 for these networks: 1e-3 bars from 1e-4-level kernel differences).
SESSION_GAIN = 10.0


def session_bound(n, hw):
    return SESSION_GAIN * 2 * n * hw * U


def check_session(device, rows=3):
    """inference_session(keep_references=True) with forced bands (3 + 3 + 2 rows of the 8 x 8 grid), four frames, two sequences
    through ONE session, against the unbanded kept session of infer_nshot_checks' shared scenario: every output but atn_vis within
    session_bound of the output's range, atn_vis within the two fp32 reductions' own bound, ref_idx equal; on the GPU the steady
    frame is a replayed capture that contains the band launches"""
    infer = _mod('infer')
    r = nc.scenario('mul', device)
    nc.check_two_sequences(device)                                # (fills r['got2'] / r['eager2'] once)
    opt = r['opt']
    kw, _ = nc.CONFIGS['mul']
    _, model = ic.tiny_setup(device, **kw)
    n, hw, side = opt.n_shot, 64, 8
    bound = session_bound(n, hw)
    with forced(band_mb(rows, n, hw, side)), recorded_plans() as plans:
        sess = infer.InferenceSession(model, opt, warmup=1, keep_references=True)
        sess.keep_graph = device.type == 'cuda'
        seq2 = ic.tiny_sequence(opt, 4, device, nc.SECOND_SEQUENCE_SEED)
        got = nc.run_session(sess, r['seq'])
        graph, caps = sess._graph, sess.n_captures
        band = sess._kept.band
        got2 = nc.run_session(sess, seq2)
    assert plans and all(p == [(0, 1, 0, 3), (0, 1, 3, 6), (0, 1, 6, 8)] for p in plans), plans
    assert band is not None and sess._kept.band is band and band.numel() == rows * side * n * hw
    assert sess._graph is graph and sess.n_captures == caps and sess.capture_failures == []
    ic.assert_captured(sess, device)
    worst = 0.0
    for what, want, have in (('first sequence', r['got'], got), ('second sequence', r['got2'], got2)):
        assert len(want[0]) == len(have[0]) == 4
        for t, (a, b) in enumerate(zip(want[0], have[0])):
            assert len(a) == len(b) == 6
            for i, (x, y) in enumerate(zip(ic._flat(a[:5]), ic._flat(b[:5]))):
                assert (x is None) == (y is None), (what, t, i)
                if x is None:
                    continue
                assert x.shape == y.shape and bool(torch.isfinite(y).all())
                rel = float((x.double() - y.double()).abs().max() / max(float(x.abs().max()), 1e-12))
                worst = max(worst, rel)
                assert rel <= bound, '%s frame %d output %d: %.3e > %.3e' % (what, t, i, rel, bound)
            assert torch.equal(want[1][t], have[1][t]), (what, t)
            va, vb = a[5].double().cpu(), b[5].double().cpu()
            assert va.shape == vb.shape and bool(((va - vb).abs() <= 2 * hw * U * va).all()), (what, t)
    print('banded kept session against the unbanded one: worst relative difference %.3e (bound %.3e)' % (worst, bound))
    assert ic.same_bits(got[0][1], got2[0][1]), 'the second sequence must differ from the first'
    sess.close()
    assert sess._kept.band is None


# ------------------------------------------------------------------------------------------------ 5: past 2 GiB (hardware only)
REAL_CASES = {'b2_n2': (2, 2, 128, 8), 'b1_n3': (1, 3, 128, 8)}


def check_real_limit(device, name):
    """(b, n, h = w, c) whose attention tensor is 4 GiB / 3 GiB: the unbanded code refuses them (FsvError, fsv_status -2).  Forward
    under no_grad against float64 on the device, computed in chunks of 8 query rows (no float64 tensor over 1 GiB): out and atn_vis at
    op_checks.REL_TOL; peak allocated memory below one full attention tensor; the launches are those of the plan.
    b2_n2: the per-sample launches still count the bytes of all their samples (csrc/conv_igemm.hip, include/fsv2v.h), so the plan
    keeps one band per sample: 2 x (2 gather-GEMMs + 1 softmax)."""
    b, n, side, c = REAL_CASES[name]
    h = w = side
    hw = h * w
    full = b * n * hw * hw * 4
    g = torch.Generator().manual_seed(11)
    key = torch.randn(b * n, c, h, w, generator=g).to(device)
    query = torch.randn(b, c, h, w, generator=g).to(device)
    x = torch.randn(b * n, c, h, w, generator=g).to(device)
    net = stub_generator(n, key, query)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    with forced(None), torch.no_grad(), recorded_plans() as plans, recorded_calls() as calls:
        out, atn, vis = net.attention_module(x, None, None)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    plan = plans[0]
    print('%s: attention tensor %.2f GiB, peak allocated %.2f GiB, plan %s' % (name, full / 2.0 ** 30, peak / 2.0 ** 30, plan))
    assert peak < full, (peak, full)
    assert plan == ([(0, 1, 0, 128), (1, 2, 0, 128)] if name == 'b2_n2' else [(0, 1, 0, 85), (0, 1, 85, 128)])
    names = _names(calls)
    assert names == ['fsv_conv_gather_fwd', 'fsv_softmax_rows_fwd', 'fsv_conv_gather_fwd'] * len(plan), names
    mass = atn.mass.clone()
    del atn
    # float64, eight query rows at a time
    k = key.double().view(b, n, c, hw).permute(0, 1, 3, 2).reshape(b, n * hw, c)
    xm = x.double().view(b, n, c, hw).permute(0, 2, 1, 3).reshape(b, c, n * hw)
    q = query.double().view(b, c, hw)
    want = torch.empty(b, c, hw, dtype=torch.float64, device=device)
    want_mass = torch.empty(b, n, hw, dtype=torch.float64, device=device)
    step = 8 * w
    assert b * n * hw * step * 8 <= 1 << 30
    for p0 in range(0, hw, step):
        a = torch.softmax(torch.bmm(k, q[:, :, p0:p0 + step]), dim=1)
        want[:, :, p0:p0 + step] = torch.bmm(xm, a)
        want_mass[:, :, p0:p0 + step] = a.view(b, n, hw, -1).sum(2)
        del a
    op_checks.assert_close('%s: out' % name, out, want.view(b, c, h, w), op_checks.REL_TOL)
    op_checks.assert_close('%s: atn_vis' % name, vis, want_mass.view(b, n, h, w)[-1:, 0:1], op_checks.REL_TOL)
    op_checks.assert_close('%s: masses' % name, mass.permute(0, 3, 1, 2), want_mass.view(b, n, h, w), op_checks.REL_TOL)


# ------------------------------------------------------------------------------------------------ 6: host-side bounds
def check_host_bounds(device):
    """the documented per-launch bounds (include/fsv2v.h), probed on untouched buffers with calls that return before any launch:
    the row softmax refuses more than 4 (2^24 - 1) rows, forward and backward (FSV_ERR_UNSUPPORTED - argument errors still come
    first); a per-sample gather-GEMM counts the input bytes of ALL its samples: 2 GiB and one pixel is refused"""
    lib = _mod('lib')
    unsup, bad = lib.ENUMS['FSV_ERR_UNSUPPORTED'], lib.ENUMS['FSV_ERR_BAD_ARG']
    x = torch.empty(64, device=device)
    y = torch.empty(64, device=device)
    z = torch.empty(64, device=device)
    top = 4 * ((1 << 24) - 1)

    def fwd(rows, c, groups=0, gsum=None):
        return lib.call_status("fsv_softmax_rows_fwd", lib.ptr(x), lib.ptr(y), rows, c, groups, lib.ptr(gsum), lib.stream_ptr())

    def bwd(rows, c):
        return lib.call_status("fsv_softmax_rows_bwd", lib.ptr(x), lib.ptr(y), lib.ptr(z), rows, c, lib.stream_ptr())
    assert fwd(top + 1, 4) == unsup and bwd(top + 1, 4) == unsup
    assert fwd(1 << 40, 1 << 20) == unsup and bwd(1 << 40, 1 << 20) == unsup
    assert fwd(top + 1, 4, 2, z) == unsup
    assert fwd(top + 1, 0) == bad and bwd(top + 1, 0) == bad and fwd(top + 1, 4, 3, z) == bad     # argument errors first
    assert fwd(16, 4) == 0 and bwd(16, 4) == 0                                                       # (inside the bound: launched)
    # gather-GEMM, per-sample 1x1: N x H x W x Cin x 4 bytes of input over 2 GiB -> refused whatever the sample's own size
    zero = lib.int_array([0])

    def gemm(n, h, w, cin, cout=32, per_sample=1):
        return lib.call_status("fsv_conv_gather_fwd", lib.ptr(x), lib.ptr(y), None, None, lib.ptr(z), n, h, w, cin, h, w, cout, 1,
                               zero, zero, 1, 1, h, w, 1, 1, 0, 0, 32, (cin + 31) // 32 * 32 * 32, 0, per_sample, 0, 1.0, -1, 0, 0,
                               None, None, 0, 0, lib.stream_ptr())
    assert gemm(2, 128, 128, 2 * 128 * 128 + 4) == unsup                  # 4 GiB and a bit, 2 GiB and a bit per sample
    assert gemm(2, 128, 128, 128 * 128 + 4) == unsup                      # 2 GiB and 512 KiB in all: each sample is half of it
    assert gemm(2, 128, 128, 128 * 128 + 4, per_sample=0) == unsup
