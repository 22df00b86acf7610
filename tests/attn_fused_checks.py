"""Shared checks of the streaming few-shot attention (few-shot-vid2vid_amd/csrc/attention.hip, ops.attention_fused, the
FSV_ATTN_FUSED switch of networks.FewShotGenerator.attention_module, InferenceSession(fused_attention=True)): the operator against the
float64 restatement of generator.py:298-316 (attn_band_checks.attention_ref) at the smallest ragged shape and at more than one tile
each way, the online-softmax rescaling under energies in the hundreds, determinism, the untouched default path, fallback and
bounds, the step level, the kept session and - hardware only - the real size.  Used by tests/test_attn_fused_emu.py (emulator)
and tests/test_attn_fused_gpu.py (hardware)."""
import contextlib
import os

import torch

import attn_band_checks as ab
import infer_nshot_checks as nc
import infer_session_checks as ic
import model_checks as mc
import op_checks

_mod = ic._mod
U = ab.U
SWITCH = 'FSV_ATTN_FUSED'
ENTRY = 'fsv_attention_fused_fwd'

# (b, n, c, c0, c1, h, w).  small: the inputs of attn_band_checks.operator_inputs - 30 positions, no multiple of any tile, one key
# tile of 32 holds two reference boundaries.  prod: the production channel counts, both maps in one launch, 72 queries x 144 keys.
# ragged: 99 queries (a tail in the query tile), 198 keys with the reference boundary inside a key tile, a 36-channel second map
# (a partial 32-channel output tile).
# wide: 128 < c <= 256 runs the kernel's second instantiation (no prefetch registers, four output tiles per walk, its own K / V
# staging geometry) - c = 160 is five of its eight 32-channel query chunks, hw = 35 is ragged both ways (70 keys: two full key tiles
# and six keys), 5 + 4 output tiles (the last of the 100-channel map partial) are three walks, the middle one across both maps.
# two_walks: c <= 128 with c0 + c1 > 256: nine output tiles, two walks of the prefetching instantiation, the second one a single tile
# of the second map from column 128.
SHAPES = {'small': (ab.B, ab.N, ab.C, ab.C, ab.C + 4, ab.H, ab.W), 'prod': (1, 2, 128, 128, 128, 8, 9), 'ragged': (1, 2, 32, 32, 36, 9, 11),
          'wide': (1, 2, 160, 160, 100, 7, 5), 'two_walks': (1, 2, 128, 128, 160, 7, 5)}
SEEDS = {'prod': 21, 'ragged': 22, 'wide': 23, 'two_walks': 24}
WALKS = {'wide': {2: 3, 1: 2}, 'two_walks': {2: 2, 1: 1}}          # case -> {value maps: walks over the keys}


@contextlib.contextmanager
def switched(value):
    """FSV_ATTN_FUSED = value (None: unset) for the block; the switch is read per call"""
    old = os.environ.pop(SWITCH, None)
    if value is not None:
        os.environ[SWITCH] = value
    try:
        yield
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def inputs(case):
    """key, query, image features, label features"""
    if case == 'small':
        return ab.operator_inputs()[:4]
    b, n, c, c0, c1, h, w = SHAPES[case]
    g = torch.Generator().manual_seed(SEEDS[case])
    return [torch.randn(b * n, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g),
            torch.randn(b * n, c0, h, w, generator=g), torch.randn(b * n, c1, h, w, generator=g)]


_refs = {}


def reference(case, ts=None):
    """float64, computed once per input set, shared, never written"""
    if case not in _refs:
        n = SHAPES[case.split(':')[0]][1]
        key, query, x, xl = [t.double() for t in (ts if ts is not None else inputs(case))]
        out, outl, vis, mass = ab.attention_ref(key, query, x, xl, n)
        top = torch.sort(mass, dim=1, descending=True)[0]
        assert float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 1e-3, 'the references tie: choose another seed'
        full = torch.softmax(torch.bmm(key.view(query.shape[0], n, key.shape[1], -1).permute(0, 1, 3, 2).reshape(query.shape[0], -1, key.shape[1]),
                                       query.view(query.shape[0], key.shape[1], -1)), dim=1)
        b, hw = query.shape[0], query.shape[2] * query.shape[3]
        _refs[case] = dict(out=out, outl=outl, vis=vis, idx=torch.argmax(mass, dim=1),
                           mass=full.view(b, n, hw, hw).sum(2).permute(0, 2, 1))            # [b, hw, n]
    return _refs[case]


def run(device, ts, n, second, fused):
    """the product's attention the way reference_encoding calls it, under no_grad; second: 'announced' / 'unannounced' / 'absent'"""
    key, query, x, xl = [t.to(device) for t in ts]
    net = ab.stub_generator(n, key, query)
    with switched('1' if fused else None), ab.forced(None), torch.no_grad(), ab.recorded_calls() as calls:
        if second == 'announced':
            net._atn_second = xl
        out, atn, vis = net.attention_module(x, None, None)
        net.__dict__.pop('_atn_second', None)
        outl = None
        if second != 'absent':
            outl, atn2, vis2 = net.attention_module(xl, None, None, atn)
            assert atn2 is atn and torch.equal(vis, vis2)
        if torch.is_tensor(atn):
            idx = torch.argmax(atn.reshape(query.shape[0], n, -1).sum(2), dim=1)
        else:
            idx = atn.ref_idx()
    return dict(out=out, outl=outl, vis=vis, idx=idx, atn=atn, calls=calls)


def errors(got, ref):
    """max |difference| to float64 relative to the reference's range, per output"""
    e = {}
    for k in ('out', 'outl', 'vis'):
        if got[k] is not None:
            r = ref[k]
            e[k] = float((got[k].double().cpu() - r).abs().max() / max(float(r.abs().max()), 1e-6))
    return e


def assert_fused(device, case, ts, n, second, what):
    """the bars of check 1: out / outl / atn_vis within op_checks.REL_TOL, ref_idx equal, and the fused error against float64 at most
    the larger of 4x the unfused path's error on the same inputs (the fold_norms precedent) and the fp32 summation bound
    n hw 2^-24 of the output's range"""
    net = _mod('networks')
    ref = reference(case, ts)
    hw = ts[1].shape[2] * ts[1].shape[3]
    got = run(device, ts, n, second, True)
    plain = run(device, ts, n, second, False)
    assert isinstance(got['atn'], net.AttentionFused) and torch.is_tensor(plain['atn'])
    names = [c[0] for c in got['calls']]
    assert names == [ENTRY] * (2 if second == 'unannounced' else 1), names
    e_f, e_p = errors(got, ref), errors(plain, ref)
    print('%s: fused %s, unfused %s (relative to float64)' % (what, {k: '%.1e' % v for k, v in e_f.items()},
                                                               {k: '%.1e' % v for k, v in e_p.items()}))
    for k in e_f:
        assert tuple(got[k].shape) == tuple(ref[k].shape), (what, k)
        assert bool(torch.isfinite(got[k]).all()), (what, k)
        op_checks.assert_close('%s: %s' % (what, k), got[k], ref[k], op_checks.REL_TOL)
        assert e_f[k] <= max(4 * e_p[k], n * hw * U), (what, k, e_f[k], e_p[k], n * hw * U)
    assert torch.equal(got['idx'].cpu(), ref['idx']), (what, got['idx'], ref['idx'])
    m = got['atn'].mass.double().cpu().reshape(ref['mass'].shape)
    assert float((m - ref['mass']).abs().max()) <= op_checks.REL_TOL * float(ref['mass'].max())
    got['plain_err'] = e_p
    return got


def check_operator(device, case, second='announced'):
    """1, 2: the operator through attention_module with the switch on, against float64"""
    ts = inputs(case)
    if case == 'small':          # the shared reference of attn_band_checks answers for the same inputs
        r = ab.operator_reference()
        mine = reference(case, ts)
        assert torch.equal(r['idx'], mine['idx'])
        assert max(float((r[k] - mine[k]).abs().max()) for k in ('out', 'outl', 'vis')) <= 1e-12
    assert_fused(device, case, ts, SHAPES[case][1], second, '%s, second map %s' % (case, second))


def check_splits(device):
    """the key ranges of a query tile: one workgroup walking all keys (no workspace for the sums, the normalisation in the kernel's own
    epilogue), two and three ranges combined by the finishing pass - each against float64 at the bars of check 1, with and without
    the masses, with one and with two value maps"""
    ops, lib = _mod('ops'), _mod('lib')

    def launches():
        return int(lib.get_lib().fsv_emu_launch_count()) if lib.is_emu() else 0
    for case in ('small', 'ragged'):
        b, n, c, c0, c1, h, w = SHAPES[case]
        ts = inputs(case)
        ref = reference(case, ts)
        key, query, x, xl = [t.to(device) for t in ts]
        with torch.no_grad():
            for split in (1, 2, 3):
                for vals, want_mass in (([x, xl], True), ([x], True), ([x], False)):
                    n0 = launches()
                    outs, mass = ops.attention_fused(query, key, vals, n, want_mass=want_mass, split=split)
                    assert (mass is not None) == want_mass
                    if lib.is_emu():         # one launch, plus the finishing launch where there is something to finish
                        assert launches() - n0 == (2 if (split > 1 or want_mass) else 1)
                    for o, k in zip(outs, ('out', 'outl')):
                        e = float((o.double().cpu() - ref[k]).abs().max() / float(ref[k].abs().max()))
                        assert e <= max(n * h * w * U, 4e-7), (case, split, k, e)
                    if want_mass:
                        m = mass.double().cpu().reshape(ref['mass'].shape)
                        assert float((m - ref['mass']).abs().max()) <= n * h * w * U
                        assert float((m.sum(-1) - 1).abs().max()) <= n * h * w * U


def check_walks(device, case, second):
    """more output tiles than one walk over the keys carries (SHAPES 'wide': the 128 < c <= 256 instantiation, 'two_walks': the
    prefetching one with c0 + c1 > 256), at the bars of check 1: through attention_module with the library's own key ranges (more
    than one at these sizes: the finishing pass combines the walks' workspace copies), then the operator itself with ONE key range
    (every walk normalises in its own epilogue) and with two, with and without the masses"""
    ops, lib = _mod('ops'), _mod('lib')
    b, n, c, c0, c1, h, w = SHAPES[case]
    ts = inputs(case)
    ref = reference(case, ts)
    got = assert_fused(device, case, ts, n, second, '%s, second map %s' % (case, second))
    assert all(cc[1][6] > 1 for cc in got['calls']), got['calls']             # (the scalar arguments: b, n, hw, c, c0, c1, nsplit)
    key, query, x, xl = [t.to(device) for t in ts]
    vals = [x] if second == 'absent' else [x, xl]
    for split in (1, 2):
        for want_mass in (True, False):
            n0 = int(lib.get_lib().fsv_emu_launch_count()) if lib.is_emu() else 0
            with torch.no_grad():
                outs, mass = ops.attention_fused(query, key, vals, n, want_mass=want_mass, split=split)
            if lib.is_emu():                 # one launch per walk, plus the finishing launch where there is something to finish
                assert int(lib.get_lib().fsv_emu_launch_count()) - n0 == WALKS[case][len(vals)] + (1 if (split > 1 or want_mass) else 0)
            for o, k in zip(outs, ('out', 'outl')):
                assert bool(torch.isfinite(o).all())
                e = op_checks.assert_close('%s split %d: %s' % (case, split, k), o, ref[k], op_checks.REL_TOL)
                assert e <= max(4 * got['plain_err'][k], n * h * w * U), (case, split, k, e, got['plain_err'][k])
            if want_mass:
                m = mass.double().cpu().reshape(ref['mass'].shape)
                assert float((m - ref['mass']).abs().max()) <= op_checks.REL_TOL * float(ref['mass'].max())
                assert float((m.sum(-1) - 1).abs().max()) <= n * h * w * U
                assert torch.equal(torch.argmax(mass.sum((1, 2)), dim=1).cpu(), ref['idx'])


# ------------------------------------------------------------------------------------------------ 3: rescaling
def rescale_inputs(placement):
    """the small shape with the query scaled so that the energies reach the hundreds (a softmax without the running maximum
    overflows: exp(300) is not an fp32 number), and ONE key per sample whose energy is the largest of every query by 2:
    'first': key 1 of reference 0 - the maximum is met in the first tile and every later tile only adds;
    'last': the very last key of the last reference - the running maximum rises at the end, after every reference's keys have passed,
    so every accumulated sum and every reference's partial mass is rescaled"""
    key, query, x, xl = [t.clone() for t in ab.operator_inputs()[:4]]
    b, n, c, h, w = ab.B, ab.N, ab.C, ab.H, ab.W
    hw = h * w
    query = query * 40.0
    k = key.view(b, n, c, hw)
    k[:, :, 0, :] = 0.0                                # channel 0 belongs to the planted key: the other energies do not read it
    g, pos = (0, 1) if placement == 'first' else (n - 1, hw - 1)
    k[:, g, :, pos] = 0.0
    k[:, g, 0, pos] = 16.0
    q = query.view(b, c, hw)
    q[:, 0, :] = 0.0
    e = torch.bmm(k.permute(0, 1, 3, 2).reshape(b, n * hw, c).double(), q.double())       # the planted key's row is 0 here
    top = e.max(dim=1)[0]                                                                   # [b, hw]
    assert float(top.min()) > 100.0, float(top.min())
    q[:, 0, :] = ((top + 2.0) / 16.0).float()
    e = torch.bmm(k.permute(0, 1, 3, 2).reshape(b, n * hw, c).double(), q.double())
    assert bool((e.argmax(dim=1) == g * hw + pos).all()) and float(e.max()) > 200.0
    return [key, query, x, xl]


def check_rescale(device, placement):
    """3: against float64 at the bars of check 1; every value finite; the masses of a query sum to 1 within n hw 2^-24"""
    ts = rescale_inputs(placement)
    got = assert_fused(device, 'small:' + placement, ts, ab.N, 'announced', 'energies in the hundreds, maximum %s' % placement)
    mass = got['atn'].mass
    assert bool(torch.isfinite(mass).all())
    assert float((mass.double().sum(-1) - 1).abs().max()) <= ab.N * ab.H * ab.W * U


# ------------------------------------------------------------------------------------------------ 4: determinism
def check_determinism(device):
    ops = _mod('ops')
    old = os.environ.pop('FSV_DETERMINISTIC', None)
    try:
        res = []
        for case in ('small', 'prod'):
            key, query, x, xl = [t.to(device) for t in inputs(case)]
            for det in (None, '1', None):
                if det is None:
                    os.environ.pop('FSV_DETERMINISTIC', None)
                else:
                    os.environ['FSV_DETERMINISTIC'] = det
                with torch.no_grad():
                    outs, mass = ops.attention_fused(query, key, [x, xl], SHAPES[case][1])
                res.append(outs + [mass])
            assert not ic.same_bits(res[-3], res[-2]) and not ic.same_bits(res[-3], res[-1]), case
    finally:
        os.environ.pop('FSV_DETERMINISTIC', None)
        if old is not None:
            os.environ['FSV_DETERMINISTIC'] = old


# ------------------------------------------------------------------------------------------------ 5: the default path
def check_default_path(device):
    """switch unset: attn_band_checks.check_default_path - the recorded calls and the bits of the code before the bands.  Switch on
    under no_grad: the fused entry point and no gather-GEMM / softmax launch.  Switch on with autograd: the recording of the
    switch-off pass, and the gradients pass attn_band_checks' float64 comparison."""
    with switched(None):
        ab.check_default_path(device)
    ts = inputs('small')
    fused = run(device, ts, ab.N, 'announced', True)
    names = [c[0] for c in fused['calls']]
    assert ENTRY in names and not ab._names(fused['calls']), names
    with ab.forced(None):
        with switched(None), ab.recorded_calls() as off:
            plain = ab.run_operator(device, True)
        with switched('1'), ab.recorded_calls() as on:
            got = ab.run_operator(device, True)
    assert on == off and ENTRY not in [c[0] for c in on]
    assert torch.is_tensor(got['atn'])
    assert not ic.same_bits([plain['out'], plain['outl'], plain['vis']] + plain['grads'], [got['out'], got['outl'], got['vis']] + got['grads'])
    ab.assert_operator(got, 'switch on, autograd enabled')


# ------------------------------------------------------------------------------------------------ 6: fallback and bounds
def check_fallback(device):
    """c = 6 is no multiple of 4: attention_module with the switch on runs today's launches, and is correct"""
    b, n, c, h, w = 2, 3, 6, 6, 5
    g = torch.Generator().manual_seed(9)
    ts = [torch.randn(b * n, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g),
          torch.randn(b * n, c, h, w, generator=g), torch.randn(b * n, c, h, w, generator=g)]
    SHAPES['c6'] = (b, n, c, c, c, h, w)
    ref = reference('c6', ts)
    got = run(device, ts, n, 'announced', True)
    plain = run(device, ts, n, 'announced', False)
    assert torch.is_tensor(got['atn']) and got['calls'] == plain['calls']
    assert ab._names(got['calls']) == ['fsv_conv_gather_fwd', 'fsv_softmax_rows_fwd', 'fsv_conv_gather_fwd', 'fsv_conv_gather_fwd']
    for k in ('out', 'outl', 'vis'):
        op_checks.assert_close('c = 6: %s' % k, got[k], ref[k], op_checks.REL_TOL)
    assert torch.equal(got['idx'].cpu(), ref['idx'])
    ops = _mod('ops')
    key, query, x, xl = [t.to(device) for t in ts]
    assert not ops.attention_fused_supported(query, key, [x, xl], n)
    sk, sq, sx, sxl = [t.to(device) for t in inputs('small')]
    assert ops.attention_fused_supported(sq, sk, [sx], ab.N) and ops.attention_fused_supported(sq, sk, [sx, sxl], ab.N)
    assert not ops.attention_fused_supported(sq, sk, [sx], ab.N - 1)
    import pytest
    with pytest.raises(_mod('lib').FsvError):
        ops.attention_fused(query, key, [x], n)
    with pytest.raises(ValueError), torch.enable_grad():
        ops.attention_fused(query.clone().requires_grad_(True), key, [x], n)


def check_bounds(device):
    """the entry point itself on untouched buffers: what it does not serve is FSV_ERR_UNSUPPORTED before any launch, argument errors
    come first"""
    lib = _mod('lib')
    unsup, bad = lib.ENUMS['FSV_ERR_UNSUPPORTED'], lib.ENUMS['FSV_ERR_BAD_ARG']
    bufs = [torch.full((4096,), 7.0, device=device) for _ in range(8)]
    q, k, v0, v1, o0, o1, mass, ws = bufs

    def call(b=1, n=2, p=4, c=8, c0=8, c1=8, q=q, v1=v1, o1=o1, nsplit=1, ws_floats=4096):
        return lib.call_status(ENTRY, lib.ptr(q), lib.ptr(k), lib.ptr(v0), lib.ptr(v1), lib.ptr(o0), lib.ptr(o1), lib.ptr(mass),
                               b, n, p, c, c0, c1, nsplit, lib.ptr(ws), ws_floats, lib.stream_ptr())
    assert call(c=6) == unsup and call(c=260) == unsup
    assert call(c0=6) == unsup and call(c0=260) == unsup and call(c1=10) == unsup and call(c1=260) == unsup
    assert call(q=None) == bad and call(n=0) == bad and call(p=0) == bad
    assert call(q=None, c=6) == bad and call(n=0, c=260) == bad and call(p=0, c=6) == bad            # argument errors first
    assert call(o1=None) == bad and call(c1=0) == bad and call(b=0) == bad and call(c=0) == bad
    assert call(nsplit=9) == bad and call(nsplit=2) == bad          # more ranges than the one tile of 8 keys
    assert call(ws_floats=8) == bad                                 # the masses need 2 * 4 * (1 + 2) floats
    assert call(v1=None, o1=None, c1=0, c0=260) == unsup
    if device.type == 'cuda':
        torch.cuda.synchronize()
    for t in bufs:
        assert float((t - 7.0).abs().max()) == 0.0
    import ctypes
    out = (ctypes.c_longlong * 2)()
    assert lib.call_status('fsv_attention_fused_plan', 1, 3, 128 * 128, 128, 128, 0, 0, 0, out) == 0
    assert (out[0], out[1]) == (2, 2 * 128 * 128 * (128 + 2))       # two key ranges: 16 MiB of partial sums
    assert lib.call_status('fsv_attention_fused_plan', 1, 3, 128 * 128, 128, 128, 0, 1, 0, out) == 0
    assert out[1] == 2 * 128 * 128 * (128 + 2 + 2 * 3)
    assert lib.call_status('fsv_attention_fused_plan', 1, 3, 128 * 128, 130, 128, 0, 1, 0, out) == unsup
    assert call() == 0                                              # (inside the contract: launched)


# ------------------------------------------------------------------------------------------------ 7: the step level
def check_fixture_step(device, case='face_nshot2'):
    """the reference's n_shot 2 iteration (tests/golden/step_face_nshot2.pt) with the switch on - the D step's generator pass runs
    under no_grad and is fused, the G step keeps the differentiable chain: the comparison and the bars of
    attn_band_checks.check_fixture_step"""
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
    with switched('1'), ab.forced(None), ab.recorded_calls() as calls:
        d = M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
        cut = len(calls)
        _check_grad_norms(model.netD, g['grad_norm_D'], 'netD')
        _check_grad_sketches(model.netD, g['grad_sketch_D'], g['grad_norm_D'], 'netD')
        gl, generated, _ = model(data, save_images=True, mode='generator')
        gl = M.loss_backward(opt, gl, opt_G, 0)
    assert [c[0] for c in calls[:cut]].count(ENTRY) >= 1, 'the D step did not take the fused path'
    assert ENTRY not in [c[0] for c in calls[cut:]], 'the differentiable pass took the fused path'
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


# ------------------------------------------------------------------------------------------------ 8: the session
def check_session(device, name='mul'):
    """inference_session(keep_references=True, fused_attention=True), four frames, two sequences through ONE session, against the
    eager frames of infer_nshot_checks' shared scenario: images, flows and masks within 1e-3 of the output's range (the project's
    output bar), atn_vis within op_checks.REL_TOL, ref_idx equal; on the GPU the steady frame is a replayed capture, one capture in
    all; the session holds no band buffer and no K-major layout of the kept operands"""
    r = nc.scenario(name, device)
    opt = r['opt']
    kw, _ = nc.CONFIGS[name]
    if 'eager2' not in r:
        if name == 'mul':
            nc.check_two_sequences(device)                        # (fills r['eager2'] once, shared with the other session tests)
        else:
            r['eager2'] = nc.run_eager(r['twin'], ic.tiny_sequence(opt, 4, device, nc.SECOND_SEQUENCE_SEED))
    _, model = ic.tiny_setup(device, **kw)
    seq2 = ic.tiny_sequence(opt, 4, device, nc.SECOND_SEQUENCE_SEED)
    with switched(None), ab.forced(None), ab.recorded_calls() as calls, ab.recorded_plans() as plans:
        sess = model.inference_session(warmup=1, keep_references=True, fused_attention=True)
        sess.keep_graph = device.type == 'cuda'
        got = nc.run_session(sess, r['seq'])
        graph, caps = sess._graph, sess.n_captures
        kept = sess._kept
        n_maps = 1 if opt.use_label_ref == 'concat' else 2
        assert kept.ready and kept.key is not None and len(kept.vals) == n_maps
        ptrs = [t.data_ptr() for t in [kept.key] + kept.vals]
        got2 = nc.run_session(sess, seq2)
    names = [c[0] for c in calls]
    # frame 0 and the eager steady frame(s) of both sequences; a replayed frame issues no library call
    assert names.count(ENTRY) >= 3 and not plans, (names.count(ENTRY), plans)
    assert kept.kmat is None and kept.xmats == [] and kept.band is None
    for t in [kept.key] + kept.vals:
        assert t.permute(0, 2, 3, 1).is_contiguous() and getattr(t, '_fsv_frozen', None) is None      # their own NHWC memory, no layout
    assert ptrs == [t.data_ptr() for t in [kept.key] + kept.vals]                                      # refilled in place
    assert sess._graph is graph and sess.n_captures == caps and sess.capture_failures == []
    ic.assert_captured(sess, device)
    worst = 0.0
    for what, eager, have in (('first sequence', r['eager'], got), ('second sequence', r['eager2'], got2)):
        assert len(eager[0]) == len(have[0]) == 4
        for t, (a, b) in enumerate(zip(eager[0], have[0])):
            assert len(a) == len(b) == 6
            for i, (x, y) in enumerate(zip(ic._flat(a[:5]), ic._flat(b[:5]))):
                assert (x is None) == (y is None), (what, t, i)
                if x is None:
                    continue
                assert x.shape == y.shape and bool(torch.isfinite(y).all())
                rel = float((x.double() - y.double()).abs().max() / max(float(x.abs().max()), 1e-12))
                worst = max(worst, rel)
                assert rel <= 1e-3, '%s frame %d output %d: %.3e' % (what, t, i, rel)
            assert torch.equal(eager[1][t], have[1][t]), (what, t)
            op_checks.assert_close('%s frame %d atn_vis' % (what, t), b[5], eager[2][t]['vis64'], op_checks.REL_TOL)
    print('fused kept session (%s) against the eager frames: worst relative difference %.3e' % (name, worst))
    assert ic.same_bits(got[0][1], got2[0][1]), 'the second sequence must differ from the first'
    sess.close()
    assert kept.key is None and '_attn_fused' not in model.netG.__dict__ and '_kept_refs' not in model.netG.__dict__


# ------------------------------------------------------------------------------------------------ 9: the real size (hardware only)
def check_real_size(device):
    """b = 1, n = 3, h = w = 128, c = 128, one value map, under no_grad: the banded code needs two bands and a 2 GiB buffer for it.
    Against float64 on the device in chunks of 8 query rows (as attn_band_checks.check_real_limit) at op_checks.REL_TOL.  What the
    attention allocates - the output, the masses and the split-key workspace: torch.cuda.max_memory_allocated over the call, beyond
    the inputs that were there before - stays under 64 MiB (the attention tensor would be 3 GiB; the float64 chunks of the
    comparison, 384 MiB each, come after the measurement).  One entry-point call: one launch plus the finishing launch."""
    b, n, side, c = 1, 3, 128, 128
    h = w = side
    hw = h * w
    g = torch.Generator().manual_seed(11)
    key = torch.randn(b * n, c, h, w, generator=g).to(device).contiguous(memory_format=torch.channels_last)
    query = torch.randn(b, c, h, w, generator=g).to(device).contiguous(memory_format=torch.channels_last)
    x = torch.randn(b * n, c, h, w, generator=g).to(device).contiguous(memory_format=torch.channels_last)
    net = ab.stub_generator(n, key, query)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with switched('1'), ab.forced(None), torch.no_grad(), ab.recorded_calls() as calls, ab.recorded_plans() as plans:
        out, atn, vis = net.attention_module(x, None, None)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert [cc[0] for cc in calls] == [ENTRY] and not plans, (calls, plans)
    scalars = calls[0][1]
    nsplit = scalars[6]
    assert scalars[:6] == (b, n, hw, c, c, 0) and 1 <= nsplit <= 8, scalars
    print('real size: %d key ranges, %.1f MiB allocated by the call' % (nsplit, peak / 2.0 ** 20))
    assert peak < 64 << 20, peak
    mass = atn.mass
    k = key.double().permute(0, 2, 3, 1).reshape(b, n * hw, c)
    xm = x.double().permute(0, 2, 3, 1).reshape(b, n * hw, c).transpose(1, 2)
    q = query.double().permute(0, 2, 3, 1).reshape(b, hw, c).transpose(1, 2)
    step = 8 * w
    assert b * n * hw * step * 8 <= 1 << 30
    worst = 0.0
    for p0 in range(0, hw, step):
        a = torch.softmax(torch.bmm(k, q[:, :, p0:p0 + step]), dim=1)
        want = torch.bmm(xm, a)                                           # [b, c, step]
        want_mass = a.view(b, n, hw, -1).sum(2)                           # [b, n, step]
        del a
        have = out.permute(0, 2, 3, 1).reshape(b, hw, c)[:, p0:p0 + step].transpose(1, 2)
        worst = max(worst, op_checks.assert_close('real size: out, rows from %d' % (p0 // w), have, want, op_checks.REL_TOL))
        op_checks.assert_close('real size: masses, rows from %d' % (p0 // w), mass.reshape(b, hw, n)[:, p0:p0 + step].transpose(1, 2),
                               want_mass, op_checks.REL_TOL)
        del want, want_mass
    assert torch.equal(vis, mass.permute(0, 3, 1, 2)[-1:, 0:1])
    print('real size: worst relative error of the attended features %.2e' % worst)
