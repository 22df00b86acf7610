"""Shared checks of the differentiable streaming few-shot attention (few-shot-vid2vid_amd/csrc/attention.hip
fsv_attention_fused_fwd_lse, csrc/attention_bwd.hip fsv_attention_fused_bwd, ops.attention_fused_grad, the FSV_ATTN_FUSED_GRAD switch
of networks.FewShotGenerator.attention_module): the forward with statistics against the plain forward bit for bit, the gradients
against the float64 restatement of generator.py:298-316 (attn_band_checks.attention_ref) at the smallest ragged shape and at the
production channel counts, forced key ranges and NULL outputs, energies in the hundreds, determinism, fallback and bounds, the
untouched default path, the step level, the graphed step and - hardware only - the real size.  Used by
tests/test_attn_fused_grad_emu.py (emulator) and tests/test_attn_fused_grad_gpu.py (hardware)."""
import contextlib
import os

import torch

import attn_band_checks as ab
import attn_fused_checks as af
import infer_nshot_checks as nc
import infer_session_checks as ic
import model_checks as mc
import op_checks

_mod = ic._mod
U = ab.U
SWITCH = 'FSV_ATTN_FUSED_GRAD'
FWD, BWD = 'fsv_attention_fused_fwd_lse', 'fsv_attention_fused_bwd'
NAMES = ('d key', 'd query', 'd image features', 'd label features')


@contextlib.contextmanager
def switched(value):
    """FSV_ATTN_FUSED_GRAD = value (None: unset) for the block; the switch is read per call"""
    old = os.environ.pop(SWITCH, None)
    if value is not None:
        os.environ[SWITCH] = value
    try:
        yield
    finally:
        os.environ.pop(SWITCH, None)
        if old is not None:
            os.environ[SWITCH] = old


def cotangents(case):
    """seeded cotangents of the two attended maps"""
    if case == 'small':
        return ab.operator_inputs()[4:]
    b, n, c, c0, c1, h, w = af.SHAPES[case]
    g = torch.Generator().manual_seed(af.SEEDS[case] + 100)
    return [torch.randn(b, c0, h, w, generator=g), torch.randn(b, c1, h, w, generator=g)]


_refs = {}


def reference(case, ts, gs, n):
    """float64 outputs and gradients (key, query, image features, label features) of sum(out g0) + sum(outl g1); computed once per
    input set, shared, never written.  `absent`: the same with the first map alone."""
    if case not in _refs:
        leaves = [t.double().clone().requires_grad_(True) for t in ts]
        out, outl, vis, mass = ab.attention_ref(*leaves, n)
        both = torch.autograd.grad((out * gs[0].double()).sum() + (outl * gs[1].double()).sum(), leaves, retain_graph=True)
        one = torch.autograd.grad((out * gs[0].double()).sum(), leaves[:3])
        e = torch.bmm(leaves[0].detach().view(leaves[1].shape[0], n, leaves[0].shape[1], -1).permute(0, 1, 3, 2)
                      .reshape(leaves[1].shape[0], -1, leaves[0].shape[1]), leaves[1].detach().flatten(2))
        _refs[case] = dict(out=out.detach(), outl=outl.detach(), vis=vis.detach(), idx=torch.argmax(mass.detach(), dim=1),
                           grads=list(both), grads_absent=list(one) + [None], lse=torch.logsumexp(e, dim=1))       # lse [b, hw]
    return _refs[case]


def run_module(device, ts, gs, n, second, switch):
    """the product's attention the way reference_encoding calls it, with autograd; second: 'announced' / 'unannounced' / 'absent';
    switch: the value of FSV_ATTN_FUSED_GRAD (None: today's differentiable chain)"""
    leaves = [t.to(device).clone().requires_grad_(True) for t in ts]
    g0, g1 = [t.to(device) for t in gs]
    net = ab.stub_generator(n, leaves[0], leaves[1])
    with switched(switch), af.switched(None), ab.forced(None), torch.enable_grad(), ab.recorded_calls() as calls:
        if second == 'announced':
            net._atn_second = leaves[3]
        out, atn, vis = net.attention_module(leaves[2], None, None)
        net.__dict__.pop('_atn_second', None)
        outl = None
        loss = (out * g0).sum()
        if second != 'absent':
            outl, atn2, vis2 = net.attention_module(leaves[3], None, None, atn)
            assert atn2 is atn and torch.equal(vis, vis2)
            loss = loss + (outl * g1).sum()
        if torch.is_tensor(atn):
            idx = torch.argmax(atn.reshape(leaves[1].shape[0], n, -1).sum(2), dim=1)
        else:
            idx = atn.ref_idx()
        loss.backward()
    return dict(out=out.detach(), outl=None if outl is None else outl.detach(), vis=vis.detach(), idx=idx, atn=atn, calls=calls,
                grads=[t.grad for t in leaves])


def _err(a, r):
    return float((a.double().cpu() - r).abs().max() / max(float(r.abs().max()), 1e-6))


def errors(got, ref, second):
    """max |difference| to float64 relative to the reference's range, per quantity"""
    e = {}
    for k in ('out', 'outl', 'vis'):
        if got[k] is not None:
            e[k] = _err(got[k], ref[k])
    want = ref['grads_absent'] if second == 'absent' else ref['grads']
    for name, a, r in zip(NAMES, got['grads'], want):
        if r is None:
            assert a is None, name
            continue
        assert a is not None, name
        e[name] = _err(a, r)
    return e


def assert_bars(what, e_f, e_p, n, hw):
    """the bars of the issue: every quantity within op_checks.REL_TOL of float64, and at most the larger of 4x the error of today's
    differentiable chain on the same inputs and n hw 2^-24 of the quantity's range"""
    print('%s: streaming %s, today\'s chain %s (relative to float64)' % (what, {k: '%.1e' % v for k, v in e_f.items()},
                                                                        {k: '%.1e' % v for k, v in e_p.items()}))
    for k in e_f:
        assert e_f[k] <= op_checks.REL_TOL, (what, k, e_f[k])
        assert e_f[k] <= max(4 * e_p[k], n * hw * U), (what, k, e_f[k], e_p[k], n * hw * U)


# ------------------------------------------------------------------------------------------------ 1: the forward with statistics
def check_forward_lse(device, case):
    """fsv_attention_fused_fwd_lse against fsv_attention_fused_fwd on the same arguments: o0 / o1 / mass bit for bit (key ranges 1 / 2 /
    3, one and two maps, with and without the masses), lse within n hw 2^-24 max(1, |lse|) of the float64 log-sum-exp"""
    lib, ops = _mod('lib'), _mod('ops')
    b, n, c, c0, c1, h, w = af.SHAPES[case]
    hw = h * w
    ts = af.inputs(case)
    ref = reference(case, ts, cotangents(case), n)
    key, query, x, xl = [ops.to_nhwc(t.to(device)) for t in ts]
    for split in (1, 2, 3):
        for vals, want_mass in (([x, xl], True), ([x, xl], False), ([x], True), ([x], False)):
            two = len(vals) > 1
            cvs = [v.shape[1] for v in vals]
            nsplit, floats = ops._attention_fused_plan(b, n, hw, c, cvs, want_mass, split)
            assert nsplit == split
            res = []
            for entry in (af.ENTRY, FWD):
                outs = [torch.full((b, h, w, cv), 3.0, device=device).permute(0, 3, 1, 2) for cv in cvs]
                mass = torch.full((b, h, w, n), 3.0, device=device) if want_mass else None
                lse = torch.full((b, hw), 3.0, device=device)
                ws = torch.empty(max(floats, 1), device=device)
                args = [lib.ptr(query), lib.ptr(key), lib.ptr(vals[0]), lib.ptr(vals[1]) if two else None, lib.ptr(outs[0]),
                        lib.ptr(outs[1]) if two else None, lib.ptr(mass)]
                if entry == FWD:
                    args.append(lib.ptr(lse))
                n0 = int(lib.get_lib().fsv_emu_launch_count()) if lib.is_emu() else 0
                assert lib.call_status(entry, *args, b, n, hw, c, cvs[0], cvs[1] if two else 0, split, lib.ptr(ws), floats,
                                       lib.stream_ptr()) == 0
                if lib.is_emu():             # the launch counts of the plain forward
                    assert int(lib.get_lib().fsv_emu_launch_count()) - n0 == (2 if (split > 1 or want_mass) else 1)
                res.append((outs + [mass], lse))
            assert not ic.same_bits(res[0][0], res[1][0]), (case, split, len(vals), want_mass)
            assert float((res[0][1] - 3.0).abs().max()) == 0.0                         # (the plain forward writes no statistics)
            lse = res[1][1].double().cpu()
            bound = n * hw * U * ref['lse'].abs().clamp(min=1.0)
            assert bool(((lse - ref['lse']).abs() <= bound).all()), (case, split, float((lse - ref['lse']).abs().max()))
            for o, k in zip(res[1][0][:len(vals)], ('out', 'outl')):
                op_checks.assert_close('%s split %d: %s' % (case, split, k), o, ref[k], op_checks.REL_TOL)
    # lse == NULL is the plain forward
    outs = [torch.empty((b, h, w, c0), device=device).permute(0, 3, 1, 2)]
    ws = torch.empty(1, device=device)
    assert lib.call_status(FWD, lib.ptr(query), lib.ptr(key), lib.ptr(x), None, lib.ptr(outs[0]), None, None, None, b, n, hw, c, c0, 0,
                           1, lib.ptr(ws), 0, lib.stream_ptr()) == 0
    with torch.no_grad():
        assert torch.equal(outs[0], ops.attention_fused(query, key, [x], n, want_mass=False, split=1)[0][0])


# ------------------------------------------------------------------------------------------------ 2: gradients against float64
def check_gradients(device, case, second):
    """through attention_module with the switch on, then through ops.attention_fused_grad itself (the same bits): outputs, atn_vis and
    the four gradients against float64 at the bars of assert_bars, ref_idx equal; the recorded calls are the new entry points alone"""
    net, ops = _mod('networks'), _mod('ops')
    b, n, c, c0, c1, h, w = af.SHAPES[case]
    hw = h * w
    ts, gs = af.inputs(case), cotangents(case)
    ref = reference(case, ts, gs, n)
    if case == 'small':              # the shared float64 gradients of attn_band_checks answer for the same inputs
        r = ab.operator_reference()
        assert max(float((x - y).abs().max()) for x, y in zip(r['grads'], ref['grads'])) <= 1e-12
    got = run_module(device, ts, gs, n, second, '1')
    plain = run_module(device, ts, gs, n, second, None)
    assert isinstance(got['atn'], net.AttentionFused) and torch.is_tensor(plain['atn'])
    names = [cc[0] for cc in got['calls']]
    twice = 2 if second == 'unannounced' else 1
    assert names == [FWD] * twice + [BWD] * twice, names
    assert BWD not in [cc[0] for cc in plain['calls']] and ab._names(plain['calls'])
    assert torch.equal(got['idx'].cpu(), ref['idx'])
    what = '%s, second map %s' % (case, second)
    for k, v in got.items():
        if k in ('out', 'outl', 'vis') and v is not None:
            assert tuple(v.shape) == tuple(ref[k].shape) and bool(torch.isfinite(v).all()), (what, k)
    assert_bars(what, errors(got, ref, second), errors(plain, ref, second), n, hw)
    # the operator itself
    leaves = [t.to(device).clone().requires_grad_(True) for t in ts]
    key, query, x, xl = leaves
    vals = [x] if second == 'absent' else [x, xl]
    with torch.enable_grad():
        if second == 'unannounced':
            outs = [ops.attention_fused_grad(query, key, [x], n)[0][0], ops.attention_fused_grad(query, key, [xl], n, want_mass=False)[0][0]]
        else:
            outs, mass = ops.attention_fused_grad(query, key, vals, n)
            assert not mass.requires_grad and torch.equal(mass, got['atn'].mass)
        sum((o * g.to(device)).sum() for o, g in zip(outs, gs)).backward()
    assert not ic.same_bits([got['out'], got['outl']] + got['grads'], [outs[0].detach(), outs[1].detach() if len(outs) > 1 else None]
                            + [t.grad for t in leaves])


# ------------------------------------------------------------------------------------------------ 3: forced ranges, NULL outputs
def run_operator(device, ts, gs, n, split, need=(True, True, True, True), two=True):
    """ops.attention_fused_grad with `split` key ranges; need: which of key / query / image features / label features require grad"""
    ops = _mod('ops')
    key, query, x, xl = [t.to(device).clone().requires_grad_(r) for t, r in zip(ts, need)]
    vals = [x, xl] if two else [x]
    with torch.enable_grad():
        outs, mass = ops.attention_fused_grad(query, key, vals, n, split=split)
        sum((o * g.to(device)).sum() for o, g in zip(outs, gs)).backward()
    return dict(out=outs[0].detach(), outl=outs[1].detach() if two else None, vis=None, grads=[key.grad, query.grad, x.grad, xl.grad])


def check_splits(device):
    """1, 2 and 3 key ranges on `small` and `ragged`: each of dq / dk / dv0 / dv1 at the bars of check 2; then the nullable outputs -
    only the values, only the query, only the key requiring grad: what is produced has the bits of the all-outputs call"""
    for case in ('small', 'ragged'):
        b, n, c, c0, c1, h, w = af.SHAPES[case]
        ts, gs = af.inputs(case), cotangents(case)
        ref = reference(case, ts, gs, n)
        e_p = errors(run_module(device, ts, gs, n, 'announced', None), ref, 'announced')
        for split in (1, 2, 3):
            full = run_operator(device, ts, gs, n, split)
            assert_bars('%s, %d key ranges' % (case, split), errors(full, ref, 'announced'), e_p, n, h * w)
            for need in ((False, False, True, True), (False, True, False, False), (True, False, False, False),
                         (False, False, False, True)):
                part = run_operator(device, ts, gs, n, split, need)
                for i, r in enumerate(need):
                    assert (part['grads'][i] is not None) == r, (case, split, need, i)
                    if r:
                        assert torch.equal(part['grads'][i], full['grads'][i]), (case, split, need, NAMES[i])
            one = run_operator(device, ts, gs, n, split, two=False)
            assert_bars('%s, %d key ranges, one map' % (case, split), errors(one, ref, 'absent'),
                        errors(run_module(device, ts, gs, n, 'absent', None), ref, 'absent'), n, h * w)


# ------------------------------------------------------------------------------------------------ 4: energies in the hundreds
def check_rescale(device, placement):
    """attn_fused_checks.rescale_inputs (energies past 200: exp overflows without the saved statistics) with seeded cotangents: every
    gradient finite and within op_checks.REL_TOL of float64"""
    ts, gs = af.rescale_inputs(placement), ab.operator_inputs()[4:]
    ref = reference('small:' + placement, ts, gs, ab.N)
    for split in (0, 1):
        got = run_operator(device, ts, gs, ab.N, split)
        for name, a, r in zip(NAMES, got['grads'], ref['grads']):
            assert bool(torch.isfinite(a).all()), (placement, name)
            op_checks.assert_close('maximum %s: %s' % (placement, name), a, r, op_checks.REL_TOL)
        for k in ('out', 'outl'):
            op_checks.assert_close('maximum %s: %s' % (placement, k), got[k], ref[k], op_checks.REL_TOL)


# ------------------------------------------------------------------------------------------------ 5: determinism
def check_determinism(device):
    old = os.environ.pop('FSV_DETERMINISTIC', None)
    try:
        for case in ('small', 'prod'):
            ts, gs = af.inputs(case), cotangents(case)
            res = []
            for det in (None, '1', None):
                if det is None:
                    os.environ.pop('FSV_DETERMINISTIC', None)
                else:
                    os.environ['FSV_DETERMINISTIC'] = det
                got = run_operator(device, ts, gs, af.SHAPES[case][1], 0)
                res.append([got['out'], got['outl']] + got['grads'])
            assert not ic.same_bits(res[0], res[1]) and not ic.same_bits(res[0], res[2]), case
    finally:
        os.environ.pop('FSV_DETERMINISTIC', None)
        if old is not None:
            os.environ['FSV_DETERMINISTIC'] = old


# ------------------------------------------------------------------------------------------------ 6: fallback and bounds
def check_fallback(device):
    """`wide` (c = 160) and c = 6 with the switch on and autograd: today's chain call for call, and correct"""
    ops = _mod('ops')
    g = torch.Generator().manual_seed(9)
    b, n, c, h, w = 2, 3, 6, 6, 5
    c6 = [torch.randn(b * n, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g),
          torch.randn(b * n, c, h, w, generator=g), torch.randn(b * n, c, h, w, generator=g)]
    c6g = [torch.randn(b, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g)]
    af.SHAPES.setdefault('c6', (b, n, c, c, c, h, w))
    for case, ts, gs in (('c6', c6, c6g), ('wide', af.inputs('wide'), cotangents('wide'))):
        n = af.SHAPES[case][1]
        ref = reference('fallback:' + case, ts, gs, n)
        got = run_module(device, ts, gs, n, 'announced', '1')
        plain = run_module(device, ts, gs, n, 'announced', None)
        assert torch.is_tensor(got['atn']) and got['calls'] == plain['calls']
        assert FWD not in [cc[0] for cc in got['calls']] and BWD not in [cc[0] for cc in got['calls']]
        assert ab._names(got['calls'])[:4] == ['fsv_conv_gather_fwd', 'fsv_softmax_rows_fwd', 'fsv_conv_gather_fwd', 'fsv_conv_gather_fwd']
        for k, e in errors(got, ref, 'announced').items():
            assert e <= op_checks.REL_TOL, (case, k, e)
        assert torch.equal(got['idx'].cpu(), ref['idx'])
        key, query, x, xl = [t.to(device) for t in ts]
        assert not ops.attention_fused_grad_supported(query, key, [x, xl], n)
        assert not ops.attention_fused_grad_supported(query, key, [x], n)
    assert ops.attention_fused_supported(query, key, [x, xl], n)             # (wide: the forward alone serves 160 channels)
    sk, sq, sx, sxl = [t.to(device) for t in af.inputs('small')]
    assert ops.attention_fused_grad_supported(sq, sk, [sx], ab.N) and ops.attention_fused_grad_supported(sq, sk, [sx, sxl], ab.N)
    assert not ops.attention_fused_grad_supported(sq, sk, [sx], ab.N - 1)
    assert ops.attention_fused_grad_serves(1, 2, 128 * 128, 128, [128, 128]) and not ops.attention_fused_grad_serves(1, 2, 64, 128, [132])
    import pytest
    with pytest.raises(_mod('lib').FsvError):
        ops.attention_fused_grad(query, key, [x], n)
    with pytest.raises(ValueError), torch.enable_grad():             # the forward-only operator stays forward-only
        ops.attention_fused(sq.clone().requires_grad_(True), sk, [sx], ab.N)
    with switched('2'), torch.enable_grad(), pytest.raises(ValueError):
        ab.stub_generator(ab.N, sk, sq).attention_module(sx, None, None)


def check_bounds(device):
    """fsv_attention_fused_bwd itself on buffers filled with a constant: what it does not serve is FSV_ERR_UNSUPPORTED before any
    launch, argument errors come first, every buffer is untouched; one call inside the contract returns 0"""
    lib = _mod('lib')
    unsup, bad = lib.ENUMS['FSV_ERR_UNSUPPORTED'], lib.ENUMS['FSV_ERR_BAD_ARG']
    bufs = [torch.full((4096,), 7.0, device=device) for _ in range(14)]
    q, k, v0, v1, o0, o1, g0, g1, lse, dq, dk, dv0, dv1, ws = bufs
    keep = dict(q=q, k=k, v0=v0, v1=v1, o0=o0, o1=o1, do0=g0, do1=g1, lse=lse, dq=dq, dk=dk, dv0=dv0, dv1=dv1, ws=ws)

    def call(b=1, n=2, p=4, c=8, c0=8, c1=8, nsplit=1, ws_floats=4096, **kw):
        a = dict(keep, **kw)
        return lib.call_status(BWD, *[lib.ptr(a[x]) for x in ('q', 'k', 'v0', 'v1', 'o0', 'o1', 'do0', 'do1', 'lse', 'dq', 'dk', 'dv0',
                                                              'dv1')], b, n, p, c, c0, c1, nsplit, lib.ptr(a['ws']), ws_floats,
                               lib.stream_ptr())
    assert call(c=6) == unsup and call(c=132) == unsup and call(c=260) == unsup
    assert call(c0=6) == unsup and call(c0=132) == unsup and call(c1=10) == unsup and call(c1=260) == unsup
    for name in ('q', 'k', 'v0', 'o0', 'do0', 'lse', 'o1', 'do1'):
        assert call(**{name: None}) == bad and call(c=6, **{name: None}) == bad, name           # argument errors first
    assert call(b=0) == bad and call(n=0) == bad and call(p=0) == bad and call(c=0) == bad and call(c0=0) == bad and call(c1=0) == bad
    assert call(n=0, c=260) == bad and call(p=0, c=6) == bad and call(b=-1, c0=132) == bad
    assert call(dq=None, dk=None, dv0=None, dv1=None) == bad and call(dq=None, dk=None, dv0=None, dv1=None, c=132) == bad
    assert call(v1=None, o1=None, do1=None) == bad                  # a dv1 without a v1
    assert call(nsplit=9) == bad and call(nsplit=2) == bad          # more ranges than the one tile of 8 keys
    assert call(ws=None) == bad and call(ws_floats=3) == bad        # delta alone is 4 floats
    assert call(v1=None, o1=None, do1=None, dv1=None, c1=0, c0=260) == unsup
    if device.type == 'cuda':
        torch.cuda.synchronize()
    for t in bufs:
        assert float((t - 7.0).abs().max()) == 0.0
    import ctypes
    out = (ctypes.c_longlong * 2)()
    hw = 128 * 128
    assert lib.call_status('fsv_attention_fused_bwd_plan', 1, 2, hw, 128, 128, 128, 0, out) == 0
    assert (out[0], out[1]) == (2, hw + 2 * hw * 128)               # 128 query tiles: two key ranges, 16 MiB of partial dq
    assert lib.call_status('fsv_attention_fused_bwd_plan', 2, 2, hw, 128, 128, 0, 0, out) == 0
    assert (out[0], out[1]) == (1, 2 * hw)
    assert lib.call_status('fsv_attention_fused_bwd_plan', 1, 2, hw, 132, 128, 0, 0, out) == unsup
    assert lib.call_status('fsv_attention_fused_bwd_plan', 1, 2, hw, 128, 128, 0, 0, None) == bad
    assert call() == 0 and call(dq=None, dv1=None) == 0             # (inside the contract: launched)
    if device.type == 'cuda':
        torch.cuda.synchronize()
    for t in (q, k, v0, v1, o0, o1, g0, g1, lse):
        assert float((t - 7.0).abs().max()) == 0.0
    for t, used in ((dq, 4 * 8), (dk, 8 * 8), (dv0, 8 * 8), (dv1, 8 * 8)):
        # nothing past the outputs (their values say nothing: a constant 7 is no log-sum-exp of these energies)
        assert float((t[used:] - 7.0).abs().max()) == 0.0 and bool((t[:used] != 7.0).all())


# ------------------------------------------------------------------------------------------------ 7: the default path
def check_default_path(device):
    """both switches unset: attn_band_checks.check_default_path.  Only FSV_ATTN_FUSED = 1: the autograd pass records the calls of the
    switch-off pass.  FSV_ATTN_FUSED_GRAD = 1 under no_grad: ignored, today's launches."""
    with switched(None), af.switched(None):
        ab.check_default_path(device)
    with ab.forced(None), switched(None):
        with af.switched(None), ab.recorded_calls() as off:
            plain = ab.run_operator(device, True)
        with af.switched('1'), ab.recorded_calls() as on:
            got = ab.run_operator(device, True)
    assert on == off and not [cc for cc in on if cc[0].startswith('fsv_attention_fused')]
    assert not ic.same_bits([plain['out'], plain['outl'], plain['vis']] + plain['grads'], [got['out'], got['outl'], got['vis']] + got['grads'])
    with ab.forced(None), af.switched(None):
        with switched(None), ab.recorded_calls() as off:
            plain = ab.run_operator(device, False)
        with switched('1'), ab.recorded_calls() as on:
            got = ab.run_operator(device, False)
    assert on == off and torch.is_tensor(got['atn'])
    assert not ic.same_bits([plain['out'], plain['outl'], plain['vis']], [got['out'], got['outl'], got['vis']])


# ------------------------------------------------------------------------------------------------ 8: the step level
def check_fixture_step(device, case='face_nshot2'):
    """the reference's n_shot 2 iteration (tests/golden/step_face_nshot2.pt) with BOTH switches on: the comparison and the bars of
    attn_fused_checks.check_fixture_step; the G step's calls hold the new backward entry point and neither step launches anything of
    the attention tensor's size (the attention's gather-GEMMs are the per-sample ones)"""
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
    with switched('1'), af.switched('1'), ab.forced(None), ab.recorded_calls() as calls, ab.recorded_plans() as plans:
        d = M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
        cut = len(calls)
        _check_grad_norms(model.netD, g['grad_norm_D'], 'netD')
        _check_grad_sketches(model.netD, g['grad_sketch_D'], g['grad_norm_D'], 'netD')
        gl, generated, _ = model(data, save_images=True, mode='generator')
        gl = M.loss_backward(opt, gl, opt_G, 0)
    d_names, g_names = [cc[0] for cc in calls[:cut]], [cc[0] for cc in calls[cut:]]
    assert d_names.count(af.ENTRY) >= 1 and FWD not in d_names and BWD not in d_names, 'the D step did not take the forward-only path'
    assert g_names.count(FWD) >= 1 and g_names.count(BWD) == g_names.count(FWD) and af.ENTRY not in g_names
    # no attention-tensor launch in either step: the band planner (the entrance of the dense and the banded chain) was never asked,
    # and no softmax over n hw channels ran
    side = g['size'] >> model.netG.n_downsample_A
    assert not plans, plans
    assert not [cc for cc in calls if cc[0].startswith('fsv_softmax_rows') and opt.n_shot * side * side in cc[1]]
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


def check_tiny_step(device):
    """one D + G step of the `nshot3` tiny configuration through model_checks.check_train_step with the switch on: the comparison,
    the bars and the (shared) oracle of attn_band_checks.check_tiny_step"""
    kw = dict(nc.CONFIGS['nshot3'][0])
    opt = mc.tiny_opt(**kw)
    with switched('1'), af.switched(None), ab.forced(None), ab.recorded_calls() as calls:
        mc.check_train_step(device, opt, b=1)
    names = [cc[0] for cc in calls]
    assert names.count(FWD) >= 1 and names.count(BWD) == names.count(FWD), (names.count(FWD), names.count(BWD))


# ------------------------------------------------------------------------------------------------ 9: the graphed step (hardware)
_graphed = {}


def _graphed_runs(device, iters=5, seed=610):
    """the eager loop and the GraphedIteration loop (two warm-up iterations, one capture, replays) of the tiny `nshot3` configuration
    with the switch on, from the same state; run once, shared by the two checks below"""
    if 'runs' in _graphed:
        return _graphed['runs']
    gs = _mod('graph_step')
    M = mc._model()

    def run(graphed):
        """graph_step_checks._run with the references of n_shot 3"""
        opt = mc.tiny_opt(**dict(nc.CONFIGS['nshot3'][0]))
        model = M.create_model(opt)
        mc.fill_state(model.netG); mc.fill_state(model.netD)
        model = model.to(device).train()
        opt_G, opt_D = model.build_optimizers()
        step = gs.GraphedIteration(model, opt, warmup=2) if graphed else None
        h, w = int(opt.fineSize / opt.aspect_ratio), opt.fineSize
        log = []
        for it in range(iters):
            data = mc.with_n_shot(mc.synth_pose_inputs(1, h, w, seed + it, opt.input_nc), opt.n_shot, 1, h, w, seed + it, opt.input_nc)
            data = [data[0], data[1], [None, None], [None, None], data[2], data[3], None, None, None]
            if graphed:
                d, g, gen, prev = step(data, save_images=True)
            else:
                data = [t.to(device) if torch.is_tensor(t) else t for t in data]
                d = M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
                g, gen, prev = model(data, save_images=True, mode='generator')
                g = M.loss_backward(opt, g, opt_G, 0)
            log.append(dict(d=[float(x.detach()) for x in d], g=[float(x.detach()) for x in g if not isinstance(x, int)],
                            img=gen[0].detach().clone().cpu()))
        return log, opt_G.flat_p.detach().clone().cpu(), opt_D.flat_p.detach().clone().cpu(), step
    with switched('1'), af.switched(None), ab.forced(None):
        with ab.recorded_calls() as calls:
            ref = run(False)
        got = run(True)
    assert iters - 2 >= 3                                          # the capture and at least two replays
    _graphed['runs'] = (ref, got, calls)
    return _graphed['runs']


def check_graphed_capture(device):
    """the capture itself: the eager loop issues the backward entry point, GraphedIteration captures the step with no capture failure
    and replays it as a hipGraph; losses within the bar graph_step_checks holds the graphed loop to on hardware (5e-2 relative: Adam
    turns a rounding-level gradient difference into a +-lr step), the first iteration - before any weight update - within 1e-4"""
    (ref, pG, pD, _), (got, qG, qD, step), calls = _graphed_runs(device)
    assert BWD in [cc[0] for cc in calls] and FWD in [cc[0] for cc in calls]
    assert step.capture_failures == [], step.capture_failures
    assert len(step.entries) == 1
    if device.type == 'cuda':
        assert step.launch_mode() == 'hipgraph' and any(e.graphs is not None for e in step.entries.values()), step.launch_mode()
    for it, (a, b) in enumerate(zip(ref, got)):
        for x, y in zip(a['d'] + a['g'], b['d'] + b['g']):
            assert abs(x - y) <= (1e-4 if it == 0 else 5e-2) * max(abs(x), 1.0), (it, a, b)
    assert float((ref[0]['img'] - got[0]['img']).abs().max()) <= 1e-4


def check_graphed_step(device):
    """the replays against the eager iterations from the same state, bit for bit: losses, images and the weights after the last step.
    Holds in the fixed-order mode (FSV_DETERMINISTIC=1, the tests' fixture) because that mode keeps the weight gradients of
    thin-output layers (Cout <= 4: at this width the first layers of the three-reference encoders) off the vector-ALU kernel that
    adds its pixel chunks atomically (csrc/conv_igemm.hip fsv_conv_wgrad); the attention's own gradients have no atomics at all."""
    (ref, pG, pD, _), (got, qG, qD, step), calls = _graphed_runs(device)
    assert step.capture_failures == [], step.capture_failures
    worst = max(abs(x - y) for a, b in zip(ref, got) for x, y in zip(a['d'] + a['g'], b['d'] + b['g']))
    print('graphed against eager: losses differ by at most %.3e, generator weights by %.3e, discriminator weights by %.3e'
          % (worst, float((pG - qG).abs().max()), float((pD - qD).abs().max())))
    for it, (a, b) in enumerate(zip(ref, got)):
        assert a['d'] == b['d'] and a['g'] == b['g'], (it, a['d'], b['d'], a['g'], b['g'])
        assert torch.equal(a['img'], b['img']), it
    assert torch.equal(pG, qG) and torch.equal(pD, qD)


# ------------------------------------------------------------------------------------------------ 10: the real size (hardware only)
def check_real_size(device, rows_per_chunk=8):
    """b = 1, n = 2, h = w = 128, c = c0 = 128, one value map: one forward plus one backward through ops.attention_fused_grad.  What
    the two calls allocate beyond the inputs and the cotangent that were there before - outputs, statistics, gradients, workspace:
    torch.cuda.max_memory_allocated - stays under one eighth of the attention tensor's bytes (256 MiB of 2 GiB).  Then, allocated
    after that reading, float64 on the device in chunks of 8 query rows (dk / dv accumulated over the chunks): all four gradients
    within op_checks.REL_TOL."""
    ops = _mod('ops')
    b, n, side, c = 1, 2, 128, 128
    h = w = side
    hw = h * w
    g = torch.Generator().manual_seed(12)

    def cl(t):
        return t.to(device).contiguous(memory_format=torch.channels_last)
    key, query, x = cl(torch.randn(b * n, c, h, w, generator=g)), cl(torch.randn(b, c, h, w, generator=g)), cl(torch.randn(b * n, c, h, w, generator=g))
    key *= 0.25                                   # (energies of a few units: an attention that is neither uniform nor one-hot)
    go = cl(torch.randn(b, c, h, w, generator=g))
    leaves = [t.requires_grad_(True) for t in (key, query, x)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with torch.enable_grad(), ab.recorded_calls() as calls:
        outs, mass = ops.attention_fused_grad(query, key, [x], n)
        (outs[0] * go).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    full = b * n * hw * hw * 4
    print('real size: %.1f MiB allocated by forward + backward, the attention tensor is %.0f MiB' % (peak / 2.0 ** 20, full / 2.0 ** 20))
    assert [cc[0] for cc in calls] == [FWD, BWD], calls
    assert peak < full // 8, (peak, full // 8)
    dk_, dq_, dx_ = [t.grad for t in leaves]
    out = outs[0].detach()
    del outs, mass
    k = key.detach().double().permute(0, 2, 3, 1).reshape(b, n * hw, c)
    xm = x.detach().double().permute(0, 2, 3, 1).reshape(b, n * hw, c)
    q = query.detach().double().permute(0, 2, 3, 1).reshape(b, hw, c)
    gd = go.double().permute(0, 2, 3, 1).reshape(b, hw, c)
    want_dk, want_dv = torch.zeros_like(k), torch.zeros_like(xm)
    want_dq, want_o = torch.empty_like(q), torch.empty_like(q)
    step = rows_per_chunk * w
    assert b * n * hw * step * 8 <= 1 << 30
    for p0 in range(0, hw, step):
        a = torch.softmax(torch.bmm(k, q[:, p0:p0 + step].transpose(1, 2)), dim=1)           # [b, n hw, step]
        o = torch.bmm(a.transpose(1, 2), xm)                                                 # [b, step, c]
        want_o[:, p0:p0 + step] = o
        want_dv += torch.bmm(a, gd[:, p0:p0 + step])
        dp = torch.bmm(xm, gd[:, p0:p0 + step].transpose(1, 2))                              # [b, n hw, step]
        dp -= (o * gd[:, p0:p0 + step]).sum(2).unsqueeze(1)
        dp *= a                                                                              # ds
        del a
        want_dq[:, p0:p0 + step] = torch.bmm(dp.transpose(1, 2), k)
        want_dk += torch.bmm(dp, q[:, p0:p0 + step])
        del dp

    def flat(t):
        return t.permute(0, 2, 3, 1).reshape(t.shape[0] // (n if t.shape[0] == b * n else 1), -1, c)
    worst = {}
    for name, have, want in (('out', out, want_o), ('d key', dk_, want_dk), ('d query', dq_, want_dq), ('d image features', dx_, want_dv)):
        worst[name] = op_checks.assert_close('real size: ' + name, flat(have), want, op_checks.REL_TOL)
    print('real size: relative to float64 %s' % {k_: '%.1e' % v for k_, v in worst.items()})
