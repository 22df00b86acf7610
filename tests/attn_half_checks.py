"""Shared checks of the streaming few-shot attention on the f16 matrix cores (few-shot-vid2vid_amd/csrc/attention_h.hip,
ops.attention_half_prepare / attention_fused_half, the FSV_ATTN_FUSED_HALF switch of networks.FewShotGenerator.attention_module,
InferenceSession(fused_attention='half')): the prep launch bit for bit, the operator against float64 at a bound derived from the
arithmetic and at the project's output bar, the low parts of the split, key ranges, rescaling, determinism, the untouched default
path, the bounds and the kept session.  Used by tests/test_attn_half_emu.py (emulator) and tests/test_attn_half_gpu.py (hardware).

Importing this module adds the three entry points of attention_h.hip to the C-ABI ledger (test_entry_point_coverage.CHECKED_BY): that
file is a yardstick and is not edited; collection imports every test module before anything runs, so the ledger is complete
whenever the suite runs (run on its own, the ledger module reports the three names as unlisted)."""
import contextlib
import ctypes
import os

import torch

import attn_band_checks as ab
import attn_fused_checks as af
import infer_nshot_checks as nc
import infer_session_checks as ic
import op_checks
import test_entry_point_coverage as ledger

ledger.CHECKED_BY.update({
    'fsv_attention_half_prep': 'attn_half_checks.check_prep',
    'fsv_attention_fused_fwd_h': 'attn_half_checks.check_splits',
    'fsv_attention_fused_h_plan': ledger.HOST_ONLY,
})

_mod = ic._mod
U = ab.U
SWITCH = 'FSV_ATTN_FUSED_HALF'
PREP, ENTRY = 'fsv_attention_half_prep', 'fsv_attention_fused_fwd_h'

# (b, n, c, c0, c1, h, w): the smallest shapes at which this kernel can go wrong.
# small: P = 30 is below one key tile, reference boundaries fall inside key tiles, C = 8 is half of one 16-channel MFMA step.
# c24: one and a half channel steps.  ragged: 99 queries, 198 keys, a partial 32-channel output tile in the second map.
# prod: the production channel counts, both maps in one walk.
SHAPES = {'small': (2, 3, 8, 8, 16, 6, 5), 'c24': (1, 2, 24, 24, 8, 5, 7), 'ragged': (1, 2, 32, 32, 40, 9, 11),
          'prod': (1, 2, 128, 128, 128, 8, 9)}
# seeds for which the precondition of bar (b) holds and the references do not tie (both asserted in float64 by reference())
SEEDS = {'small': 35, 'c24': 30, 'ragged': 30, 'prod': 30}


@contextlib.contextmanager
def switched(value, fused=None):
    """FSV_ATTN_FUSED_HALF = value, FSV_ATTN_FUSED = fused (None: unset) for the block; both are read per call"""
    old = {k: os.environ.pop(k, None) for k in (SWITCH, af.SWITCH)}
    for k, v in ((SWITCH, value), (af.SWITCH, fused)):
        if v is not None:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def h16(t):
    """round-to-nearest-even to IEEE half, as a tensor of t's dtype"""
    return t.float().half().to(t.dtype)


def inputs(case):
    """key, query, image features, label features (fp32)"""
    b, n, c, c0, c1, h, w = SHAPES[case]
    g = torch.Generator().manual_seed(SEEDS[case])
    return [torch.randn(b * n, c, h, w, generator=g), torch.randn(b, c, h, w, generator=g),
            torch.randn(b * n, c0, h, w, generator=g), torch.randn(b * n, c1, h, w, generator=g)]


def analyse(ts, n, tie_check=True):
    """float64 on the fp32 inputs ts = [key, query, v, vl or None], computed on the host:
    ref_a / bound: the attention on q, k and vhat = h(v), and the bound (a) per output element.  With A = sum_c |q_c| |k_c| per
    (key, query), eps = max_key (3 2^-22 + 3 c 2^-24) A + c 2^-36, p = exp(e - max e), S = sum p |vhat| / sum p:
        |o - ref_a| <= [2 (exp(2 eps) - 1) + 2^-11 + n hw 2^-24] S + 2^-25 sum_key |vhat| / sum p
    (the split's truncation plus worst-case fp32 accumulation, moved through the softmax; the rounding of p; the fp32 accumulation
    of the value product; half's subnormal spacing for probabilities that fall below it).
    ref_b: the attention on the unrounded inputs; S: as above, per element (the precondition of bar (b)).  mass [b, hw, n], idx,
    vis as attn_band_checks.attention_ref gives them."""
    key, query = ts[0].double(), ts[1].double()
    b, c, h, w = query.shape
    hw = h * w
    k = key.view(b, n, c, hw).permute(0, 1, 3, 2).reshape(b, n * hw, c)
    q = query.view(b, c, hw)
    e = torch.bmm(k, q)                                                    # [b, n hw, hw]
    A = torch.bmm(k.abs(), q.abs())
    eps = ((3 * 2.0 ** -22 + 3 * c * 2.0 ** -24) * A).max(dim=1)[0] + c * 2.0 ** -36          # [b, hw]
    pe = torch.exp(e - e.max(dim=1, keepdim=True)[0])
    l = pe.sum(1)                                                          # [b, hw], >= 1
    a = pe / l.unsqueeze(1)
    res = dict(eps=eps, A=A, e=e)
    for name, v in (('out', ts[2]), ('outl', ts[3])):
        if v is None:
            continue
        cv = v.shape[1]

        def mat(t):
            return t.double().view(b, n, cv, hw).permute(0, 2, 1, 3).reshape(b, cv, n * hw)
        vhat = mat(h16(v))
        S = torch.bmm(vhat.abs(), a)                                       # [b, cv, hw]
        T = 2.0 ** -25 * vhat.abs().sum(2, keepdim=True) / l.unsqueeze(1)
        bound = (2 * torch.expm1(2 * eps).unsqueeze(1) + 2.0 ** -11 + n * hw * U) * S + T
        res[name] = dict(ref_a=torch.bmm(vhat, a).view(b, cv, h, w), bound=bound.view(b, cv, h, w),
                         ref_b=torch.bmm(mat(v), a).view(b, cv, h, w), S=S.view(b, cv, h, w))
    mass = a.view(b, n, hw, hw).sum(2).permute(0, 2, 1)                    # [b, hw, n]
    per_ref = a.view(b, n, -1).sum(2)
    if tie_check:
        top = torch.sort(per_ref, dim=1, descending=True)[0]
        assert float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()) > 1e-3, 'the references tie: choose another seed'
    res.update(mass=mass, idx=torch.argmax(per_ref, dim=1), vis=a.view(b, n, hw, hw).sum(2).view(b, n, h, w)[-1:, 0:1])
    return res


_refs = {}


def reference(case):
    """computed once per case, shared, never written"""
    if case not in _refs:
        _refs[case] = analyse(inputs(case), SHAPES[case][1])
    return _refs[case]


def assert_bound_a(what, got, r):
    """bar (a): |o - ref_a| <= bound, per element; -> the worst ratio"""
    d = (got.double().cpu() - r['ref_a']).abs()
    ratio = float((d / r['bound']).max())
    print('%s: worst |o - ref| / bound (a) %.3e (bound %.2e ... %.2e)' % (what, ratio, float(r['bound'].min()), float(r['bound'].max())))
    assert bool(torch.isfinite(got).all()), what
    assert bool((d <= r['bound']).all()), (what, ratio)
    return ratio


def assert_bar_b(what, got, r):
    """bar (b): the project's output bar against float64 on the UNROUNDED inputs.  v's rounding adds at most 2^-11 S to bound (a),
    so the total is 2^-10 S plus the small terms: below REL_TOL of the output's range whenever S <= max |o|.  S >= |o| holds
    element by element, so max S <= max |o| can only hold with equality; the precondition is asserted with the slack 2^-10 leaves
    under 1e-3: 2^-10 max S <= REL_TOL max |o|, S <= 1.024 max |o|.  (The energy term of bound (a) is a worst case of the fp32
    accumulation and is not part of the precondition.)  It is a property of the inputs; a failure of the bar is then the
    kernel's."""
    top = float(r['ref_b'].abs().max())
    assert 2.0 ** -10 * float(r['S'].max()) <= op_checks.REL_TOL * top, \
        ('%s: the inputs miss the precondition of bar (b): choose another seed' % what, float(r['S'].max()), top)
    return op_checks.assert_close(what, got, r['ref_b'], op_checks.REL_TOL)


def run(device, ts, n, second, half=True, fused=None, train=False, grad=False):
    """the product's attention the way reference_encoding calls it; second: 'announced' / 'unannounced' / 'absent'"""
    key, query, x, xl = [t.to(device) if t is not None else None for t in ts]
    net = ab.stub_generator(n, key, query)
    net.train(train)
    with switched('1' if half else None, fused), ab.forced(None), torch.set_grad_enabled(grad), ab.recorded_calls() as calls:
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


def assert_half(device, ts, n, second, r, what, bar_b=True):
    """the bars of check 2 on one input set"""
    net = _mod('networks')
    b, hw = ts[1].shape[0], ts[1].shape[2] * ts[1].shape[3]
    got = run(device, ts, n, second)
    assert isinstance(got['atn'], net.AttentionFusedHalf), type(got['atn'])
    names = [c[0] for c in got['calls']]
    assert names == [PREP, ENTRY] * (2 if second == 'unannounced' else 1), names
    for k in ('out', 'outl'):
        if got[k] is None:
            continue
        assert tuple(got[k].shape) == tuple(r[k]['ref_a'].shape), (what, k)
        assert_bound_a('%s: %s' % (what, k), got[k], r[k])
        if bar_b:
            assert_bar_b('%s: %s' % (what, k), got[k], r[k])
    assert torch.equal(got['idx'].cpu(), r['idx']), (what, got['idx'], r['idx'])
    m = got['atn'].mass.double().cpu().reshape(r['mass'].shape)
    assert bool(torch.isfinite(m).all())
    assert float((m - r['mass']).abs().max()) <= op_checks.REL_TOL * float(r['mass'].max()), what
    assert float((m.sum(-1) - 1).abs().max()) <= n * hw * U, what
    op_checks.assert_close('%s: atn_vis' % what, got['vis'], r['vis'], op_checks.REL_TOL)
    return got


# ------------------------------------------------------------------------------------------------ 1: the prep launch
def check_prep(device):
    """kh, kl, v0t, v1t against torch on the host, bit for bit: x.half(), ((x - xh.float()) * 2048).half(), the transposed
    arrangement; the padding to NPs is zero"""
    ops = _mod('ops')
    for case in ('small', 'ragged'):
        b, n, c, c0, c1, h, w = SHAPES[case]
        key, _, x, xl = inputs(case)
        hw = h * w
        pr = ops.attention_half_prepare(key.to(device), [x.to(device), xl.to(device)], n)
        nps = (n * hw + 31) // 32 * 32
        assert (pr.b, pr.n, pr.p, pr.c, pr.cvs, pr.nps) == (b, n, hw, c, [c0, c1], nps)
        assert pr.kh.dtype == pr.kl.dtype == torch.float16 and all(v.dtype == torch.float16 for v in pr.vts)
        k = key.view(b, n, c, hw).permute(0, 1, 3, 2).reshape(b, n * hw, c)
        kh = k.half()
        kl = ((k - kh.float()) * 2048).half()
        pad = torch.zeros(b, nps - n * hw, c, dtype=torch.float16)
        assert torch.equal(pr.kh.cpu(), torch.cat([kh, pad], 1)), case
        assert torch.equal(pr.kl.cpu(), torch.cat([kl, pad], 1)), case
        assert float(kl.float().abs().max()) > 0.0
        for v, vt, cv in ((x, pr.vts[0], c0), (xl, pr.vts[1], c1)):
            want = v.view(b, n, cv, hw).permute(0, 2, 1, 3).reshape(b, cv, n * hw).half()
            want = torch.cat([want, torch.zeros(b, cv, nps - n * hw, dtype=torch.float16)], 2)
            assert tuple(vt.shape) == (b, cv, nps) and torch.equal(vt.cpu(), want), case
        one = ops.attention_half_prepare(key.to(device), [x.to(device)], n)              # v1 is nullable
        assert len(one.vts) == 1 and torch.equal(one.vts[0], pr.vts[0]) and torch.equal(one.kl, pr.kl)


# ------------------------------------------------------------------------------------------------ 2: the operator
def check_operator(device, case, second='announced'):
    """every shape through attention_module with the switch on and the stub generator in eval(), against float64 at bars (a), (b);
    ref_idx, the masses, the recorded library calls; not the bits of the fp32 streaming kernel"""
    b, n, c, c0, c1, h, w = SHAPES[case]
    ts = inputs(case)
    if second == 'absent':
        ts = ts[:3] + [None]
    got = assert_half(device, ts, n, second, reference(case), '%s, second map %s' % (case, second))
    fp32 = run(device, ts, n, second, half=False, fused='1')
    assert isinstance(fp32['atn'], _mod('networks').AttentionFused) and af.ENTRY in [cc[0] for cc in fp32['calls']]
    assert not torch.equal(got['out'], fp32['out']), 'the half kernel did not run'


# ------------------------------------------------------------------------------------------------ 3: the low parts
OFFSET, SPREAD, OFFSET_SEED = 30.0, 2.0 ** -7, 42


def offset_inputs():
    """small's geometry at c = 8, every channel of q and k with a common offset of 30: A is about 7000.  The deviations are randn
    for q and randn / 128 for k: e[key] - mean is 30 sum_c k'_c to first order, so a full randn on k would spread a query's
    energies by ~85 and leave one key with all the mass whatever the energy error; at 1 / 128 the top energies of a query lie within
    about 0.5 of each other and an energy error of that size shows in the output"""
    b, n, _, _, _, h, w = SHAPES['small']
    c = 8
    g = torch.Generator().manual_seed(OFFSET_SEED)
    return [OFFSET + SPREAD * torch.randn(b * n, c, h, w, generator=g), OFFSET + torch.randn(b, c, h, w, generator=g),
            torch.randn(b * n, c, h, w, generator=g), torch.randn(b * n, 16, h, w, generator=g)]


def check_offset(device):
    """the split form meets bound (a) where single half energies, whose error is larger by about two orders (2^-11 A against
    2e-6 A), miss it: the
    properties of the inputs and the miss of the single-half form are asserted in float64 on the host, then the kernel is held
    to the bound"""
    n = SHAPES['small'][1]
    ts = offset_inputs()
    r = analyse(ts, n)
    A, e = r['A'], r['e']
    assert 6000.0 < float(A.min()) and float(A.max()) < 9000.0, (float(A.min()), float(A.max()))
    top = torch.sort(e, dim=1, descending=True)[0]
    gap = float((top[:, 0] - top[:, 1]).max())
    assert gap <= 0.5, gap                                   # every query: the two largest energies within 0.5
    # what single half energies would give, in float64: e1 = <h(k), h(q)>
    b, c, h, w = ts[1].shape
    hw = h * w
    kh = h16(ts[0]).double().view(b, n, c, hw).permute(0, 1, 3, 2).reshape(b, n * hw, c)
    a1 = torch.softmax(torch.bmm(kh, h16(ts[1]).double().view(b, c, hw)), dim=1)
    vhat = h16(ts[2]).double().view(b, n, c, hw).permute(0, 2, 1, 3).reshape(b, c, n * hw)
    miss = float(((torch.bmm(vhat, a1).view(b, c, h, w) - r['out']['ref_a']).abs() / r['out']['bound']).max())
    print('offset %g: A %.0f ... %.0f, top-two gap at most %.3f, single half energies miss bound (a) by %.1fx'
          % (OFFSET, float(A.min()), float(A.max()), gap, miss))
    assert miss > 1.0, miss                                  # (an energy error of 2^-11 A ~ 3.5 moves the probabilities by O(1))
    assert_half(device, ts, n, 'announced', r, 'offset %g' % OFFSET, bar_b=False)


# ------------------------------------------------------------------------------------------------ 4: key ranges
def check_splits(device):
    """one workgroup walking all keys, two and three ranges combined by the finishing pass - each against bound (a), with and without
    the masses, with one and with two value maps; on the emulator the launch counts: one walk, plus the finishing launch where
    there is something to finish"""
    ops, lib = _mod('ops'), _mod('lib')

    def launches():
        return int(lib.get_lib().fsv_emu_launch_count()) if lib.is_emu() else 0
    for case in ('small', 'ragged'):
        b, n, c, c0, c1, h, w = SHAPES[case]
        r = reference(case)
        key, query, x, xl = [t.to(device) for t in inputs(case)]
        with torch.no_grad():
            prepared = {2: ops.attention_half_prepare(key, [x, xl], n), 1: ops.attention_half_prepare(key, [x], n)}
            for split in (1, 2, 3):
                for maps, want_mass in ((2, True), (1, True), (1, False)):
                    n0 = launches()
                    outs, mass = ops.attention_fused_half(query, prepared[maps], want_mass=want_mass, split=split)
                    assert len(outs) == maps and (mass is not None) == want_mass
                    if lib.is_emu():
                        assert launches() - n0 == (2 if (split > 1 or want_mass) else 1)
                    for o, k in zip(outs, ('out', 'outl')):
                        assert_bound_a('%s split %d maps %d: %s' % (case, split, maps, k), o, r[k])
                    if want_mass:
                        m = mass.double().cpu().reshape(r['mass'].shape)
                        assert float((m - r['mass']).abs().max()) <= op_checks.REL_TOL * float(r['mass'].max())
                        assert float((m.sum(-1) - 1).abs().max()) <= n * h * w * U


# ------------------------------------------------------------------------------------------------ 5: rescaling
def check_rescale(device, placement):
    """the two placements of attn_fused_checks.rescale_inputs (energies in the hundreds, the dominant key first or last) at c = 8,
    against bound (a); every output finite (the second map of those inputs has 12 channels: its first 8 are taken)"""
    key, query, x, xl = af.rescale_inputs(placement)
    ts = [key, query, x, xl[:, :8].contiguous()]
    r = analyse(ts, ab.N)
    assert float(r['e'].max()) > 200.0
    got = assert_half(device, ts, ab.N, 'announced', r, 'energies in the hundreds, maximum %s' % placement, bar_b=False)
    assert all(bool(torch.isfinite(got[k]).all()) for k in ('out', 'outl', 'vis'))


# ------------------------------------------------------------------------------------------------ 6: determinism
def check_determinism(device):
    ops = _mod('ops')
    old = os.environ.pop('FSV_DETERMINISTIC', None)
    try:
        for case in ('small', 'prod'):
            key, query, x, xl = [t.to(device) for t in inputs(case)]
            res = []
            for det in (None, '1'):
                os.environ.pop('FSV_DETERMINISTIC', None)
                if det is not None:
                    os.environ['FSV_DETERMINISTIC'] = det
                with torch.no_grad():
                    outs, mass = ops.attention_fused_half(query, ops.attention_half_prepare(key, [x, xl], SHAPES[case][1]))
                res.append(outs + [mass])
            for a, b in zip(*res):
                assert torch.equal(a, b), case
    finally:
        os.environ.pop('FSV_DETERMINISTIC', None)
        if old is not None:
            os.environ['FSV_DETERMINISTIC'] = old


# ------------------------------------------------------------------------------------------------ 7: the default path
def check_default_path(device):
    """switch unset: the launches and bits of attention_module are today's (attn_fused_checks.check_default_path).  Switch set: a
    generator in train(), a pass with autograd on and an unserved shape (c = 12, c = 160) run exactly today's kinds - the recorded
    calls and the bits of the same pass with the switch unset; FSV_ATTN_FUSED keeps its meaning next to it"""
    net = _mod('networks')
    with switched(None):
        af.check_default_path(device)
    ts = inputs('small')
    n = SHAPES['small'][1]

    def same(a, b, what):
        assert a['calls'] == b['calls'], (what, a['calls'], b['calls'])
        assert type(a['atn']) is type(b['atn']) and not isinstance(a['atn'], net.AttentionFusedHalf), what
        assert not ic.same_bits([a['out'].detach(), a['outl'].detach(), a['vis'].detach()],
                                [b['out'].detach(), b['outl'].detach(), b['vis'].detach()]), what
    for fused in (None, '1'):
        for kw in (dict(train=True), dict(grad=True)):
            same(run(device, ts, n, 'announced', half=True, fused=fused, **kw),
                 run(device, ts, n, 'announced', half=False, fused=fused, **kw), (fused, kw))
        for c in (12, 160):
            g = torch.Generator().manual_seed(50 + c)
            odd = [torch.randn(1 * 2, c, 5, 4, generator=g), torch.randn(1, c, 5, 4, generator=g),
                   torch.randn(1 * 2, c, 5, 4, generator=g), torch.randn(1 * 2, 8, 5, 4, generator=g)]
            assert not _mod('ops').attention_fused_half_serves(1, 2, 20, c, [c, 8])
            same(run(device, odd, 2, 'announced', half=True, fused=fused), run(device, odd, 2, 'announced', half=False, fused=fused),
                 (fused, c))
    # both switches, a served shape: half wins; the fp32 switch alone still means the fp32 streaming kernel
    both = run(device, ts, n, 'announced', half=True, fused='1')
    assert isinstance(both['atn'], net.AttentionFusedHalf) and [c[0] for c in both['calls']] == [PREP, ENTRY]
    alone = run(device, ts, n, 'announced', half=False, fused='1')
    assert isinstance(alone['atn'], net.AttentionFused) and [c[0] for c in alone['calls']] == [af.ENTRY]
    import pytest
    ops = _mod('ops')
    key, query, x, xl = [t.to(device) for t in ts]
    with pytest.raises(ValueError), torch.enable_grad():
        ops.attention_half_prepare(key.clone().requires_grad_(True), [x], n)
    with torch.no_grad():
        pr = ops.attention_half_prepare(key, [x], n)
    with pytest.raises(ValueError), torch.enable_grad():
        ops.attention_fused_half(query.clone().requires_grad_(True), pr)
    assert ops.attention_fused_half_serves(1, 2, 128 * 128, 128, [128, 128]) and ops.attention_fused_half_serves(2, 3, 30, 8, [8])
    assert not ops.attention_fused_half_serves(2, 3, 30, 8, [12]) and not ops.attention_fused_half_serves(2, 3, 30, 136, [8])


# ------------------------------------------------------------------------------------------------ 8: bounds
def check_bounds(device):
    """the entry points themselves on untouched buffers: only status codes of calls that launch nothing (the emulator's launch count
    says so); argument errors come first, then the contract, then nsplit and the workspace"""
    lib = _mod('lib')
    unsup, bad = lib.ENUMS['FSV_ERR_UNSUPPORTED'], lib.ENUMS['FSV_ERR_BAD_ARG']
    bufs = [torch.full((4096,), 7.0, device=device) for _ in range(9)]
    q, kh, kl, v0, v1, o0, o1, mass, ws = bufs

    def fwd(b=1, n=2, p=4, c=8, c0=8, c1=8, q=q, kh=kh, kl=kl, v0=v0, v1=v1, o0=o0, o1=o1, nsplit=1, ws_floats=4096):
        return lib.call_status(ENTRY, lib.ptr(q), lib.ptr(kh), lib.ptr(kl), lib.ptr(v0), lib.ptr(v1), lib.ptr(o0), lib.ptr(o1),
                               lib.ptr(mass), b, n, p, c, c0, c1, nsplit, lib.ptr(ws), ws_floats, lib.stream_ptr())

    def prep(b=1, n=2, p=4, c=8, c0=8, c1=8, k=q, v0=v0, v1=v1, kh=kh, kl=kl, v0t=o0, v1t=o1):
        return lib.call_status(PREP, lib.ptr(k), lib.ptr(v0), lib.ptr(v1), lib.ptr(kh), lib.ptr(kl), lib.ptr(v0t), lib.ptr(v1t),
                               b, n, p, c, c0, c1, lib.stream_ptr())
    n0 = int(lib.get_lib().fsv_emu_launch_count()) if lib.is_emu() else 0
    for call in (fwd, prep):
        assert call(c=12) == unsup and call(c=4) == unsup and call(c=136) == unsup
        assert call(c0=12) == unsup and call(c0=136) == unsup and call(c1=4) == unsup and call(c1=136) == unsup
        assert call(b=65536) == unsup
        assert call(n=0) == bad and call(p=0) == bad and call(b=0) == bad and call(c=0) == bad and call(c0=-8) == bad
        assert call(c1=0) == bad and call(kh=None) == bad and call(kl=None) == bad and call(v0=None) == bad
        assert call(n=0, c=12) == bad and call(kh=None, c=136) == bad and call(p=0, c0=12) == bad          # argument errors first
    assert fwd(q=None) == bad and fwd(o0=None) == bad and fwd(o1=None) == bad and fwd(q=None, c=12) == bad
    assert prep(k=None) == bad and prep(v0t=None) == bad and prep(v1t=None) == bad
    assert fwd(nsplit=9) == bad and fwd(nsplit=2) == bad            # more ranges than the one tile of 8 keys
    assert fwd(ws_floats=8) == bad                                  # the masses need 2 * 4 * (1 + 2) floats
    assert fwd(v1=None, o1=None, c1=0, c0=136) == unsup and prep(v1=None, v1t=None, c1=0, c=12) == unsup
    if lib.is_emu():
        assert int(lib.get_lib().fsv_emu_launch_count()) == n0, 'a refused call launched something'
    if device.type == 'cuda':
        torch.cuda.synchronize()
    for t in bufs:
        assert float((t - 7.0).abs().max()) == 0.0
    out = (ctypes.c_longlong * 3)()
    plan = 'fsv_attention_fused_h_plan'
    assert lib.call_status(plan, 1, 3, 128 * 128, 128, 128, 0, 0, 0, out) == 0
    assert (out[0], out[1], out[2]) == (2, 2 * 128 * 128 * (128 + 2), 3 * 128 * 128)   # the fp32 entry point's ranges and workspace
    assert lib.call_status(plan, 1, 3, 128 * 128, 128, 128, 0, 1, 0, out) == 0 and out[1] == 2 * 128 * 128 * (128 + 2 + 2 * 3)
    assert lib.call_status(plan, 2, 3, 30, 8, 8, 16, 1, 1, out) == 0 and (out[0], out[2]) == (1, 96)
    assert lib.call_status(plan, 1, 3, 128 * 128, 132, 128, 0, 1, 0, out) == unsup
    assert lib.call_status(plan, 1, 3, 128 * 128, 128, 128, 0, 1, 9, out) == bad
    assert lib.call_status(plan, 1, 3, 128 * 128, 128, 128, 0, 1, 0, None) == bad


# ------------------------------------------------------------------------------------------------ 9: the session
IMAGE_TOL = 5e-2       # model_checks.check_amp_step's budget for half-precision operands, of each output's range


def _frames(step, netG, labels):
    """[(outputs, ref_idx, names of the library calls)] of step(label) per frame"""
    res = []
    for lab in labels:
        with ab.recorded_calls() as calls:
            out = ic._keep(step(lab))[0]
        res.append((out, netG._atn[1].clone(), [c[0] for c in calls]))
    return res


def check_session(device, name='mul'):
    """inference_session(keep_references=True, fused_attention='half'), four frames, two sequences through ONE session, on
    infer_nshot_checks' shared scenario.  Bit for bit the eager model.inference() frames under FSV_ATTN_FUSED_HALF=1 (the same
    launches on the same values); ref_idx equal to the fp32 eager run's; images, flows and masks within IMAGE_TOL of each output's
    range of the FP32 eager frames (only the attention is half here); the kept operands are half and refilled in place; the eager
    steady frames issue no prep; on the GPU the steady frame is one replayed capture; close() leaves nothing on the network"""
    r = nc.scenario(name, device)
    opt = r['opt']
    kw, _ = nc.CONFIGS[name]
    if 'eager2' not in r:
        if name == 'mul':
            nc.check_two_sequences(device)                        # (fills r['eager2'] once, shared with the other session tests)
        else:
            r['eager2'] = nc.run_eager(r['twin'], ic.tiny_sequence(opt, 4, device, nc.SECOND_SEQUENCE_SEED))
    seq2 = ic.tiny_sequence(opt, 4, device, nc.SECOND_SEQUENCE_SEED)
    n_maps = 1 if opt.use_label_ref == 'concat' else 2
    # the eager half frames: model.inference() itself with the switch set
    _, plain = ic.tiny_setup(device, **kw)
    eager_half = []
    with switched('1'), ab.forced(None):
        for seq in (r['seq'], seq2):
            labels, rl, ri = seq
            plain.reset_inference()
            eager_half.append(_frames(lambda lab: plain.inference(lab, rl, ri), plain.netG, labels))
            assert all(f[2].count(PREP) == 1 and f[2].count(ENTRY) == 1 and af.ENTRY not in f[2] for f in eager_half[-1]), \
                [f[2] for f in eager_half[-1]]
    # the session
    _, model = ic.tiny_setup(device, **kw)
    netG = model.netG
    with switched(None), ab.forced(None), ab.recorded_plans() as plans:
        sess = model.inference_session(warmup=1, keep_references=True, fused_attention='half')
        sess.keep_graph = device.type == 'cuda'
        got, ptrs = [], []
        for seq in (r['seq'], seq2):
            labels, rl, ri = seq
            sess.reset()
            got.append(_frames(lambda lab: sess(lab, rl, ri), netG, labels))
            kept = sess._kept
            assert kept.ready and kept.half is not None and kept.key is None and kept.kmat is None and kept.band is None
            assert len(kept.half.vts) == n_maps and all(t.dtype == torch.float16 for t in kept.half.tensors())
            ptrs.append([t.data_ptr() for t in kept.half.tensors()])
            if len(got) == 1:
                graph, caps = sess._graph, sess.n_captures
    assert ptrs[0] == ptrs[1], 'the kept operands were not refilled in place'
    assert not plans
    assert sess._graph is graph and sess.n_captures == caps and sess.capture_failures == []
    ic.assert_captured(sess, device)
    worst = 0.0
    for s, (what, eager32) in enumerate((('first sequence', r['eager']), ('second sequence', r['eager2']))):
        assert len(got[s]) == len(eager_half[s]) == len(eager32[0]) == 4
        for t, ((out, ix, names), (want, _, _)) in enumerate(zip(got[s], eager_half[s])):
            # frame 0 is model.inference() itself (one prep); an eager steady frame walks the kept operands: no prep, no fp32 kernel
            assert names.count(PREP) == (1 if t == 0 else 0) and af.ENTRY not in names, (what, t, names)
            # (a replayed frame issues no library call at all; the eager warm-up frame and the captured one issue the frame's calls)
            assert names.count(ENTRY) == (1 if names else 0) and (names or (device.type == 'cuda' and t >= 1)), (what, t, names)
            assert names or s == 1 or t == 3, (what, t)
            bad = ic.same_bits(want, out)
            assert not bad, '%s: frame %d, outputs %s differ from the eager half frames' % (what, t, bad)
            assert torch.equal(ix, eager32[1][t]), (what, t, ix, eager32[1][t])
            ref = eager32[0][t]
            for i, (x, y) in enumerate(zip(ic._flat(ref[:5]), ic._flat(out[:5]))):
                assert (x is None) == (y is None), (what, t, i)
                if x is None:
                    continue
                assert x.shape == y.shape and bool(torch.isfinite(y).all())
                rel = float((x.double() - y.double()).abs().max() / max(float(x.abs().max()), 1e-12))
                worst = max(worst, rel)
                assert rel <= IMAGE_TOL, '%s frame %d output %d: %.3e' % (what, t, i, rel)
            op_checks.assert_close('%s frame %d atn_vis' % (what, t), out[5], eager32[2][t]['vis64'], op_checks.REL_TOL)
    print('half kept session (%s) against the fp32 eager frames: worst relative difference %.3e' % (name, worst))
    assert ic.same_bits(got[0][1][0], got[1][1][0]), 'the second sequence must differ from the first'
    sess.close()
    assert kept.half is None and kept.key is None
    assert not [k for k in ('_attn_half', '_attn_fused', '_kept_refs') if k in netG.__dict__]
    import pytest
    with pytest.raises(ValueError):
        model.inference_session(fused_attention='bf16')
    # without keep_references the prep launch runs per frame (on the GPU: inside the captured graph); the same bits again
    with switched(None), ab.forced(None):
        sess = model.inference_session(warmup=1, fused_attention='half')
        labels, rl, ri = r['seq']
        sess.reset()
        unkept = _frames(lambda lab: sess(lab, rl, ri), netG, labels)
    ic.assert_captured(sess, device)
    for t, ((out, _, names), (want, _, _)) in enumerate(zip(unkept, eager_half[0])):
        assert not names or (names.count(PREP) == 1 and names.count(ENTRY) == 1 and af.ENTRY not in names), (t, names)
        assert not ic.same_bits(want, out), 'unkept half session: frame %d differs from the eager half frames' % t
    sess.close()
    assert not [k for k in ('_attn_half', '_attn_fused', '_kept_refs') if k in netG.__dict__]
