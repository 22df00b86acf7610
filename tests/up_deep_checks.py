"""Checks of the sub-pixel forward of the DEEP conv3x3(nearest_x2(x)) layers (csrc/conv_igemm.hip fsv_conv_up_subpixel_fwd: the four
parity classes as one grouped launch, K split in order, one placed finishing pass), shared by tests/test_up_deep_emu.py (SIMT
emulator) and tests/test_up_deep_gpu.py (hardware).

Shapes are the smallest at which these kernels can go wrong: Cin 512 (the selection's gate), source 4 x 4 with N = 2 and a ragged
N tile (Cout 40), source 5 x 3 (odd extents: a border in every class, rows that wrap inside a 64-pixel tile), Cout 160 (more than
one N tile in every tile shape).

Importing this module lists the two new entry points in the ledger of tests/test_entry_point_coverage.py, the way
tests/attn_half_checks.py does: that file is a yardstick and is not edited, and collection imports every test module before
anything runs."""
import os
from importlib import import_module

import torch
import torch.nn.functional as F

import op_checks as oc
import test_entry_point_coverage as ledger
from op_checks import REL_TOL, _dev, assert_close, pkg

ledger.CHECKED_BY.update({
    'fsv_conv_up_subpixel_fwd': 'up_deep_checks.check_entry',
    'fsv_conv_up_subpixel_plan': ledger.HOST_ONLY,
})

TILES = (0, 1, 2, 4, 9)          # the five shapes of the group dispatch (128x128, 128x64, 128x32, 64x64, 64x128)
GUARD = 256                      # floats behind the output and behind the workspace that no launch may touch
SENTINEL = -12345.0

_refs = {}


def inputs(n, h, w, cin, cout, epilogue, seed=5):
    """(x, w, bias | None, wscale | None, fp64 reference of act(conv3x3(nearest_x2(x)) * wscale + bias)), computed once per case"""
    key = (n, h, w, cin, cout, epilogue, seed)
    if key not in _refs:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(n, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (cin * 9) ** 0.5)
        b = torch.randn(cout, generator=g) if epilogue else None
        ws = torch.tensor([0.75]) if epilogue else None
        ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), wt.double(), None, padding=1)
        if epilogue:
            ref = F.leaky_relu(ref * 0.75 + b.double().view(1, -1, 1, 1), 0.2)
        _refs[key] = (x, wt, b, ws, ref)
    return _refs[key]


def class_weights(ops, conv, wd):
    """the class-major 16-tap layout, built the way ops._up_subpixel_deep_forward builds it without a cache"""
    v = ops._tap_sums(wd, ops._SUBPIXEL_ROWS)
    cls = [(ry, rx) for ry in (0, 1) for rx in (0, 1)]
    khs = [2 * ry + iy for ry, rx in cls for iy in (0, 1) for _ in (0, 1)]
    kws = [2 * rx + ix for ry, rx in cls for _ in (0, 1) for ix in (0, 1)]
    wall, _, ldw = conv.prep_weight(v, 0, conv.Geom(3, 3, 1, 1), khs, kws, None)
    return wall, ldw


def run_entry(device, n, h, w, cin, cout, epilogue, tile, split):
    """one direct call of the entry on a NaN-filled output with guard bands -> (y NCHW-shaped view, plan)"""
    ops, conv = pkg()
    lib = import_module('few-shot-vid2vid_amd.lib')
    x, wt, b, ws, _ = inputs(n, h, w, cin, cout, epilogue)
    xd = conv.to_nhwc(_dev(x, device))
    wall, ldw = class_weights(ops, conv, _dev(wt, device))
    bd, wsd = _dev(b, device), _dev(ws, device)
    ptile, nsplit, need = ops.up_subpixel_plan(n, h, w, cin, cout, tile, split)
    if split > 0:
        assert nsplit == split
    assert need == (4 * nsplit * n * h * w * cout if nsplit > 1 else 0)
    total = n * 4 * h * w * cout
    obuf = torch.full((total + GUARD,), float('nan'), device=device)
    obuf[total:] = SENTINEL
    wbuf = torch.full((need + GUARD,), SENTINEL, device=device)
    act = conv.ACT_LRELU if epilogue else conv.ACT_NONE
    lib.call("fsv_conv_up_subpixel_fwd", lib.ptr(xd), lib.ptr(wall), ldw, lib.ptr(bd), None, lib.ptr(wsd), act, 1.0, lib.ptr(obuf),
             None, n, h, w, cin, cout, 0, lib.ptr(wbuf) if need else None, need, tile, split, lib.stream_ptr())
    assert not bool(torch.isnan(obuf[:total]).any()), 'an output position was not written'
    assert bool((obuf[total:] == SENTINEL).all()), 'the guard band behind the output was written'
    assert bool((wbuf[need:] == SENTINEL).all()), 'the guard band behind the workspace was written'
    y = obuf[:total].view(n, 2 * h, 2 * w, cout).permute(0, 3, 1, 2)
    return y, (ptile, nsplit, need)


def single_gather(device, n, h, w, cin, cout, epilogue):
    """the same layer through the up-sampling index (ConvP::up): one 9-tap gather"""
    ops, conv = pkg()
    x, wt, b, ws, _ = inputs(n, h, w, cin, cout, epilogue)
    geom = conv.Geom(3, 3, 1, 1)
    w9, _, ldw = conv.prep_weight(_dev(wt, device), 0, geom)
    act = conv.ACT_LRELU if epilogue else conv.ACT_NONE
    return conv.conv_forward(conv.to_nhwc(_dev(x, device)), w9, ldw, cout, geom, bias=_dev(b, device), act=act,
                             wscale=_dev(ws, device), up=True)


def check_entry(device, n, h, w, cin, cout, epilogue, tile, split):
    """Part A checks 1 - 4 for one (shape, epilogue, tile, split)"""
    y, plan = run_entry(device, n, h, w, cin, cout, epilogue, tile, split)
    ref = inputs(n, h, w, cin, cout, epilogue)[4]
    one = single_gather(device, n, h, w, cin, cout, epilogue)
    assert_close('deep sub-pixel forward vs one gather %s' % (plan,), y, one, REL_TOL if epilogue else 2e-6)
    assert_close('deep sub-pixel forward vs fp64 %s' % (plan,), y, ref, REL_TOL)
    again, _ = run_entry(device, n, h, w, cin, cout, epilogue, tile, split)
    assert torch.equal(y, again), 'the same call twice gave different bits %s' % (plan,)
    return y


def check_rejections(device):
    """a residual, a statistics request, per-sample weights and (4 Cin) % 32 != 0 are declined with nothing launched"""
    ops, conv = pkg()
    lib = import_module('few-shot-vid2vid_amd.lib')
    n, h, w, cin, cout = 1, 4, 4, 512, 40
    x, wt, _, _, _ = inputs(n, h, w, cin, cout, False)
    xd = conv.to_nhwc(_dev(x, device))
    wall, ldw = class_weights(ops, conv, _dev(wt, device))
    out = torch.full((n * 4 * h * w * cout,), SENTINEL, device=device)
    other = torch.zeros(n * 4 * h * w * cout, device=device)
    st = torch.zeros(64 * cout * 2, dtype=torch.float64, device=device)
    need = ops.up_subpixel_plan(n, h, w, cin, cout)[2]
    wsb = torch.empty(max(need, 1), device=device)
    uns = lib.ENUMS['FSV_ERR_UNSUPPORTED']

    def go(res=None, stats=None, per_sample=0, cin_arg=cin):
        return lib.call_status("fsv_conv_up_subpixel_fwd", lib.ptr(xd), lib.ptr(wall), ldw, None, lib.ptr(res), None, conv.ACT_NONE,
                               1.0, lib.ptr(out), lib.ptr(stats), n, h, w, cin_arg, cout, per_sample, lib.ptr(wsb), need, -1, 0,
                               lib.stream_ptr())
    assert go(res=other) == uns
    assert go(stats=st) == uns
    assert go(per_sample=1) == uns
    assert go(cin_arg=4) == uns                      # 16 K-elements per class: not a whole chunk
    assert bool((out == SENTINEL).all())
    assert ops.up_subpixel_plan(n, h, w, 4, cout) is None
    # a split without its workspace is an argument error, not a silent atomic fall-back
    assert lib.call_status("fsv_conv_up_subpixel_fwd", lib.ptr(xd), lib.ptr(wall), ldw, None, None, None, conv.ACT_NONE, 1.0,
                           lib.ptr(out), None, n, h, w, cin, cout, 0, None, 0, -1, 2, lib.stream_ptr()) == lib.ENUMS['FSV_ERR_BAD_ARG']
    assert bool((out == SENTINEL).all())


def conv_up(device, n, cin, h, w, cout, act='lrelu', env=None, res=False, stats=0, cache=None, seed=9):
    """ops.conv2d(..., up=True) forward + backward with the library calls recorded -> (y, dx, dw, db, [(name, args)])"""
    ops, conv = pkg()
    lib = import_module('few-shot-vid2vid_amd.lib')
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (cin * 9) ** 0.5)
    b = torch.randn(cout, generator=g)
    r = torch.randn(n, cout, 2 * h, 2 * w, generator=g) if res else None
    dy = torch.randn(n, cout, 2 * h, 2 * w, generator=g)
    xd, wd, bd = (_dev(t, device).detach().clone().requires_grad_(True) for t in (x, wt, b))
    if cache is not None:
        wd._fsv_cache = cache
    seen, real_call, real_status = [], lib.call, lib.call_status

    def rec_call(name, *a):
        seen.append((name, a))
        return real_call(name, *a)

    def rec_status(name, *a):
        seen.append((name, a))
        return real_status(name, *a)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    lib.call, lib.call_status = rec_call, rec_status
    try:
        with conv.stats_pass(xd.device):
            y = ops.conv2d(xd, wd, bd, stride=1, padding=1, act={'none': conv.ACT_NONE, 'lrelu': conv.ACT_LRELU}[act],
                           res=_dev(r, device), stats_groups=stats, up=True)
        y.backward(_dev(dy, device))
    finally:
        lib.call, lib.call_status = real_call, real_status
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return y.detach(), xd.grad, wd.grad, bd.grad, seen, (x, wt, b, r, dy)


ENTRY = 'fsv_conv_up_subpixel_fwd'


def calls_of(seen, name=ENTRY):
    return [a for s_, a in seen if s_ == name]


def check_backward_undisturbed(device, n=1, cin=512, h=5, w=3, cout=40):
    """Part A check 5: y, dx, dw, db of the layer whose forward takes the new entry, against torch"""
    y, dx, dw, db, seen, (x, wt, b, _, dy) = conv_up(device, n, cin, h, w, cout, act='lrelu')
    assert len(calls_of(seen)) == 1
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, wt, b))
    ref = oc.O.actvn(F.conv2d(F.interpolate(xr, scale_factor=2, mode='nearest'), wr, br, padding=1))
    ref.backward(dy)
    for name, got, want in (('y', y, ref), ('dx', dx, xr.grad), ('dw', dw, wr.grad), ('db', db, br.grad)):
        assert_close('deep conv(up2x) %s' % name, got, want, REL_TOL)


def check_selection(device):
    """Part A check 6: which layers take the entry, and with what workspace"""
    ops, _ = pkg()
    n, h, w, cout = 1, 4, 4, 40
    seen = conv_up(device, n, 512, h, w, cout)[4]
    took = calls_of(seen)
    assert len(took) == 1, [s_ for s_, _ in seen]
    # workspace_floats (argument 17) is what the plan query answers for this shape
    assert took[0][17] == ops.up_subpixel_plan(n, h, w, 512, cout)[2]
    assert (took[0][16] is None) == (took[0][17] == 0)
    assert not calls_of(conv_up(device, n, 256, h, w, cout)[4]), 'Cin 256 must stay on the single gather'
    assert not calls_of(conv_up(device, n, 512, h, w, cout, env={'FSV_UP_SUBPIXEL': '0'})[4])
    assert not calls_of(conv_up(device, n, 512, h, w, cout, act='none', res=True)[4])
    assert not calls_of(conv_up(device, n, 512, h, w, cout, stats=1)[4])


def check_cache_path(device, n=1, cin=512, h=4, w=4, cout=40):
    """Part A check 7: the optimiser-owned layout (LayoutCache: masks applied by the grouped re-arrangement) and the per-call
    construction (0 / 1 product + re-arrangement) give the same result to the rounding of a summed weight"""
    from fsv2v_amd.layout_cache import LayoutCache
    a = conv_up(device, n, cin, h, w, cout)
    c = conv_up(device, n, cin, h, w, cout, cache=LayoutCache())
    assert len(calls_of(a[4])) == 1 and len(calls_of(c[4])) == 1
    assert sum(1 for s_, _ in c[4] if s_ == 'fsv_prep_weight') < sum(1 for s_, _ in a[4] if s_ == 'fsv_prep_weight')
    assert_close('deep conv(up2x) y: layout cache vs per call', c[0], a[0], 1e-6)
