"""Checks of the half-precision convolution kernels (csrc/conv_h.hip, few-shot-vid2vid_amd/hconv.py) against their CPU definition
(oracle/np_oracle.py: operands in IEEE half, exact products, fp32 accumulation, one rounding at a half output), parameterised by
device: the emulator tests (test_h_emu.py) and the GPU tests (test_h_gpu.py) share them.  The reference is the definition in
float64 from the half-rounded operands (conv_ref64), so the kernel's fp32 accumulation is the only summation error inside the
tolerance; a half OUTPUT may in addition land on the neighbouring half value when the fp32 sum straddles a rounding boundary,
hence the half-ulp term of the half-output tolerance."""
import ctypes
import functools
import os
import sys

import torch
import torch.nn.functional as F

import op_checks as oc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import np_oracle as NO   # noqa: E402

TOL = 3e-5
HALF_ULP = 2.0 ** -10          # relative spacing of halves: one ulp of a rounded result

GEOMS = [  # n, cin, h, w, cout, k, stride, pad
    (1, 8, 9, 7, 72, 3, 1, 1),
    (2, 16, 11, 13, 136, 3, 2, 1),
    (1, 24, 10, 9, 40, 4, 2, 2),
    (1, 40, 6, 5, 200, 1, 1, 0),
    (2, 64, 8, 8, 64, 3, 1, 1),
    (1, 32, 12, 12, 3, 3, 1, 1),
]
# weight-gradient geometries (output maps large enough for the 64-pixel walk): stride 2 with odd sizes, 4x4 taps, a ragged Cout
WG_GEOMS = [(2, 16, 21, 27, 136, 3, 2, 1), (1, 64, 8, 8, 64, 3, 1, 1), (1, 24, 30, 17, 40, 4, 2, 2), (3, 8, 9, 16, 200, 1, 1, 0)]
BIG_GEOMS = [(2, 64, 64, 64, 128, 3, 1, 1), (2, 128, 32, 32, 256, 3, 2, 1), (1, 256, 16, 16, 512, 4, 2, 1), (2, 512, 16, 16, 64, 1, 1, 0),
             (1, 32, 96, 128, 32, 3, 1, 1)]
FWD_TILES = [(-1, 0), (0, 1), (0, 3), (1, 1), (2, 1), (3, 1), (3, 2), (4, 2), (5, 1), (5, 3), (9, 1), (16, 1), (16, 2), (17, 1), (18, 1), (19, 1),
             (20, 3), (21, 2), (25, 1)]
WGRAD_TILES = [(0, 0), (1, 1), (1, 3), (2, 2), (3, 1), (4, 1), (4, 2), (5, 1), (6, 1), (6, 2)]

# Ragged forward geometries: the smallest shapes at which every forced tile meets a partial pixel tile, a partial channel tile, a K
# tail, taps outside the image and the padding workgroups of the XCD remap (tiles_xy % 8 != 0).
RAGGED_GEOMS = [
    (1, 24, 13, 11, 136, 3, 1, 1),    # M = 143 (odd; 128 + 15; one partial 256-row tile), Cout = 128 + 8, K = 216 = 3 chunks + 24, taps
                                      # straddle chunk boundaries (64 % 24 != 0), at most 6 tiles: every other workgroup is padding
    (3, 8, 9, 10, 72, 4, 2, 2),       # stride 2, 16 taps, K = 128 exactly, every border pixel has taps outside the image, M = 90
    (2, 40, 17, 19, 264, 1, 1, 0),    # K = 40: one partial chunk; M = 646, Cout = 2 x 128 + 8; tiles_xy = 9 / 18 / 33 for 256 / 128 / 64 rows
    (1, 72, 6, 7, 48, 3, 1, 1),       # K = 648 = 11 chunks under splits 1, 2, 3, 5: uneven shares, an empty last split, trips of two and
                                      # of three buffers that end mid-trip; Cout = 48 under 128-wide tiles
]
RAGGED_SPLITS = [(1,), (1,), (1,), (1, 2, 3, 5)]
RAGGED_TILES = [0, 1, 2, 3, 4, 5, 9, 16, 17, 18, 19, 20, 21, 25]
RAGGED_CASES_PER_TILE = 2 * sum(len(sp) for sp in RAGGED_SPLITS)          # half and fp32 output
EPILOGUE_TILES = [19, 20, 18, 25]
PER_SAMPLE_GEOM = (3, 16, 7, 9, 88, 3, 1, 1)                             # 63 pixels per sample
# ragged weight-gradient geometries, all eligible (hconv.wgrad_eligible)
RAGGED_WG_GEOMS = [
    (2, 16, 21, 27, 136, 3, 2, 1),    # 308 pixels (4 chunks + 52), Cout = 128 + 8, stride 2, K = 144
    (1, 24, 30, 17, 40, 4, 2, 2),     # 16 taps, K = 384, Cout = 40, 144 pixels
    (3, 8, 9, 16, 200, 1, 1, 0),      # K = 8, 432 pixels
    (1, 40, 10, 7, 72, 3, 1, 1),      # 70 pixels: one full chunk + 6; K = 360 (no multiple of 64 or 128); 64 / OW + 1 == OH
]
PER_SAMPLE_WG_GEOM = (3, 16, 9, 11, 72, 3, 1, 1)                          # 99 pixels per sample: one chunk + 35
H_TILE_DIMS = {0: (128, 128), 1: (128, 64), 2: (128, 32), 3: (128, 128), 4: (64, 64), 5: (256, 128), 9: (64, 128)}
SENTINEL_H = -777.0               # a half no output takes (|outputs| stay below 100)
SLOPE = float(torch.tensor(0.2, dtype=torch.float32))      # the kernels' `0.2f`
observed = {}                     # (kind, tile, 'half' | 'fp32') -> largest max|error| / max|ref| seen in this process


def _mods():
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.conv'), import_module('few-shot-vid2vid_amd.hconv')


def _h(x):
    return x.to(torch.float16).to(torch.float32)


def _lib():
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    return import_module('few-shot-vid2vid_amd.lib')


def close_half(name, got, want, tol=TOL):
    """got: a half tensor the kernel stored; want: the value before rounding.  Returns max|error| / max|want|."""
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    err = (got - want).abs()
    lim = tol * want.abs().max() + HALF_ULP * want.abs() * 1.01 + 6e-8
    bad = ~(err <= lim)           # (a NaN fails)
    assert not bool(bad.any()), (name, float(err.max()), float(want.abs().max()), int(bad.sum()))
    print('H_HALF %s worst error / limit %.3f' % (name.split(' tile')[0], float((err / lim).max())))
    return float(err.max()) / max(float(want.abs().max()), 1e-6)


def _act64(v, act):
    return v if not act else torch.where(v > 0, v, SLOPE * v)


def conv_ref64(x, w, stride, pad, bias=None, wscale=1.0, scale=1.0, act=0, res=None, aux=None):
    """The definition in the header of csrc/conv_h.hip in float64, from operands that are already rounded to half:
    (acc * wscale + bias) * scale -> act (0 none, 1 LeakyReLU 0.2) -> + res; with `aux` the FSV_ACT_DLRELU form
    v * leaky_relu'(aux) instead of activation and residual.  w [Cout][Cin][k][k], or [N][Cout][Cin][k][k] with bias [N][Cout]
    for per-sample weights."""
    if w.dim() == 5:
        return torch.cat([conv_ref64(x[i:i + 1], w[i], stride, pad, None if bias is None else bias[i], wscale, scale, act,
                                     None if res is None else res[i:i + 1], None if aux is None else aux[i:i + 1])
                          for i in range(w.shape[0])])
    v = F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad) * float(wscale)
    if bias is not None:
        v = v + bias.double().view(1, -1, 1, 1)
    v = v * float(scale)
    if aux is not None:
        return torch.where(aux.double() > 0, v, SLOPE * v)
    v = _act64(v, act)
    return v if res is None else v + res.double()


def wgrad_ref64(x, dy, w_shape, stride, pad):
    """d/dw of sum(conv(x, w) * dy) in float64 (linear in w: taken at w = 0)"""
    w = torch.zeros(w_shape, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, stride=stride, padding=pad).backward(dy.double())
    return w.grad


def dgrad_ref64(x_shape, w, dy, stride, pad):
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, stride=stride, padding=pad).backward(dy.double())
    return x.grad


def _note(kind, tile, half, rel):
    key = (kind, tile, 'half' if half else 'fp32')
    observed[key] = max(observed.get(key, 0.0), rel)
    print('H_ERR %s tile %d %s %.3e' % (kind, tile, key[2], rel))
    return rel


def _compare(name, got, ref64, kind, tile):
    half = got.dtype == torch.float16
    rel = close_half(name, got, ref64) if half else oc.assert_close(name, got, ref64, TOL)
    return _note(kind, tile, half, rel)


class launches:
    """`with launches() as rec:` - rec.log lists (entry point, fsv_status) of every library call issued inside the block, so that a
    check can assert that ITS launch went out and returned FSV_OK (a non-zero status still raises)"""

    def __enter__(self):
        self.L, self.log = _lib(), []
        self.real = self.L.call

        def call(name, *a):
            rc = self.L.call_status(name, *a)
            self.log.append((name, rc))
            if rc != 0:
                raise self.L.FsvError("%s failed with fsv_status %d" % (name, rc))
        self.L.call = call
        return self

    def __exit__(self, et, ev, tb):
        self.L.call = self.real
        return False

    def ok(self, name, times=1):
        return [e for e in self.log if e[0] == name] == [(name, 0)] * times


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class guarded_out:
    """The output of one launch as a view into a larger allocation: one pixel-row of Cout elements in front of it and one behind,
    everything pre-filled with a sentinel (a finite constant for half, NaN for fp32).  intact(): the guards kept their bits (no
    store past a ragged edge - without ever leaving the allocation); filled(): no sentinel is left inside the output."""

    def __init__(self, n, cout, oh, ow, half, device):
        self.half, self.cout, self.numel = half, cout, n * oh * ow * cout
        self.buf = torch.full((self.numel + 2 * cout,), SENTINEL_H if half else float('nan'),
                              dtype=torch.float16 if half else torch.float32, device=device)
        self.out = self.buf[cout:cout + self.numel].view(n, oh, ow, cout).permute(0, 3, 1, 2)
        self.before = self.buf.clone()

    def refill(self):
        self.buf.copy_(self.before)

    def intact(self):
        c = self.cout
        return bool((_bits(self.buf[:c]) == _bits(self.before[:c])).all() and (_bits(self.buf[-c:]) == _bits(self.before[-c:])).all())

    def sentinel(self, t):
        return (t == SENTINEL_H) if self.half else torch.isnan(t)

    def filled(self):
        return not bool(self.sentinel(self.out).any())


def check_forward(device, geom, tile, split, out_half, seed=7000, res_half=None, act=True):
    conv, hc = _mods()
    n, cin, h, w, cout, k, s, p = geom
    g = torch.Generator().manual_seed(seed + tile * 10 + split)
    x = _h(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, k, k, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    geo = conv.Geom(k, k, s, p)
    res = None
    if res_half is not None:
        res = torch.randn((n, cout) + geo.out_hw(h, w), generator=g)
        if res_half:
            res = _h(res)
    ref = conv_ref64(x, _h(wt), s, p, bias=b, act=1 if act else 0, res=res)
    wf, _, ldw = conv.prep_weight(wt.to(device), 0, geo)
    wh, kpad, nrows = hc.prep_weight_h(wf)
    nchunks = (geo.ntaps * cin + 63) // 64
    rd = None if res is None else conv.to_nhwc(res.to(device).to(torch.float16 if res_half else torch.float32))
    y = hc.conv_forward_h(hc.to_half_nhwc(x.to(device)), wh, kpad, nrows, cout, geo, bias=b.to(device),
                          act=conv.ACT_LRELU if act else conv.ACT_NONE, res=rd, out_half=out_half, force_tile=tile,
                          force_split=min(split, nchunks))
    assert y.dtype == (torch.float16 if out_half else torch.float32)
    name = 'h fwd tile %d split %d half %d %s' % (tile, split, out_half, geom)
    _compare(name, y, ref, 'fwd', tile)


def check_wgrad(device, geom, tile, split, seed=8000):
    conv, hc = _mods()
    n, cin, h, w, cout, k, s, p = geom
    g = torch.Generator().manual_seed(seed + tile * 10 + split)
    x = _h(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, k, k, generator=g) * 0.2          # (unused: keeps the draws of x and dy where they were)
    geo = conv.Geom(k, k, s, p)
    oh, ow = geo.out_hw(h, w)
    dy = _h(torch.randn(n, cout, oh, ow, generator=g))
    if not hc.wgrad_eligible(cin, cout, oh, ow):
        return False
    ref = wgrad_ref64(x, dy, wt.shape, s, p)
    dwt = hc.conv_wgrad_h(hc.to_half_nhwc(x.to(device)), hc.to_half_nhwc(dy.to(device)), geo, force_tile=tile, force_split=split)
    dw = conv.unprep_weight_grad(dwt, (cout, cin, k, k), geo)
    _note('wgrad', tile, False, oc.assert_close('h wgrad tile %d split %d %s' % (tile, split, geom), dw, ref, TOL))
    return True


def check_dgrad(device, geom, out_half, seed=9000):
    conv, hc = _mods()
    n, cin, h, w, cout, k, s, p = geom
    if cout % 8:
        return False
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)                     # (unused: keeps the draws of wt and dy where they were)
    wt = torch.randn(cout, cin, k, k, generator=g) * 0.2
    geo = conv.Geom(k, k, s, p)
    dy = _h(torch.randn((n, cout) + geo.out_hw(h, w), generator=g))
    ref = dgrad_ref64(x.shape, _h(wt), dy, s, p)
    layouts = []
    for c in geo.dgrad_classes:
        if not c['khs']:
            layouts.append(None)
            continue
        wd, _, _ = conv.prep_weight(wt.to(device), 1, geo, c['khs'], c['kws'])
        layouts.append(hc.prep_weight_h(wd))
    dx = hc.conv_dgrad_h(hc.to_half_nhwc(dy.to(device)), layouts, geo, (h, w), cin, out_half=out_half)
    name = 'h dgrad half %d %s' % (out_half, geom)
    _compare(name, dx, ref, 'dgrad', -1)
    return True


GROUP_PROBS = [(8, 16, 24, 40), (3, 40, 8, 136), (16, 64, 64, 64), (5, 8, 200, 72)]     # rows, cin, cout


def check_group(device, seed=9500):
    """independent problems of different sizes in ONE grid == the same problems one by one"""
    conv, hc = _mods()
    g = torch.Generator().manual_seed(seed)
    probs = GROUP_PROBS
    singles, outs, refs = [], [], []
    geo = conv.Geom(1, 1, 1, 0)
    with conv.launch_group(True):
        for rows, cin, cout, _ in probs:
            x = _h(torch.randn(1, cin, 1, rows, generator=g))
            wt = torch.randn(cout, cin, 1, 1, generator=g) * 0.3
            b = torch.randn(cout, generator=g)
            refs.append(conv_ref64(x, _h(wt), 1, 0, bias=b, act=1))
            wf, _, _ = conv.prep_weight(wt.to(device), 0, geo)
            wh, kpad, nrows = hc.prep_weight_h(wf)
            outs.append(hc.conv_forward_h(hc.to_half_nhwc(x.to(device)), wh, kpad, nrows, cout, geo, bias=b.to(device),
                                          act=conv.ACT_LRELU, out_half=False))
    for o, r in zip(outs, refs):
        oc.assert_close('h group', o, r, TOL)


def check_stats(device, seed=9700):
    """the epilogue's per-channel sums == sums over the stored (rounded) output"""
    conv, hc = _mods()
    g = torch.Generator().manual_seed(seed)
    n, cin, h, w, cout = 2, 16, 16, 16, 48
    x = _h(torch.randn(n, cin, h, w, generator=g))
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    geo = conv.Geom(3, 3, 1, 1)
    wf, _, _ = conv.prep_weight(wt.to(device), 0, geo)
    wh, kpad, nrows = hc.prep_weight_h(wf)
    for groups in (1, n):
        st = dict(groups=groups)
        with conv.stats_pass(x.device if False else torch.device(device)):
            y = hc.conv_forward_h(hc.to_half_nhwc(x.to(device)), wh, kpad, nrows, cout, geo, out_half=True, stats=st)
        if 'part' not in st:
            continue
        part = st['part'].view(groups, st['slots'], cout, 2).sum(dim=1).cpu()
        yf = y.float().cpu().view(groups, n // groups, cout, h * w)
        s1 = yf.double().sum(dim=(1, 3))
        s2 = (yf.double() ** 2).sum(dim=(1, 3))
        assert float((part[..., 0] - s1).abs().max()) <= 1e-3 * float(s1.abs().max() + 1), (groups, 'sum')
        assert float((part[..., 1] - s2).abs().max()) <= 1e-3 * float(s2.abs().max() + 1), (groups, 'sumsq')


def check_cast(device, seed=9800):
    conv, hc = _mods()
    g = torch.Generator().manual_seed(seed)
    for nelem in (1, 7, 1024, 4099):
        x = torch.randn(nelem, generator=g) * 100
        y = hc.cast(x.to(device), torch.float16)
        assert y.dtype == torch.float16 and bool((y.cpu() == x.to(torch.float16)).all())
        z = hc.cast(y, torch.float32)
        assert bool((z.cpu() == x.to(torch.float16).float()).all())


# ------------------------------------------------------------------------------------------------ ragged shapes, forced tiles
@functools.lru_cache(maxsize=None)
def _problem(geom, seed, per_sample=False):
    """(x rounded to half, weights rounded to half, bias) of one geometry, drawn once per process"""
    n, cin, h, w, cout, k, s, p = geom
    g = torch.Generator().manual_seed(seed)
    x = _h(torch.randn(n, cin, h, w, generator=g))
    wt = _h(torch.randn(*((n,) if per_sample else ()), cout, cin, k, k, generator=g) * 0.2)
    b = torch.randn(*((n,) if per_sample else ()), cout, generator=g)
    return x, wt, b


@functools.lru_cache(maxsize=None)
def _ragged_ref(gi):
    x, wt, b = _problem(RAGGED_GEOMS[gi], 7100 + gi)
    return conv_ref64(x, wt, RAGGED_GEOMS[gi][6], RAGGED_GEOMS[gi][7], bias=b, act=1)


def _operands(device, geom, x, wt):
    """(half NHWC x, N-major half weights, kpad, nrows, Geom, (oh, ow)) on the device"""
    conv, hc = _mods()
    n, cin, h, w, cout, k, s, p = geom
    geo = conv.Geom(k, k, s, p)
    wf, _, _ = conv.prep_weight(wt.to(device), 0, geo)
    wh, kpad, nrows = hc.prep_weight_h(wf)
    return hc.to_half_nhwc(x.to(device)), wh, kpad, nrows, geo, geo.out_hw(h, w)


def _gather(xd, wh, kpad, nrows, cout, ohw, geo, out, **kw):
    """ONE launch of fsv_hconv_gather through hconv.gather_gemm_h into `out`; asserts that it went out and returned FSV_OK"""
    _, hc = _mods()
    with launches() as rec:
        hc.gather_gemm_h(xd, wh, kpad, nrows, cout, ohw[0], ohw[1], geo.ty, geo.tx, geo.stride, geo.stride, out=out, **kw)
    assert rec.ok('fsv_hconv_gather'), rec.log


def _assert_plan(geom, tile, split, per_sample=False):
    conv, hc = _mods()
    n, cin, h, w, cout, k, s, p = geom
    oh, ow = conv.Geom(k, k, s, p).out_hw(h, w)
    nchunks = (k * k * cin + 63) // 64
    want = (tile, max(min(split, nchunks), 1))
    got = hc.planned(oh * ow if per_sample else n * oh * ow, cout, nchunks, n if per_sample else 1, tile, want[1] if split else 0)
    assert got == want, ('plan', geom, got, want)
    return want[1]


def wgrad_eligible(geom):
    """hconv.wgrad_eligible of a geometry tuple: what check_wgrad must return for it"""
    conv, hc = _mods()
    n, cin, h, w, cout, k, s, p = geom
    return hc.wgrad_eligible(cin, cout, *conv.Geom(k, k, s, p).out_hw(h, w))


def check_forward_ragged(device, tile):
    """forced tile `tile` on every RAGGED_GEOMS entry (and every split of RAGGED_SPLITS), half and fp32 output, bias + LeakyReLU,
    against conv_ref64; the plan reports the forced tile and the clamped split, the launch returns FSV_OK, the guard rows around
    the output keep their bits and no sentinel is left inside it.  Returns the number of launches checked."""
    ran = 0
    for gi, geom in enumerate(RAGGED_GEOMS):
        n, cin, h, w, cout, k, s, p = geom
        x, wt, b = _problem(geom, 7100 + gi)
        ref = _ragged_ref(gi)
        xd, wh, kpad, nrows, geo, ohw = _operands(device, geom, x, wt)
        bd = b.to(device)
        for split in RAGGED_SPLITS[gi]:
            nsplit = _assert_plan(geom, tile, split)
            for half in (True, False):
                go = guarded_out(n, cout, ohw[0], ohw[1], half, device)
                _gather(xd, wh, kpad, nrows, cout, ohw, geo, go.out, bias=bd, act=1, force_tile=tile, force_split=nsplit)
                name = 'h ragged tile %d split %d half %d %s' % (tile, split, half, geom)
                assert go.intact(), name + ': a guard row was written'
                assert go.filled(), name + ': output elements were not written'
                _compare(name, go.out, ref, 'fwd', tile)
                ran += 1
    return ran


# ------------------------------------------------------------------------------------------------ epilogue options
def _epi_run(device, tile, geom, seed, ref_kw, dev_kw, per_sample=False, halves=(True, False)):
    """one epilogue configuration on `geom` at forced tile `tile`: ref_kw -> conv_ref64, dev_kw (tensors on the CPU) -> gather_gemm_h"""
    n, cin, h, w, cout, k, s, p = geom
    x, wt, b = _problem(geom, seed, per_sample)
    ref = conv_ref64(x, wt, s, p, **ref_kw(b))
    xd, wh, kpad, nrows, geo, ohw = _operands(device, geom, x, wt)
    _assert_plan(geom, tile, 0, per_sample)
    kw = {k_: (v.to(device) if torch.is_tensor(v) else v) for k_, v in dev_kw(b).items()}
    ran = 0
    for half in halves:
        go = guarded_out(n, cout, ohw[0], ohw[1], half, device)
        _gather(xd, wh, kpad, nrows, cout, ohw, geo, go.out, force_tile=tile, per_sample=per_sample, **kw)
        name = 'h epilogue tile %d half %d %s %s' % (tile, half, sorted(kw), geom)
        assert go.intact(), name + ': a guard row was written'
        assert go.filled(), name + ': output elements were not written'
        _compare(name, go.out, ref, 'epilogue', tile)
        ran += 1
    return ran


def _out_shape(geom):
    conv, _ = _mods()
    n, cin, h, w, cout, k, s, p = geom
    return (n, cout) + conv.Geom(k, k, s, p).out_hw(h, w)


def epi_wscale(device, tile):
    """wscale as a device scalar together with scale = 0.5, bias and LeakyReLU"""
    ws = torch.tensor([0.37])
    return _epi_run(device, tile, RAGGED_GEOMS[0], 7200, lambda b: dict(bias=b, wscale=float(ws), scale=0.5, act=1),
                    lambda b: dict(bias=b, wscale=ws, scale=0.5, act=1))


def _epi_res(device, tile, res_half, act):
    g = torch.Generator().manual_seed(7210 + res_half)
    res = torch.randn(_out_shape(RAGGED_GEOMS[0]), generator=g)
    res = _h(res) if res_half else res
    conv, _ = _mods()
    rd = conv.to_nhwc(res.to(torch.float16 if res_half else torch.float32))
    return _epi_run(device, tile, RAGGED_GEOMS[0], 7201, lambda b: dict(bias=b, act=act, res=res), lambda b: dict(bias=b, act=act, res=rd))


def epi_res_f32(device, tile):
    """fp32 residual behind bias + LeakyReLU, M = 143 odd"""
    return _epi_res(device, tile, False, 1)


def epi_res_half(device, tile):
    """half residual (the lane-pair residual load ends on an odd last pixel), no activation"""
    return _epi_res(device, tile, True, 0)


def _epi_dlrelu(device, tile, aux_half):
    g = torch.Generator().manual_seed(7220 + aux_half)
    aux = torch.randn(_out_shape(RAGGED_GEOMS[0]), generator=g)
    aux = _h(aux) if aux_half else aux
    assert bool((aux > 0).any()) and bool((aux < 0).any())
    conv, _ = _mods()
    ad = conv.to_nhwc(aux.to(torch.float16 if aux_half else torch.float32))
    return _epi_run(device, tile, RAGGED_GEOMS[0], 7202, lambda b: dict(bias=b, aux=aux), lambda b: dict(bias=b, act=conv.ACT_DLRELU, res=ad))


def epi_dlrelu_half(device, tile):
    """FSV_ACT_DLRELU with a half aux tensor of mixed signs"""
    return _epi_dlrelu(device, tile, True)


def epi_dlrelu_f32(device, tile):
    """FSV_ACT_DLRELU with an fp32 aux tensor"""
    return _epi_dlrelu(device, tile, False)


def epi_per_sample(device, tile):
    """per-sample weights and a 2-D per-sample bias whose row stride is not Cout (n = 3, 63 pixels per sample)"""
    n, cout = PER_SAMPLE_GEOM[0], PER_SAMPLE_GEOM[4]
    x, wt, b = _problem(PER_SAMPLE_GEOM, 7203, True)
    ref = conv_ref64(x, wt, 1, 1, bias=b, act=1)
    xd, wh, kpad, nrows, geo, ohw = _operands(device, PER_SAMPLE_GEOM, x, wt)
    assert wh.shape[0] == n
    _assert_plan(PER_SAMPLE_GEOM, tile, 0, True)
    wide = torch.full((n, cout + 5), 1e4)
    wide[:, :cout] = b
    bias = wide.to(device)[:, :cout]          # (sliced on the device: a sliced CPU tensor would arrive dense)
    assert bias.stride(0) == cout + 5 and bias.stride(1) == 1
    ran = 0
    for half in (True, False):
        go = guarded_out(n, cout, ohw[0], ohw[1], half, device)
        _gather(xd, wh, kpad, nrows, cout, ohw, geo, go.out, force_tile=tile, per_sample=True, bias=bias, act=1)
        name = 'h per-sample tile %d half %d' % (tile, half)
        assert go.intact() and go.filled(), name + ': guard rows / unwritten output'
        _compare(name, go.out, ref, 'epilogue', tile)
        ran += 1
    return ran


def epi_placed(device, tile):
    """placed output: the four parity classes of a 2 x 2 grid, one launch each into a sentinel-filled tensor - a class writes
    exactly its own pixels, the other three quarters keep the sentinel"""
    geom = RAGGED_GEOMS[0]
    n, cin, h, w, cout, k, s, p = geom
    x, wt, b = _problem(geom, 7204)
    ref = conv_ref64(x, wt, s, p, bias=b, act=1)
    xd, wh, kpad, nrows, geo, (oh, ow) = _operands(device, geom, x, wt)
    _assert_plan(geom, tile, 0)
    bd = b.to(device)
    ran = 0
    for half in (True, False):
        go = guarded_out(n, cout, 2 * oh, 2 * ow, half, device)
        for py in range(2):
            for px in range(2):
                go.refill()
                _gather(xd, wh, kpad, nrows, cout, (oh, ow), geo, go.out, bias=bd, act=1, force_tile=tile,
                        place=(2 * oh, 2 * ow, 2, 2, py, px))
                name = 'h placed tile %d half %d class (%d, %d)' % (tile, half, py, px)
                assert go.intact(), name + ': a guard row was written'
                out = go.out.cpu()
                for qy in range(2):
                    for qx in range(2):
                        q = out[:, :, qy::2, qx::2]
                        if (qy, qx) == (py, px):
                            assert not bool(go.sentinel(q).any()), name + ': own pixels not written'
                            _compare(name, q, ref, 'epilogue', tile)
                        else:
                            assert bool(go.sentinel(q).all()), name + ': wrote into class (%d, %d)' % (qy, qx)
                ran += 1
    return ran


def make_desc(xd, wh, kpad, nrows, cout, ohw, geo, out, place=None, **fields):
    """an fsv_hconv_desc filled by hand (include/fsv2v.h); tensors among `fields` go in as their addresses"""
    _, hc = _mods()
    d = hc.HConvDesc()
    n, cin, h, w = xd.shape
    d.inp, d.wt, d.out = xd.data_ptr(), wh.data_ptr(), out.data_ptr()
    d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout, d.ntaps = n, h, w, cin, ohw[0], ohw[1], cout, len(geo.ty)
    for i, (a, b) in enumerate(zip(geo.ty, geo.tx)):
        d.ty[i], d.tx[i] = a, b
    d.sy = d.sx = geo.stride
    d.outH, d.outW, d.osy, d.osx, d.ooy, d.oox = place if place is not None else (ohw[0], ohw[1], 1, 1, 0, 0)
    d.Kpad, d.nrows, d.scale, d.force_tile = kpad, nrows, 1.0, -1
    d.out_h = 1 if out.dtype == torch.float16 else 0
    for name, v in fields.items():
        setattr(d, name, v.data_ptr() if torch.is_tensor(v) else v)
    return d


def epi_accumulate(device, tile):
    """accumulate != 0 (fp32 placed output into a zeroed tensor, no bias / residual / activation, scale == 1): two launches add up
    to the sum of their references and touch nothing else; with a bias, a residual, an activation, scale != 1 or a half output the
    call returns FSV_ERR_BAD_ARG and leaves the output alone"""
    L = _lib()
    geom = RAGGED_GEOMS[0]
    n, cin, h, w, cout, k, s, p = geom
    place = None
    refs, descs, keep = [], [], []
    out = None
    for seed in (7205, 7206):
        x, wt, b = _problem(geom, seed)
        refs.append(conv_ref64(x, wt, s, p, wscale=0.37))
        xd, wh, kpad, nrows, geo, (oh, ow) = _operands(device, geom, x, wt)
        if out is None:
            place = (2 * oh, 2 * ow, 2, 2, 1, 0)
            out = torch.zeros((n, 2 * oh, 2 * ow, cout), dtype=torch.float32, device=device).permute(0, 3, 1, 2)
        ws = torch.tensor([0.37], device=device)
        descs.append(make_desc(xd, wh, kpad, nrows, cout, (oh, ow), geo, out, place, accumulate=1, force_tile=tile, wscale=ws))
        keep.append((xd, wh, ws))
    for d in descs:
        assert L.call_status('fsv_hconv_gather', ctypes.byref(d), 1, None, L.stream_ptr()) == L.ENUMS['FSV_OK']
    got = out.cpu()
    name = 'h accumulate tile %d' % tile
    _compare(name, got[:, :, 1::2, 0::2], refs[0] + refs[1], 'epilogue', tile)
    rest = got.clone()
    rest[:, :, 1::2, 0::2] = 0
    assert not bool(rest.any()), name + ': wrote outside its parity class'
    # the combinations the epilogue has no accumulating form for
    xd, wh, ws = keep[0]
    b = torch.randn(cout).to(device)
    res = torch.zeros_like(out)
    before = _bits(out)
    hout = torch.zeros((n, 2 * oh, 2 * ow, cout), dtype=torch.float16, device=device).permute(0, 3, 1, 2)
    bad = [dict(bias=b), dict(res=res), dict(act=1), dict(scale=0.5)]
    ran = 0
    for extra in bad:
        d = make_desc(xd, wh, kpad, nrows, cout, (oh, ow), geo, out, place, accumulate=1, force_tile=tile, **extra)
        assert L.call_status('fsv_hconv_gather', ctypes.byref(d), 1, None, L.stream_ptr()) == L.ENUMS['FSV_ERR_BAD_ARG'], sorted(extra)
        ran += 1
    d = make_desc(xd, wh, kpad, nrows, cout, (oh, ow), geo, hout, place, accumulate=1, force_tile=tile)
    assert d.out_h == 1
    assert L.call_status('fsv_hconv_gather', ctypes.byref(d), 1, None, L.stream_ptr()) == L.ENUMS['FSV_ERR_BAD_ARG'], 'half output'
    ran += 1
    assert bool((_bits(out) == before).all()) and not bool(hout.any()), name + ': a refused call wrote'
    return 2 + ran


EPILOGUE_CASES = {'wscale': (epi_wscale, 2), 'res_f32': (epi_res_f32, 2), 'res_half': (epi_res_half, 2), 'dlrelu_half': (epi_dlrelu_half, 2),
                  'dlrelu_f32': (epi_dlrelu_f32, 2), 'per_sample': (epi_per_sample, 2), 'placed': (epi_placed, 8),
                  'accumulate': (epi_accumulate, 7)}          # name -> (check(device, tile), launches it must count)


def check_epilogue(device, name, tile):
    fn, want = EPILOGUE_CASES[name]
    ran = fn(device, tile)
    assert ran == want, (name, tile, ran, want)


def check_group_forced(device, tile, seed=9500):
    """ONE grouped launch (n > 1) with force_tile in problems[0]: the four problems of check_group and one with M = 143 rows and
    Cout = 136, each against conv_ref64, half and fp32 output, guard rows intact.  Returns the number of problems compared."""
    conv, hc = _mods()
    L = _lib()
    g = torch.Generator().manual_seed(seed)
    geo = conv.Geom(1, 1, 1, 0)
    probs = []
    for rows, cin, cout, _ in GROUP_PROBS + [(143, 24, 136, 0)]:
        x = _h(torch.randn(1, cin, 1, rows, generator=g))
        wt = _h(torch.randn(cout, cin, 1, 1, generator=g) * 0.3)
        b = torch.randn(cout, generator=g)
        probs.append((rows, cin, cout, x, wt, b, conv_ref64(x, wt, 1, 0, bias=b, act=1)))
    ran = 0
    for half in (True, False):
        descs, gos, keep = [], [], []
        for rows, cin, cout, x, wt, b, _ in probs:
            xd, wh, kpad, nrows, _, ohw = _operands(device, (1, cin, 1, rows, cout, 1, 1, 0), x, wt)
            go = guarded_out(1, cout, 1, rows, half, device)
            bd = b.to(device)
            descs.append(make_desc(xd, wh, kpad, nrows, cout, ohw, geo, go.out, bias=bd, act=1))
            gos.append(go)
            keep.append((xd, wh, bd))
        descs[0].force_tile = tile
        arr = (hc.HConvDesc * len(descs))(*descs)
        assert L.call_status('fsv_hconv_gather', arr, len(descs), None, L.stream_ptr()) == L.ENUMS['FSV_OK']
        for go, pr in zip(gos, probs):
            name = 'h group tile %d half %d rows %d cout %d' % (tile, half, pr[0], pr[2])
            assert go.intact() and go.filled(), name + ': guard rows / unwritten output'
            _compare(name, go.out, pr[6], 'group', tile)
            ran += 1
    return ran


def check_stats_straddle(device, hw, must_straddle, seed=9710):
    """Epilogue statistics with groups = n where a pixel tile of the PLANNED launch (statistics are refused under forced tiles)
    spans two samples: the partials summed over the slots == float64 sums of the STORED half output, and the launch must have
    produced them.  Tolerance: a lane adds at most 32 fp32 terms (and rounds each square once) before the partials become
    doubles, so |error| <= 32 * 2^-24 * sum|term| per channel; asserted with twice that.
    hw = (12, 16): H W = 192, straddled by 128-row tiles (which the plan picks from 32768 pixels up); the plan of a map this
    small is the 64-row tile, for which hw = (12, 14), H W = 168, puts the sample boundaries 168 and 336 inside tiles 2 and 5."""
    conv, hc = _mods()
    g = torch.Generator().manual_seed(seed)
    n, cin, cout = 3, 16, 72
    h, w = hw
    x = _h(torch.randn(n, cin, h, w, generator=g))
    wt = _h(torch.randn(cout, cin, 3, 3, generator=g) * 0.2)
    xd, wh, kpad, nrows, geo, ohw = _operands(device, (n, cin, h, w, cout, 3, 1, 1), x, wt)
    tile, nsplit = hc.planned(n * h * w, cout, (9 * cin + 63) // 64, 1)
    bm = H_TILE_DIMS[tile & 15][0]
    assert nsplit == 1
    assert not must_straddle or any((gidx * h * w) % bm for gidx in range(1, n)), (tile, bm, hw)
    st = dict(groups=n)
    with conv.stats_pass(torch.device(device)), launches() as rec:
        y = hc.conv_forward_h(xd, wh, kpad, nrows, cout, geo, out_half=True, stats=st)
    assert rec.ok('fsv_hconv_gather'), rec.log
    assert 'part' in st, 'the launch produced no statistics (produced != 1)'
    part = st['part'][:n * st['slots'] * cout * 2].view(n, st['slots'], cout, 2).sum(dim=1).cpu()
    close_half('h stats output %s' % (hw,), y, conv_ref64(x, wt, 1, 1))
    yd = y.cpu().double().reshape(n, cout, h * w)
    for k_, (ref, mag) in enumerate(((yd.sum(2), yd.abs().sum(2)), ((yd * yd).sum(2), (yd * yd).sum(2)))):
        err = (part[..., k_] - ref).abs()
        lim = 2 * 32 * 2.0 ** -24 * mag
        print('H_STATS %s %s worst error / bound %.3f' % (hw, ('sum', 'sumsq')[k_], float((err / lim).max())))
        assert bool((err <= lim).all()), ('h stats', hw, ('sum', 'sumsq')[k_], float((err / lim).max()))
    return 1


# ------------------------------------------------------------------------------------------------ ragged weight gradients
def wgrad_cases(geom):
    """(force_tile, force_split) pairs of one geometry: the planned launch, then tiles 0 (automatic) .. 6 under splits 1, 2, 3 as
    far as the 64-pixel chunks of the geometry allow"""
    conv, _ = _mods()
    n, cin, h, w, cout, k, s, p = geom
    oh, ow = conv.Geom(k, k, s, p).out_hw(h, w)
    pchunks = (n * oh * ow + 63) // 64
    return [(0, 0)] + [(t, sp) for t in sorted({t for t, _ in WGRAD_TILES}) for sp in (1, 2, 3) if sp <= pchunks]


def _wgrad_layout(ref):
    """OIHW (or [N] OIHW) -> the K-major rows (tap, ci) x co of dwt"""
    co, ci, kh, kw = ref.shape[-4:]
    return ref.permute(*range(ref.dim() - 4), -2, -1, -3, -4).reshape(*ref.shape[:-4], kh * kw * ci, co)


def _check_dwt(name, dwt, ref, geo, split, tile):
    """dwt [nb][Kpad][ldw] against ref ([nb] OIHW, float64): the valid region directly; the padding rows [K, Kpad) and columns
    [Cout, ldw) are zero behind a split launch (the call's memset) and are NOT read by unprep_weight_grad (poisoned here)"""
    conv, _ = _mods()
    want = _wgrad_layout(ref)
    K, cout = want.shape[-2:]
    want = want.reshape(-1, K, cout)
    _note('wgrad', tile, False, oc.assert_close(name + ' dwt', dwt[:, :K, :cout], want, TOL))
    if split > 1:
        assert not bool(dwt[:, K:, :].any()) and not bool(dwt[:, :, cout:].any()), name + ': padding behind a split launch is not zero'
    dwt[:, K:, :] = float('nan')
    dwt[:, :, cout:] = float('nan')
    dw = conv.unprep_weight_grad(dwt, tuple(ref.shape), geo)
    oc.assert_close(name + ' OIHW', dw, ref, TOL)


@functools.lru_cache(maxsize=None)
def _wgrad_problem(geom, seed, per_sample=False):
    conv, _ = _mods()
    n, cin, h, w, cout, k, s, p = geom
    g = torch.Generator().manual_seed(seed)
    x = _h(torch.randn(n, cin, h, w, generator=g))
    dy = _h(torch.randn((n, cout) + conv.Geom(k, k, s, p).out_hw(h, w), generator=g))
    if per_sample:
        ref = torch.stack([wgrad_ref64(x[i:i + 1], dy[i:i + 1], (cout, cin, k, k), s, p) for i in range(n)])
    else:
        ref = wgrad_ref64(x, dy, (cout, cin, k, k), s, p)
    return x, dy, ref


def check_wgrad_ragged(device, gi):
    """every wgrad_cases pair on RAGGED_WG_GEOMS[gi] against wgrad_ref64.  Returns the number of launches checked."""
    conv, hc = _mods()
    geom = RAGGED_WG_GEOMS[gi]
    n, cin, h, w, cout, k, s, p = geom
    geo = conv.Geom(k, k, s, p)
    assert hc.wgrad_eligible(cin, cout, *geo.out_hw(h, w)), geom
    x, dy, ref = _wgrad_problem(geom, 8100 + gi)
    xd, dyd = hc.to_half_nhwc(x.to(device)), hc.to_half_nhwc(dy.to(device))
    ran = 0
    for tile, split in wgrad_cases(geom):
        with launches() as rec:
            dwt = hc.conv_wgrad_h(xd, dyd, geo, force_tile=tile, force_split=split)
        assert rec.ok('fsv_hconv_wgrad'), rec.log
        _check_dwt('h ragged wgrad tile %d split %d %s' % (tile, split, geom), dwt, ref, geo, split, tile)
        ran += 1
    return ran


PER_SAMPLE_WG_CASES = [(0, 0), (2, 1), (4, 2), (5, 1), (6, 2)]


def check_wgrad_per_sample(device):
    """per_sample = True, n = 3: one dwt slice per sample (w_bstride = kpad * ldw), each against its own sample's gradient"""
    conv, hc = _mods()
    geom = PER_SAMPLE_WG_GEOM
    n, cin, h, w, cout, k, s, p = geom
    geo = conv.Geom(k, k, s, p)
    assert hc.wgrad_eligible(cin, cout, *geo.out_hw(h, w)), geom
    x, dy, ref = _wgrad_problem(geom, 8200, True)
    xd, dyd = hc.to_half_nhwc(x.to(device)), hc.to_half_nhwc(dy.to(device))
    ran = 0
    for tile, split in PER_SAMPLE_WG_CASES:
        with launches() as rec:
            dwt = hc.conv_wgrad_h(xd, dyd, geo, per_sample=True, force_tile=tile, force_split=split)
        assert rec.ok('fsv_hconv_wgrad'), rec.log
        assert dwt.shape[0] == n
        _check_dwt('h per-sample wgrad tile %d split %d' % (tile, split), dwt, ref, geo, split, tile)
        ran += 1
    return ran


# ------------------------------------------------------------------------------------------------ operand preparation, D-input gradient
def check_prep_weight_tables(device, seed=9900):
    """fsv_hconv_prep_weight (the table-driven form every `--amp` step uses) over three jobs in ONE launch - K32 = 32 (K64 = 64),
    K32 = 224 (K64 = 256) and a batched nb = 3 layout with nrows = 136 below ldw = 160 - bit-equal to its definition
    (src.transpose(-1, -2).to(float16), rows [0, nrows), zero-padded to K64) and to fsv_hconv_prep_weight_one on the same sources;
    four guard halves on either side of every destination keep their bits"""
    _, hc = _mods()
    L = _lib()
    g = torch.Generator().manual_seed(seed)
    shapes = [(1, 32, 64, 64, 64), (1, 224, 32, 32, 256), (3, 96, 160, 136, 128)]          # nb, k32, ldw, nrows, k64
    jobs, bufs, wants, srcs = [], [], [], []
    for nb, k32, ldw, nrows, k64 in shapes:
        src = torch.randn(nb, k32, ldw, generator=g) * 0.2
        src[:, 0, :4] = torch.tensor([0.0, -0.0, 65504.0, 2.0 ** -24])          # zeros, the largest half, the smallest subnormal
        want = torch.zeros(nb, nrows, k64, dtype=torch.float16)
        want[:, :, :k32] = src.transpose(-1, -2).to(torch.float16)[:, :nrows]
        buf = torch.full((nb * nrows * k64 + 16,), SENTINEL_H, dtype=torch.float16, device=device)
        dst = buf[8:8 + nb * nrows * k64].view(nb, nrows, k64)
        sd = src.to(device)
        jobs.append((sd, dst))
        bufs.append(buf)
        wants.append(want)
        srcs.append(sd)
    tables = hc._prep_tables(jobs, torch.device(device))
    assert tables[2] == sum(nb * ((k64 + 63) // 64) * ((nrows + 63) // 64) for nb, _, _, nrows, k64 in shapes)
    with launches() as rec:
        hc.launch_prep(tables)
    assert rec.ok('fsv_hconv_prep_weight'), rec.log
    for (nb, k32, ldw, nrows, k64), (sd, dst), buf, want in zip(shapes, jobs, bufs, wants):
        name = 'prep_weight tables %s' % ((nb, k32, ldw, nrows, k64),)
        assert bool((_bits(dst) == _bits(want)).all()), name + ': differs from the definition'
        assert bool((buf[:8] == SENTINEL_H).all()) and bool((buf[-8:] == SENTINEL_H).all()), name + ': wrote outside its destination'
        one = torch.full((nb, nrows, k64), SENTINEL_H, dtype=torch.float16, device=device)
        L.call('fsv_hconv_prep_weight_one', L.ptr(sd), L.ptr(one), k32, ldw, nrows, k64, nb, L.stream_ptr())
        assert bool((_bits(one) == _bits(dst)).all()), name + ': differs from fsv_hconv_prep_weight_one'
    return len(shapes)


UNPACK_CASES = [(2, 35, 16, 11, 3), (2, 35, 16, 10, 3), (1, 7, 8, 5, 3), (3, 300, 40, 36, 4)]          # B, P, Ct, Coff, Ci


def check_unpack_d_grad_h(device, seed=9910):
    """fsv_unpack_d_grad_h: dfake [B][Ci][P] (fp32) == dout[..., Coff:Coff + Ci].float() of the half tensor dout [B][P][Ct], bit
    for bit, at an odd and an even Coff (the halves are not 4-byte aligned at an odd one); guard words around dfake keep their bits"""
    L = _lib()
    g = torch.Generator().manual_seed(seed)
    for B, P, Ct, Coff, Ci in UNPACK_CASES:
        dout = (torch.randn(B, P, Ct, generator=g) * 3.0).to(torch.float16)
        want = dout[..., Coff:Coff + Ci].float().permute(0, 2, 1).contiguous()
        buf = torch.full((B * Ci * P + 8,), float('nan'), device=device)
        before = buf.clone()
        dst = buf[4:4 + B * Ci * P]
        dd = dout.to(device)
        L.check_device(dd, buf)
        L.call('fsv_unpack_d_grad_h', L.ptr(dd), L.ptr(dst), B, Ci, Coff, Ct, P, L.stream_ptr())
        name = 'unpack_d_grad_h %s' % ((B, P, Ct, Coff, Ci),)
        assert bool((_bits(dst) == _bits(want.reshape(-1))).all()), name
        assert bool((_bits(buf[:4]) == _bits(before[:4])).all()) and bool((_bits(buf[-4:]) == _bits(before[-4:])).all()), name + ': guards'
    return len(UNPACK_CASES)


if __name__ == '__main__':
    dev = torch.device('cuda', 0)
    check_cast(dev)
    for geom in GEOMS + BIG_GEOMS:
        for half in (True, False):
            check_forward(dev, geom, -1, 0, half)
            check_dgrad(dev, geom, half)
        check_wgrad(dev, geom, 0, 0)
    for tile, split in FWD_TILES:
        check_forward(dev, BIG_GEOMS[0], tile, split, True)
        check_forward(dev, BIG_GEOMS[2], tile, split, False, res_half=True)
    for tile, split in WGRAD_TILES:
        check_wgrad(dev, BIG_GEOMS[1], tile, split)
    check_group(dev)
    check_stats(dev)
    for tile in RAGGED_TILES:
        assert check_forward_ragged(dev, tile) == RAGGED_CASES_PER_TILE
    for name in EPILOGUE_CASES:
        for tile in EPILOGUE_TILES:
            check_epilogue(dev, name, tile)
    for gi in range(len(RAGGED_WG_GEOMS)):
        check_wgrad_ragged(dev, gi)
    print('H_GPU_OK', flush=True)
