"""Direct checks of the kernels every parameter of G and D passes through on every training step - the K-major layout writer
(fsv_prep_weight_grouped, fsv_prep_weight), the weight-gradient finalisation (fsv_wgrad_finalize), the spectral-norm backward
(fsv_sn_backward) and the power iteration (fsv_sn_power_iter, fsv_sn_power_iter_batched) - shared by the emulated (`not gpu`) and
the real-hardware (`gpu`) test modules.

Every entry point is driven through the C ABI with tables built here, and compared with PyTorch float64 on the CPU computed from
the same seeded fp32 inputs (a scalar that travels as `float` enters the reference as its fp32 value).  There are two bars and no
other: where a kernel only routes values (a selected tap, a transposed gradient plus ONE fp32 add) the comparison is bit for bit;
where it rounds, it is small_op_checks.bounded - MARGIN times the error of an fp32 PyTorch restatement of the same formula, plus
two fp32 ulp.  Buffers the producer never writes (columns [Cout, ldw) of a K-major gradient or weight) hold NaN, outputs are
surrounded by guard words whose bits must survive, and inputs are compared with their copies afterwards.

Measured kernel error / restatement error, worst over the cases, the same on the emulator and on an MI355X: summed-tap layouts
1.00, fsv_prep_weight with scale_ptr / col_scale 1.00, finalised spectral sink 2.13 and its dot 7.65, fsv_sn_backward 1.10,
power iteration u 1.00, v 1.00, eval-mode sigma 1.78 and 1 / sigma 1.31.  sigma and 1 / sigma of the training iteration are single
numbers whose restatement error is now and then tiny (ratios 54 and 944): there the two-ulp floor carries the comparison, and the
kernel's error is at most 0.46 of the bound.
"""
import torch
import torch.nn.functional as F

from op_checks import _dev, pkg
from small_op_checks import _guarded, _guards_untouched, bits, bounded, f32, lib, same_bits

GEOMS = ((1, 1), (2, 2), (3, 3), (4, 4), (3, 1), (7, 1))   # KH * KW = 1, 4, 9, 16 (the compiled tap counts but 4), 3 and 7 (generic);
#                                                            <= 8 source taps: 32-channel ci tile, above: 16
COUTS = (5, 33, 130)                                       # below one 32-co tile, one past a tile, five tiles with a ragged last
CINS = (3, 20, 35)                                         # below a ci tile, between the two tile widths, past both with a ragged tail
CPADS = (0, 1)
NAN = float('nan')
SN_EPS = 1e-12


def _ceil(a, b):
    return (a + b - 1) // b * b


def _all_taps(kh, kw):
    return [i for i in range(kh) for _ in range(kw)], [j for _ in range(kh) for j in range(kw)]


def _pack(khs, kws):
    """(kh | kw << 4) codes, eight per 64-bit word, as the two signed words an int64 tensor holds"""
    words = [0, 0]
    for j, (a, b) in enumerate(zip(khs, kws)):
        words[j // 8] |= ((a | (b << 4)) & 0xff) << (8 * (j % 8))
    return [w - (1 << 64) if w >= (1 << 63) else w for w in words]


def _table(vals, dtype, device):
    return torch.tensor(vals if vals else [0], dtype=dtype).to(device)


def _guard_copy(t, device, g):
    """device copy of the host tensor t between guard words -> (buffer, view, copy of the buffer)"""
    buf, view = _guarded(t.numel(), device, g)
    view.copy_(_dev(t.reshape(-1), device))
    return buf, view, buf.clone()


def _bad_arg():
    return lib().ENUMS['FSV_ERR_BAD_ARG']


# ------------------------------------------------------------------------------- fsv_prep_weight_grouped / fsv_prep_weight
def _layout_specs(kh, kw):
    """(name, mode, tap codes) of the layouts one launch writes for a [Cout][Cin][kh][kw] weight: the forward layout, the same
    with its taps reversed, the data-gradient layout of every stride-2 parity class that has taps (tap subsets), and for 3x3 the
    two summed-tap layouts of conv3x3(nearest_x2(x)) as LayoutCache._add_up_jobs builds them"""
    from importlib import import_module
    pkg()
    lc = import_module('few-shot-vid2vid_amd.layout_cache')
    khs, kws = _all_taps(kh, kw)
    specs = [('forward', 0, khs, kws), ('forward reversed', 0, khs[::-1], kws[::-1])]
    for a in (0, 1):
        for b in (0, 1):
            taps = [(i, j) for i in range(kh) if i % 2 == a for j in range(kw) if j % 2 == b]
            if taps:
                specs.append(('dgrad parity %d%d' % (a, b), 1, [t[0] for t in taps], [t[1] for t in taps]))
    if (kh, kw) == (3, 3):
        cls = [(ry, rx) for ry in (0, 1) for rx in (0, 1)]
        ph = [2 * ry + iy for ry, rx in cls for iy in (0, 1) for _ in (0, 1)]
        pw = [2 * rx + ix for ry, rx in cls for _ in (0, 1) for ix in (0, 1)]
        specs.append(('summed sub-pixel forward', 0 | 4, [lc.SUBPIXEL_MASKS[p] for p in ph], [lc.SUBPIXEL_MASKS[q] for q in pw]))
        specs.append(('summed dgrad', 1 | 4, [lc.DGRAD_MASKS[a] for a in range(4) for _ in range(4)],
                      [lc.DGRAD_MASKS[b] for _ in range(4) for b in range(4)]))
        assert len(specs[-1][2]) == len(specs[-2][2]) == 16
    return specs


def _layout_ref(w, cinp, mode, khs, kws, dtype):
    """the valid region of a layout, every operation in `dtype`: rows (tap, ci) x Cout columns (mode 0) or rows (tap, co) x
    CinP columns (mode 1); padded input channels are zero; mode | 4: the codes are masks and the taps they select are added
    in ascending (kh, kw) order"""
    cout, cin, KH, KW = w.shape
    wp = torch.zeros(cout, cinp, KH, KW, dtype=dtype)
    wp[:, :cin] = w.to(dtype)
    planes = []
    for a, b in zip(khs, kws):
        if mode & 4:
            acc = None
            for i in range(KH):
                for j in range(KW):
                    if (a >> i) & 1 and (b >> j) & 1:
                        acc = wp[:, :, i, j].clone() if acc is None else acc + wp[:, :, i, j]
            planes.append(acc)
        else:
            planes.append(wp[:, :, a, b])
    t = torch.stack(planes)                                                        # [ntaps][Cout][CinP]
    return t.reshape(-1, cinp) if mode & 1 else t.permute(0, 2, 1).reshape(-1, cout)


def _prep_weight(L, w, wt, scale, mode, nb, cout, cin, kh, kw, khs, kws, kpad, ldw, w_bs, wt_bs, col):
    return L.call_status('fsv_prep_weight', L.ptr(w), L.ptr(wt), L.ptr(scale), mode, nb, cout, cin, kh, kw, len(khs),
                         L.int_array(khs), L.int_array(kws), kpad, ldw, w_bs, wt_bs, L.ptr(col), L.stream_ptr())


def check_layouts(device, kh, kw, cout, cin, cpad, seed=131):
    """fsv_prep_weight_grouped: every layout of _layout_specs written by ONE launch from one [cout][cin][kh][kw] weight (one tmap
    quadruple per source tile, as LayoutCache._build lays them out).  Selected-tap layouts equal the weight bit for bit, summed-tap
    layouts are `bounded` against the fp64 sum (restatement: the fp32 sum in ascending (kh, kw) order); run once on pre-zeroed
    layouts (every cell outside the valid region is 0.0 afterwards) and once with the valid region NaN (every valid cell was
    written); guard words around every layout and the weight keep their bits.  Then fsv_prep_weight, modes 0 / 1 without scale, on
    the un-padded weight: the bits of the grouped call, and zeros everywhere else.  Returns {layout name: valid region}."""
    L = lib()
    g = torch.Generator().manual_seed(seed + 1000 * kh + 100 * kw + 7 * cout + cin + cpad)
    cinp, kk = cin + cpad, kh * kw
    w_host = torch.randn(cout, cin, kh, kw, generator=g)
    wbuf, w, wbefore = _guard_copy(w_host, device, g)
    specs = _layout_specs(kh, kw)
    tag0 = 'layouts %dx%d cout=%d cin=%d+%d ' % (kh, kw, cout, cin, cpad)
    ci_t = 32 if kk <= 8 else 16
    tmap = [v for a in range((cout + 31) // 32) for b in range((cinp + ci_t - 1) // ci_t) for v in (0, len(specs), a, b)]
    kept = {}
    for prefill in ('zero', 'nan'):
        jobs, dims, taps = [], [], []
        for name, mode, khs, kws in specs:
            ntaps = len(khs)
            rowlen, ncols = (cout, cinp) if mode & 1 else (cinp, cout)
            nrows = ntaps * rowlen
            kpad, ldw = _ceil(nrows, 32), _ceil(ncols, 32)
            buf, wt = _guarded(kpad * ldw, device, g)
            wt.zero_()
            if prefill == 'nan':
                wt.view(kpad, ldw)[:nrows, :ncols] = NAN
            jobs.append((buf, wt, buf.clone(), nrows, ncols, kpad, ldw))
            dims += [cout, cinp, cin, kh, kw, ntaps, kpad, ldw, mode]
            taps += _pack(khs, kws)
        tables = (_table([w.data_ptr()] * len(specs), torch.int64, device), _table([j[1].data_ptr() for j in jobs], torch.int64, device),
                  _table(dims, torch.int32, device), _table(taps, torch.int64, device), _table(tmap, torch.int32, device))
        L.check_device(w, *[j[1] for j in jobs])
        L.call('fsv_prep_weight_grouped', *[L.ptr(t) for t in tables], len(tmap) // 4, L.stream_ptr())
        for (name, mode, khs, kws), (buf, wt, before, nrows, ncols, kpad, ldw) in zip(specs, jobs):
            tag = tag0 + name + (' (valid region NaN before)' if prefill == 'nan' else '')
            got = wt.cpu().view(kpad, ldw)
            valid = got[:nrows, :ncols]
            assert bool(torch.isfinite(valid).all()), '%s: a valid cell was not written' % tag
            ref = _layout_ref(w_host, cinp, mode, khs, kws, torch.float64)
            if mode & 4:
                bounded(tag, valid, ref, _layout_ref(w_host, cinp, mode, khs, kws, torch.float32))
            else:
                same_bits(tag, valid, ref.float())
            outside = got.clone()
            outside[:nrows, :ncols] = 0.0
            assert bool((outside == 0.0).all()), '%s: a cell outside the valid region is not 0.0' % tag
            _guards_untouched(tag, buf, before, kpad * ldw)
            kept[name] = valid.clone()
        same_bits(tag0 + 'the weight and its guard words', wbuf, wbefore)
    for name, mode, khs, kws in specs:
        if mode & 4:
            continue
        ntaps = len(khs)
        rowlen, ncols = (cout, cin) if mode == 1 else (cin, cout)
        kpad, ldw = _ceil(ntaps * rowlen, 32), _ceil(ncols, 32)
        buf, wt = _guarded(kpad * ldw, device, g)
        wt.fill_(NAN)                                              # the single-weight kernel writes the whole [Kpad][ldw]
        before = buf.clone()
        assert _prep_weight(L, w, wt, None, mode, 1, cout, cin, kh, kw, khs, kws, kpad, ldw, cout * cin * kk, kpad * ldw, None) == 0
        want = torch.zeros(kpad, ldw)
        grouped = kept[name]                                       # drop the rows / columns of the padded input channels
        want[:ntaps * rowlen, :ncols] = grouped[:, :cin] if mode == 1 else grouped.view(ntaps, cinp, cout)[:, :cin].reshape(-1, cout)
        same_bits(tag0 + name + ': fsv_prep_weight against the grouped call', wt.view(kpad, ldw), want)
        _guards_untouched(tag0 + name + ' fsv_prep_weight', buf, before, kpad * ldw)
    return kept


def check_prep_weight_modes(device, kh, kw, cout, cin, seed=132):
    """fsv_prep_weight beyond the plain re-arrangement, on the forward layout of one weight: mode 0 with `scale_ptr` and with
    `col_scale` `bounded` against fp64; both together FSV_ERR_BAD_ARG with the buffer untouched; mode 2 on the mode-0 layout
    returns the weight bit for bit; mode 3 adds it into a seeded buffer with one fp32 add; nbatch = 2 with both batch strides
    larger than the dense sizes, the gap between the two layouts and the guard words keeping their bits."""
    L = lib()
    g = torch.Generator().manual_seed(seed + 1000 * kh + 100 * kw + 7 * cout + cin)
    kk = kh * kw
    khs, kws = _all_taps(kh, kw)
    nrows, dense = kk * cin, cout * cin * kk
    kpad, ldw = _ceil(nrows, 32), _ceil(cout, 32)
    w_host = torch.randn(cout, cin, kh, kw, generator=g)
    w = _dev(w_host, device)
    tag0 = 'prep_weight %dx%d cout=%d cin=%d ' % (kh, kw, cout, cin)
    args = (cout, cin, kh, kw, khs, kws, kpad, ldw, dense, kpad * ldw)
    ref64, ref32 = (_layout_ref(w_host, cin, 0, khs, kws, dt) for dt in (torch.float64, torch.float32))

    def full(valid):
        out = torch.zeros(kpad, ldw, dtype=valid.dtype)
        out[:nrows, :cout] = valid
        return out

    scale = torch.tensor([0.3 + float(torch.rand(1, generator=g))])
    col = 0.5 + torch.rand(cout, generator=g)
    sd, cd = _dev(scale, device), _dev(col, device)
    for name, sp, cp, r64, r32 in (('scale_ptr', sd, None, ref64 * scale.double(), ref32 * scale),
                                   ('col_scale', None, cd, ref64 * col.double(), ref32 * col)):
        buf, wt = _guarded(kpad * ldw, device, g)
        wt.fill_(NAN)
        before = buf.clone()
        assert _prep_weight(L, w, wt, sp, 0, 1, *args, cp) == 0
        bounded(tag0 + name, wt.view(kpad, ldw), full(r64), full(r32))
        _guards_untouched(tag0 + name, buf, before, kpad * ldw)
    buf, wt = _guarded(kpad * ldw, device, g)
    before = buf.clone()
    assert _prep_weight(L, w, wt, sd, 0, 1, *args, cd) == _bad_arg()
    same_bits(tag0 + 'scale_ptr and col_scale together', buf, before)

    layout = torch.empty(kpad * ldw, device=device)
    assert _prep_weight(L, w, layout, None, 0, 1, *args, None) == 0
    lay0 = layout.clone()
    for mode in (2, 3):
        buf, out = _guarded(dense, device, g)
        if mode == 2:
            out.fill_(NAN)
        before = buf.clone()
        assert _prep_weight(L, out, layout, None, mode, 1, *args, None) == 0
        want = w_host.reshape(-1) if mode == 2 else before[4:4 + dense].cpu() + w_host.reshape(-1)
        same_bits(tag0 + 'mode %d' % mode, out, want)
        _guards_untouched(tag0 + 'mode %d' % mode, buf, before, dense)
    same_bits(tag0 + 'the layout modes 2 / 3 read', layout, lay0)

    w_bs, wt_bs = dense + 3, kpad * ldw + 5
    w2 = torch.randn(w_bs + dense, generator=g)
    buf, wt = _guarded(wt_bs + kpad * ldw, device, g)
    before = buf.clone()
    assert _prep_weight(L, _dev(w2, device), wt, None, 0, 2, cout, cin, kh, kw, khs, kws, kpad, ldw, w_bs, wt_bs, None) == 0
    for z in (0, 1):
        wz = w2[z * w_bs:z * w_bs + dense].view(cout, cin, kh, kw)
        same_bits(tag0 + 'nbatch = 2, sample %d' % z, wt[z * wt_bs:z * wt_bs + kpad * ldw].view(kpad, ldw),
                  full(_layout_ref(wz, cin, 0, khs, kws, torch.float32)))
    same_bits(tag0 + 'nbatch = 2: the gap between the layouts', wt[kpad * ldw:wt_bs], before[4 + kpad * ldw:4 + wt_bs])
    _guards_untouched(tag0 + 'nbatch = 2', buf, before, wt_bs + kpad * ldw)


# ------------------------------------------------------------------------------------------------------ fsv_wgrad_finalize
def _fin_job(g, device, cout, cin, cpad, kh, kw, khs=None, kws=None, spectral=False, shares=None, W=None):
    """one job of fsv_wgrad_finalize.  dwt [Kpad][ldw]: seeded values in rows (tap, ci < CinP) x columns [0, Cout) - the rows of
    padded input channels included: nothing of them may reach the sink -, NaN in the columns [Cout, ldw) and the rows behind, which
    the weight-gradient kernel never writes.  Spectral: the K-major W likewise (zeros in the rows of padded channels), u, v
    normalised, sig = (sigma, fp32(1 / sigma)).  G: the OIHW gradient dwt holds (zero at absent taps).

    The gradient of a spectral job is randn + 5 W: with a component along W, <G, W> is about 5 |W|^2 = 0.05 n, of the order of
    the sum of the products' magnitudes.  For independent G and W the products cancel (|<G, W>| ~ 0.1 sqrt(n) against a sum of
    magnitudes of 0.08 n), and every fp32 evaluation - the restatement included - errs by the roundings of n products, some
    thousand ulp of the result: `bounded`, whose floor is two ulp of the result, then compares two such errors with each other
    and the restatement's is now and then small by chance (seen: kernel 4.3e-7, restatement 1.7e-8, on a dot of 0.69 whose
    4550 products sum to 364 in magnitude)."""
    if khs is None:
        khs, kws = _all_taps(kh, kw)
    cinp, ntaps, kk = cin + cpad, len(khs), kh * kw
    nrows, ldw = ntaps * cinp, _ceil(cout, 32)
    kpad = _ceil(nrows, 32)
    dwt = torch.full((kpad, ldw), NAN)
    dwt[:nrows, :cout] = torch.randn(nrows, cout, generator=g)
    wrows = torch.zeros(ntaps, cinp, cout)
    if spectral:
        W = torch.randn(cout, cin, kh, kw, generator=g) * 0.1 if W is None else W
        for j, (a, b) in enumerate(zip(khs, kws)):
            wrows[j, :cin] = W[:, :, a, b].t()
        dwt[:nrows, :cout] += 5.0 * wrows.view(nrows, cout)
    rows = dwt[:nrows, :cout].view(ntaps, cinp, cout)
    G = torch.zeros(cout, cin, kh, kw)
    present = torch.zeros(kh, kw, dtype=torch.bool)
    for j, (a, b) in enumerate(zip(khs, kws)):
        G[:, :, a, b] = rows[j, :cin].t()
        present[a, b] = True
    job = dict(cout=cout, cin=cin, cinp=cinp, kh=kh, kw=kw, khs=khs, kws=kws, ntaps=ntaps, ldw=ldw, kpad=kpad, G=G, present=present,
               spectral=spectral, shares=shares, n=cout * cin * kk, host=dict(dwt=dwt))
    if spectral:
        assert ntaps == kk and bool(present.all())
        wlay = torch.full((kpad, ldw), NAN)
        wlay[:nrows, :cout] = wrows.view(nrows, cout)
        sigma = 0.5 + float(torch.rand(1, generator=g))
        job['W'] = W
        job['host'].update(wlay=wlay, u=F.normalize(torch.randn(cout, generator=g), dim=0),
                           v=F.normalize(torch.randn(cin * kk, generator=g), dim=0), sig=torch.tensor([sigma, 1.0 / sigma]))
    job['dev'] = {k: _dev(t, device) for k, t in job['host'].items()}
    return job


def _fin_words(job):
    """dims[8] without the flags word, and the two tap words"""
    return [job['cout'], job['cinp'], job['cin'], job['kh'], job['kw'], job['ntaps'], job['ldw']], _pack(job['khs'], job['kws'])


def _sn_formula(s0, G, W, u, v, inv, dtype):
    """sink0 + (G - (<G, W> / sigma) u v^T) / sigma with 1 / sigma = the fp32 word sig[1], every operation in `dtype`;
    -> (result, <G, W>)"""
    s0, G, W, u, v = (t.to(dtype) for t in (s0, G, W, u, v))
    inv = torch.tensor(inv, dtype=dtype)
    dot = torch.sum(G * W)
    return s0 + inv * (G - (inv * dot) * torch.outer(u, v).view_as(G)), dot


def check_finalize(device, jobs, seed=133, name='finalize'):
    """One fsv_wgrad_finalize call over `jobs`, tables laid out as GradFinalizer._build_static does.  Every sink is a slice of
    one seeded flat buffer (job['shares'] = index of the job whose slice it adds into), with other seeded words between the
    slices.  Checks every bar of the module docstring and returns the flat buffer (host) and the sink offsets."""
    L = lib()
    g = torch.Generator().manual_seed(seed)
    offs, cursor = [], 7
    for job in jobs:
        if job['shares'] is not None:
            assert jobs[job['shares']]['n'] == job['n'] and not job['spectral'] and not jobs[job['shares']]['spectral']
            offs.append(offs[job['shares']])
        else:
            offs.append(cursor)
            cursor += job['n'] + 5
    flat0 = torch.randn(cursor + 3, generator=g)
    flat = _dev(flat0.clone(), device)
    users = {o: [j for j, oo in enumerate(offs) if oo == o] for o in offs}
    ptrs, dims, taps, tmap_dot, tmap_apply = [], [], [], [], []
    for j, (job, off) in enumerate(zip(jobs, offs)):
        d = job['dev']
        sn = job['spectral']
        ptrs += [d['dwt'].data_ptr(), d['wlay'].data_ptr() if sn else 0, flat.data_ptr() + 4 * off, d['u'].data_ptr() if sn else 0,
                 d['v'].data_ptr() if sn else 0, d['sig'].data_ptr() if sn else 0]
        words, tw = _fin_words(job)
        dims += words + [1 if len(users[off]) > 1 else 0]
        taps += tw
        if sn:
            total = job['ntaps'] * job['cinp'] * job['ldw']
            tmap_dot += [v for ch in range((total + 4095) // 4096) for v in (j, ch)]
        ci_t = 32 if job['ntaps'] <= 8 else 16
        tmap_apply += [v for a in range((job['cout'] + 31) // 32) for b in range((job['cinp'] + ci_t - 1) // ci_t) for v in (j, a, b)]
    n = len(jobs)
    dots = torch.full((n + 2,), 12345.0, dtype=torch.float64, device=device)
    tables = (_table(ptrs, torch.int64, device), _table(dims, torch.int32, device), _table(taps, torch.int64, device))
    td, ta = _table(tmap_dot, torch.int32, device), _table(tmap_apply, torch.int32, device)
    L.check_device(flat, *[t for job in jobs for t in job['dev'].values()])
    L.call('fsv_wgrad_finalize', *[L.ptr(t) for t in tables], L.ptr(dots[1:]), n, L.ptr(td), len(tmap_dot) // 2, L.ptr(ta),
           len(tmap_apply) // 3, L.stream_ptr())
    got, dots = flat.cpu(), dots.cpu()
    outside = torch.ones(flat0.numel(), dtype=torch.bool)
    for job, off in zip(jobs, offs):
        outside[off:off + job['n']] = False
    same_bits(name + ': the words of the flat buffer around the sinks', got[outside], flat0[outside])
    assert float(dots[0]) == 12345.0 and float(dots[-1]) == 12345.0, name + ': wrote outside dots[njobs]'
    for j, (job, off) in enumerate(zip(jobs, offs)):
        tag = '%s job %d (%dx%d cout=%d cin=%d+%d, %d taps%s)' % (name, j, job['kh'], job['kw'], job['cout'], job['cin'],
                                                                    job['cinp'] - job['cin'], job['ntaps'], ', spectral' if job['spectral'] else '')
        for key, t in job['host'].items():
            same_bits(tag + ': input ' + key, job['dev'][key], t)
        s0, sink = flat0[off:off + job['n']].view_as(job['G']), got[off:off + job['n']].view_as(job['G'])
        if job['spectral']:
            h = job['host']
            inv = float(h['sig'][1])
            (r64, d64), (r32, d32) = (_sn_formula(s0, job['G'], job['W'], h['u'], h['v'], inv, dt) for dt in (torch.float64, torch.float32))
            bounded(tag + ' sink', sink, r64, r32)
            bounded(tag + ' dot', dots[1 + j].reshape(1), d64.reshape(1), d32.reshape(1))
            continue
        assert float(dots[1 + j]) == 0.0, tag + ': dots of a plain job'
        if users[off] == [j]:
            same_bits(tag + ' sink', sink, s0 + job['G'])
            absent = ~job['present']
            if bool(absent.any()):
                same_bits(tag + ' sink cells of absent taps', sink[:, :, absent], s0[:, :, absent])
        elif users[off][0] == j:
            a, b = (jobs[k]['G'] for k in users[off])
            assert len(users[off]) == 2
            first, second = (s0 + a) + b, (s0 + b) + a
            assert int((bits(first) != bits(second)).sum()) > 0, 'the order of the two adds would not show'
            if L.is_emu():                                      # blocks run in launch order there
                same_bits(tag + ' shared sink', sink, first)
            bad = int(((bits(sink) != bits(first)) & (bits(sink) != bits(second))).sum())
            assert bad == 0, '%s: %d elements of the shared sink are neither (s + g1) + g2 nor (s + g2) + g1' % (tag, bad)
    return got, offs


def check_finalize_geometry(device, kh, kw, cout, cin, cpad, seed=134):
    """a plain and a spectral job of one geometry in one call, each on its own sink"""
    g = torch.Generator().manual_seed(seed + 1000 * kh + 100 * kw + 7 * cout + cin + cpad)
    jobs = [_fin_job(g, device, cout, cin, cpad, kh, kw), _fin_job(g, device, cout, cin, cpad, kh, kw, spectral=True)]
    check_finalize(device, jobs, seed + cout + cin, 'finalize')


def check_finalize_tap_subset(device, seed=135):
    """4 of the 9 taps of a 3x3 gradient, in an order that is not ascending: the sink cells of the five absent taps keep their
    bits (check_finalize asserts it); and all nine in reversed order"""
    g = torch.Generator().manual_seed(seed)
    khs, kws = _all_taps(3, 3)
    jobs = [_fin_job(g, device, 33, 20, 1, 3, 3, khs=[2, 0, 1, 0], kws=[1, 2, 1, 0]),
            _fin_job(g, device, 33, 20, 0, 3, 3, khs=khs[::-1], kws=kws[::-1]),
            _fin_job(g, device, 5, 35, 0, 3, 3, khs=khs[::-1], kws=kws[::-1], spectral=True)]
    check_finalize(device, jobs, seed, 'finalize tap subset')


def check_finalize_shared_sink(device, seed=136):
    """two plain jobs add into one sink (flags bit 0: atomic adds) next to a job with a sink of its own"""
    g = torch.Generator().manual_seed(seed)
    jobs = [_fin_job(g, device, 33, 20, 1, 3, 3), _fin_job(g, device, 5, 3, 0, 2, 2), _fin_job(g, device, 33, 20, 1, 3, 3, shares=0)]
    check_finalize(device, jobs, seed, 'finalize shared sink')


def check_finalize_five_jobs(device, seed=137):
    """five jobs of five geometries in one call, plain and spectral mixed"""
    g = torch.Generator().manual_seed(seed)
    jobs = [_fin_job(g, device, 33, 20, 0, 1, 1, spectral=True), _fin_job(g, device, 5, 3, 1, 3, 3),
            _fin_job(g, device, 33, 20, 0, 4, 4, spectral=True), _fin_job(g, device, 130, 35, 1, 7, 1),
            _fin_job(g, device, 5, 35, 1, 2, 2, spectral=True)]
    check_finalize(device, jobs, seed, 'finalize five jobs')


def check_finalize_long_dot(device, seed=138):
    """a spectral job whose ntaps * CinP * ldw = 9 * 20 * 64 = 11520 elements are two full 4096-element dot chunks and a ragged
    third"""
    g = torch.Generator().manual_seed(seed)
    job = _fin_job(g, device, 33, 20, 0, 3, 3, spectral=True)
    total = job['ntaps'] * job['cinp'] * job['ldw']
    assert total > 2 * 4096 and total % 4096 != 0
    check_finalize(device, [job], seed, 'finalize long dot')


def check_finalize_layout_cache(device, cout=33, cin=20, cpad=1, seed=139):
    """the words of a real LayoutCache entry: a 3x3 weight registered through LayoutCache.lookup gives jobs[0] = (layout, dims,
    taps); the dims / tap words this module builds by hand equal them.  Then the entry's forward layout (written by
    fsv_prep_weight_grouped) finalised as dwt into a zero sink returns the weight bit for bit, and a spectral job reads it as its
    K-major W."""
    from importlib import import_module
    _, conv = pkg()
    lc = import_module('few-shot-vid2vid_amd.layout_cache')
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    weight = _dev(W.clone(), device)
    e = lc.LayoutCache().lookup(weight, (cout, cin, 3, 3), conv.Geom(3, 3, 1, 1), cpad)
    wt, d, lo, hi = e.jobs[0]
    spectral = _fin_job(g, device, cout, cin, cpad, 3, 3, spectral=True, W=W)
    words, tw = _fin_words(spectral)
    assert words == d[:6] + [d[7]] and d[8] == 0, (words, d)
    assert tw == [lc._i64(lo), lc._i64(hi)], (tw, lo, hi)
    assert tuple(wt.shape) == (1, spectral['kpad'], spectral['ldw'])
    spectral['host']['wlay'] = wt.cpu().clone()
    spectral['dev']['wlay'] = wt
    back = _fin_job(g, device, cout, cin, cpad, 3, 3)
    back['G'] = W
    back['host']['dwt'] = wt.cpu().clone()
    back['dev']['dwt'] = wt
    got, offs = check_finalize(device, [spectral, back], seed, 'finalize layout cache')
    L = lib()
    flat = torch.zeros(back['n'] + 8, device=device)
    d_ = back['dev']
    words, tw = _fin_words(back)
    tmap = [v for a in range((cout + 31) // 32) for b in range((cin + cpad + 15) // 16) for v in (0, a, b)]
    tables = (_table([d_['dwt'].data_ptr(), 0, flat.data_ptr() + 16, 0, 0, 0], torch.int64, device), _table(words + [0], torch.int32, device),
              _table(tw, torch.int64, device))
    dots = torch.zeros(1, dtype=torch.float64, device=device)
    ta = _table(tmap, torch.int32, device)
    L.call('fsv_wgrad_finalize', *[L.ptr(t) for t in tables], L.ptr(dots), 1, None, 0, L.ptr(ta), len(tmap) // 3, L.stream_ptr())
    same_bits('finalize round trip: layout of W into a zero sink', flat[4:4 + back['n']], W.reshape(-1))
    assert not bool(flat[:4].any()) and not bool(flat[4 + back['n']:].any())


def check_finalize_bad_args(device, seed=140):
    """null ptrs / dims / taps / dots, njobs = 0, nblk_apply = 0 (and a null tmap_apply), nblk_dot > 0 with a null tmap_dot:
    FSV_ERR_BAD_ARG, and sink and dots as they were"""
    L = lib()
    g = torch.Generator().manual_seed(seed)
    job = _fin_job(g, device, 5, 3, 0, 3, 3, spectral=True)
    flat0 = torch.randn(job['n'], generator=g)
    flat = _dev(flat0.clone(), device)
    d = job['dev']
    words, tw = _fin_words(job)
    ptrs = _table([d['dwt'].data_ptr(), d['wlay'].data_ptr(), flat.data_ptr(), d['u'].data_ptr(), d['v'].data_ptr(), d['sig'].data_ptr()],
                  torch.int64, device)
    dims, taps = _table(words + [0], torch.int32, device), _table(tw, torch.int64, device)
    td, ta = _table([0, 0], torch.int32, device), _table([0, 0, 0], torch.int32, device)
    dots = torch.full((1,), 12345.0, dtype=torch.float64, device=device)
    good = [L.ptr(ptrs), L.ptr(dims), L.ptr(taps), L.ptr(dots), 1, L.ptr(td), 1, L.ptr(ta), 1]
    cases = [('null ptrs', 0, None), ('null dims', 1, None), ('null taps', 2, None), ('null dots', 3, None), ('njobs = 0', 4, 0),
             ('null tmap_dot with nblk_dot = 1', 5, None), ('nblk_apply = 0', 8, 0), ('null tmap_apply', 7, None)]
    for name, k, v in cases:
        args = list(good)
        args[k] = v
        assert L.call_status('fsv_wgrad_finalize', *args, L.stream_ptr()) == _bad_arg(), name
        same_bits('finalize ' + name + ': sink', flat, flat0)
        assert float(dots.cpu()[0]) == 12345.0, name
    assert L.call_status('fsv_wgrad_finalize', *good, L.stream_ptr()) == 0         # and the same tables are good ones
    assert int((bits(flat) != bits(flat0)).sum()) > job['n'] // 2
    return len(cases)


# --------------------------------------------------------------------------------------------------------- fsv_sn_backward
SN_BWD_SHAPES = ((1, 1), (5, 7), (40, 300), (130, 70), (512, 4608))    # one value; n % 4 != 0 in one block; ...; 2.36 M elements:
#                                                                        above the 256-partial cap, two passes of both grid-stride loops
SN_BWD_OFFSETS = ((5, 7, 1), (130, 70, 3))                             # (R, Cc, floats off 16-byte alignment): the scalar dot branch


def _sn_inputs(g, R, Cc):
    sigma = 0.5 + float(torch.rand(1, generator=g))
    return dict(dWsn=torch.randn(R, Cc, generator=g), W=torch.randn(R, Cc, generator=g) * 0.1,
                u=F.normalize(torch.randn(R, generator=g), dim=0), v=F.normalize(torch.randn(Cc, generator=g), dim=0),
                sig=torch.tensor([sigma, 1.0 / sigma]), dW0=torch.randn(R, Cc, generator=g))


def _shifted(t, off, device, g):
    """device copy of t starting 4 + off floats into its buffer (off = 1, 3: not 16-byte aligned), four seeded words behind it
    -> (buffer, view, copy of the buffer, floats in front)"""
    n, pad = t.numel(), 4 + off
    buf = _dev(torch.cat([torch.randn(pad, generator=g) + 10.0, t.reshape(-1), torch.randn(4, generator=g) + 10.0]), device)
    return buf, buf[pad:pad + n], buf.clone(), pad


def check_sn_backward(device, R, Cc, accumulate, off=0, seed=141):
    """fsv_sn_backward: dW (+)= (dWsn - (<dWsn, W> / sigma) u v^T) / sigma, `bounded` against fp64 (restatement: the same formula
    in fp32 torch, the dot as torch.sum of the products).  accumulate = 0 starts from a NaN-filled dW; the words in front of and
    behind dW, the inputs and the words around the 256 partial sums keep their bits.  Returns (result, fp64 reference, fp32
    restatement, inputs)."""
    L = lib()
    g = torch.Generator().manual_seed(seed + 31 * R + Cc + 2 * off + accumulate)
    h = _sn_inputs(g, R, Cc)
    n = R * Cc
    start = h['dW0'] if accumulate else torch.full((R, Cc), NAN)
    dws, w, dw = (_shifted(h[k] if k else start, off, device, g) for k in ('dWsn', 'W', None))
    assert off == 0 or (dws[1].data_ptr() % 16 != 0 and w[1].data_ptr() % 16 != 0 and dw[1].data_ptr() % 16 != 0)
    u, v, sig = (_dev(h[k], device) for k in ('u', 'v', 'sig'))
    part = torch.full((258,), 12345.0, dtype=torch.float64, device=device)
    L.check_device(dws[0], w[0], dw[0])
    L.call('fsv_sn_backward', L.ptr(dws[1]), L.ptr(w[1]), L.ptr(u), L.ptr(v), L.ptr(sig), L.ptr(part[1:]), L.ptr(dw[1]), R, Cc,
           accumulate, L.stream_ptr())
    tag = 'sn_backward R=%d Cc=%d accumulate=%d offset=%d' % (R, Cc, accumulate, off)
    s0 = h['dW0'] if accumulate else torch.zeros(R, Cc)
    (r64, _), (r32, _) = (_sn_formula(s0, h['dWsn'], h['W'], h['u'], h['v'], float(h['sig'][1]), dt) for dt in (torch.float64, torch.float32))
    got = dw[1].cpu().view(R, Cc)
    bounded(tag, got, r64, r32)
    buf, _, before, pad = dw
    same_bits(tag + ': words in front of dW', buf[:pad], before[:pad])
    same_bits(tag + ': words behind dW', buf[pad + n:], before[pad + n:])
    same_bits(tag + ': dWsn', dws[0], dws[2])
    same_bits(tag + ': W', w[0], w[2])
    for k, t in (('u', u), ('v', v), ('sig', sig)):
        same_bits(tag + ': ' + k, t, h[k])
    pc = part.cpu()
    assert float(pc[0]) == 12345.0 and float(pc[-1]) == 12345.0, tag + ': wrote outside part[256]'
    return got, r64, r32, h


def check_sn_backward_vs_finalize(device, R=40, Cc=300, seed=141):
    """the same data through fsv_sn_backward (accumulate = 1) and through a spectral 1x1 job of fsv_wgrad_finalize: each within
    its own bound of the SAME fp64 reference"""
    got, r64, r32, h = check_sn_backward(device, R, Cc, 1, 0, seed)
    g = torch.Generator().manual_seed(seed)
    job = _fin_job(g, device, R, Cc, 0, 1, 1, spectral=True)
    ldw, kpad = job['ldw'], job['kpad']
    dwt, wlay = torch.full((kpad, ldw), NAN), torch.full((kpad, ldw), NAN)
    dwt[:Cc, :R], wlay[:Cc, :R] = h['dWsn'].t(), h['W'].t()
    job.update(G=h['dWsn'].view(R, Cc, 1, 1), W=h['W'].view(R, Cc, 1, 1))
    job['host'] = dict(dwt=dwt, wlay=wlay, u=h['u'], v=h['v'], sig=h['sig'])
    job['dev'] = {k: _dev(t, device) for k, t in job['host'].items()}
    L = lib()
    flat = _dev(h['dW0'].reshape(-1).clone(), device)
    d = job['dev']
    words, tw = _fin_words(job)
    total = Cc * ldw
    td = [v for ch in range((total + 4095) // 4096) for v in (0, ch)]
    ta = [v for a in range((R + 31) // 32) for b in range((Cc + 31) // 32) for v in (0, a, b)]
    tables = (_table([d['dwt'].data_ptr(), d['wlay'].data_ptr(), flat.data_ptr(), d['u'].data_ptr(), d['v'].data_ptr(), d['sig'].data_ptr()],
                     torch.int64, device), _table(words + [0], torch.int32, device), _table(tw, torch.int64, device))
    dots = torch.zeros(1, dtype=torch.float64, device=device)
    tdd, tad = _table(td, torch.int32, device), _table(ta, torch.int32, device)
    L.call('fsv_wgrad_finalize', *[L.ptr(t) for t in tables], L.ptr(dots), 1, L.ptr(tdd), len(td) // 2, L.ptr(tad), len(ta) // 3,
           L.stream_ptr())
    bounded('finalize 1x1 spectral job on the data of sn_backward R=%d Cc=%d' % (R, Cc), flat.view(R, Cc), r64, r32)
    assert got.shape == flat.view(R, Cc).shape


# --------------------------------------------------------------------------- fsv_sn_power_iter / fsv_sn_power_iter_batched
POWER_SHAPES = ((5, 7), (1, 9), (3, 1), (40, 300), (65, 257), (130, 70))    # (65, 257): two 64-row slabs, two 256-column blocks, both ragged


def _power_inputs(R, Cc, seed=142):
    g = torch.Generator().manual_seed(seed + 31 * R + Cc)
    return (torch.randn(R, Cc, generator=g) * 0.1, F.normalize(torch.randn(R, generator=g), dim=0),
            F.normalize(torch.randn(Cc, generator=g), dim=0), g)


def _power_ref(W, u, dtype):
    """one iteration of torch.nn.utils.spectral_norm (SpectralNorm.compute_weight, n_power_iterations = 1) in `dtype`"""
    W, u, eps = W.to(dtype), u.to(dtype), f32(SN_EPS)
    v = F.normalize(torch.mv(W.t(), u), dim=0, eps=eps)
    wv = torch.mv(W, v)
    u = F.normalize(wv, dim=0, eps=eps)
    sigma = torch.dot(u, wv)
    return u, v, sigma.reshape(1), (1.0 / sigma).reshape(1)


def _power_iter(device, W, u, v, training, g, tag):
    """one fsv_sn_power_iter call on copies between guard words, the scratch sized by fsv_sn_scratch_floats, NaN before and
    guarded; -> (u, v, sig) on the host"""
    L = lib()
    R, Cc = W.shape
    n = L.call_status('fsv_sn_scratch_floats', R, Cc)
    assert n == R + Cc * (1 + (R + 63) // 64)
    sbuf, scratch = _guarded(n, device, g)
    scratch.fill_(NAN)
    sbefore = sbuf.clone()
    Wd = _dev(W, device)
    ub, vb, sb = (_guard_copy(t, device, g) for t in (u, v, torch.full((2,), NAN)))
    L.check_device(Wd, sbuf, ub[0], vb[0], sb[0])
    L.call('fsv_sn_power_iter', L.ptr(Wd), L.ptr(ub[1]), L.ptr(vb[1]), L.ptr(scratch), L.ptr(sb[1]), R, Cc, SN_EPS, training,
           L.stream_ptr())
    _guards_untouched(tag + ' scratch', sbuf, sbefore, n)
    for name, (buf, view, before) in (('u', ub), ('v', vb), ('sig', sb)):
        _guards_untouched(tag + ' ' + name, buf, before, view.numel())
    same_bits(tag + ': W', Wd, W)
    return ub[1].cpu().clone(), vb[1].cpu().clone(), sb[1].cpu().clone()


def check_power_iteration(device, R, Cc, training):
    """fsv_sn_power_iter.  training = 1: u, v, sigma and 1 / sigma `bounded` against the fp64 iteration of
    torch.nn.utils.spectral_norm (restatement: the same in fp32).  training = 0: u and v keep their bits, sigma and 1 / sigma
    are `bounded` against u . (W v).  Both: nothing behind the fsv_sn_scratch_floats(R, Cc) scratch floats is written."""
    W, u, v, g = _power_inputs(R, Cc)
    tag = 'power_iter R=%d Cc=%d training=%d' % (R, Cc, training)
    gu, gv, gs = _power_iter(device, W, u, v, training, g, tag)
    if training:
        ref, base = (_power_ref(W, u, dt) for dt in (torch.float64, torch.float32))
        for name, got, r, b in zip(('u', 'v', 'sigma', '1/sigma'), (gu, gv, gs[:1], gs[1:]), ref, base):
            bounded(tag + ' ' + name, got, r, b)
        return
    same_bits(tag + ' u', gu, u)
    same_bits(tag + ' v', gv, v)
    s64 = torch.dot(u.double(), torch.mv(W.double(), v.double())).reshape(1)
    s32 = torch.dot(u, torch.mv(W, v)).reshape(1)
    bounded(tag + ' sigma', gs[:1], s64, s32)
    bounded(tag + ' 1/sigma', gs[1:], 1.0 / s64, 1.0 / s32)


def check_power_iteration_batched(device, shapes=POWER_SHAPES):
    """fsv_sn_power_iter_batched over the six shapes as six layers of one call, tables laid out as ops.SpectralGroup._build does:
    u, v, sig and the snapshot buffer have the bits of six single-layer calls from the same state, the snapshot slices are the
    new u / v, and the guard words around scratch, snapshot and sig keep their bits."""
    L = lib()
    g = torch.Generator().manual_seed(143)
    layers = [_power_inputs(R, Cc)[:3] for R, Cc in shapes]
    singles = [_power_iter(device, W, u, v, 1, g, 'power_iter (single, for batched) %s' % (tuple(W.shape),)) for W, u, v in layers]
    rows, cols = [s[0] for s in shapes], [s[1] for s in shapes]
    t_off, s_off, off = [], [], 0
    for r, c in zip(rows, cols):
        t_off.append(off)
        off += c * (1 + (r + 63) // 64)
        s_off.append(off)
        off += r
    u_off, v_off, off2 = [], [], 0
    for r, c in zip(rows, cols):
        u_off.append(off2)
        off2 += r
        v_off.append(off2)
        off2 += c
    tmap_t, tmap_s = [], []
    for li, (r, c) in enumerate(zip(rows, cols)):
        tmap_t += [v for t in range(((c + 255) // 256) * ((r + 63) // 64)) for v in (li, t)]
        tmap_s += [v for grp in range((r + 3) // 4) for v in (li, grp)]
    Wd = [_dev(W, device) for W, _, _ in layers]
    ub = [_guard_copy(u, device, g) for _, u, _ in layers]
    vb = [_guard_copy(v, device, g) for _, _, v in layers]
    sbuf, scratch = _guarded(off, device, g)
    scratch.fill_(NAN)
    nbuf, snap = _guarded(off2, device, g)
    snap.fill_(NAN)
    gbuf, sig = _guarded(2 * len(shapes), device, g)
    before = [b.clone() for b in (sbuf, nbuf, gbuf)]
    i64 = lambda vals: _table(vals, torch.int64, device)                         # noqa: E731
    i32 = lambda vals: _table(vals, torch.int32, device)                         # noqa: E731
    tables = [i64([t.data_ptr() for t in Wd]), i64([b[1].data_ptr() for b in ub]), i64([b[1].data_ptr() for b in vb]), i32(rows),
              i32(cols), i32(t_off), i32(s_off)]
    tail = [i32(u_off), i32(v_off)]
    tt, ts = i32(tmap_t), i32(tmap_s)
    L.check_device(sbuf, nbuf, gbuf, *Wd)
    L.call('fsv_sn_power_iter_batched', *[L.ptr(t) for t in tables], L.ptr(scratch), off, L.ptr(sig), L.ptr(snap),
           *[L.ptr(t) for t in tail], len(shapes), L.ptr(tt), len(tmap_t) // 2, L.ptr(ts), len(tmap_s) // 2, SN_EPS, L.stream_ptr())
    _guards_untouched('power_iter batched scratch', sbuf, before[0], off)
    _guards_untouched('power_iter batched snapshot', nbuf, before[1], off2)
    _guards_untouched('power_iter batched sig', gbuf, before[2], 2 * len(shapes))
    snap_h, sig_h = snap.cpu(), sig.cpu()
    assert bool(torch.isfinite(snap_h).all()), 'a snapshot cell was not written'
    for li, ((r, c), (su, sv, ss)) in enumerate(zip(shapes, singles)):
        tag = 'power_iter batched layer %d R=%d Cc=%d ' % (li, r, c)
        _guards_untouched(tag + 'u', ub[li][0], ub[li][2], r)
        _guards_untouched(tag + 'v', vb[li][0], vb[li][2], c)
        same_bits(tag + 'u', ub[li][1], su)
        same_bits(tag + 'v', vb[li][1], sv)
        same_bits(tag + 'sig', sig_h[2 * li:2 * li + 2], ss)
        same_bits(tag + 'snapshot of u', snap_h[u_off[li]:u_off[li] + r], su)
        same_bits(tag + 'snapshot of v', snap_h[v_off[li]:v_off[li] + c], sv)
        same_bits(tag + 'W', Wd[li], layers[li][0])
