"""Shared checks of the kept reference side of n_shot > 1 sequences (few-shot-vid2vid_amd/infer.py `keep_references`, `inputs_u8`):
the softmax kernel's per-group sums against float64, fsv_cast_half dir 3 against torch bit for bit, `InferenceSession(
keep_references=True)` against the eager `Vid2VidModel.inference` of a twin model frame for frame, the lifetime of what the session
keeps, and the launch accounting of a kept steady frame.  Used by tests/test_infer_nshot_emu.py (emulator) and
tests/test_infer_nshot_gpu.py (hardware: real captures)."""
import torch

import infer_session_checks as ic
import model_checks as mc

_mod = ic._mod
U = 2.0 ** -24                    # fp32 unit roundoff

# (rows, C, groups): C < 64 with idle lanes / slices of exactly one wave stride / a slice boundary inside a lane stride / slices of one
# element / one group / a row count that is no multiple of the 4 rows per workgroup
GSUM_SHAPES = [(35, 18, 2), (6, 192, 3), (9, 200, 2), (5, 4, 4), (1, 130, 1), (7, 96, 2)]
GSUM_SCALES = ('x1', 'x30', 'dominant')

# tiny configurations: 32 x 32 frames, attention at 8 x 8 (hw = 64 positions per reference), three encoder levels (A = 2 < n = 3: one
# level still runs on the mixed feature)
SMALL = dict(fineSize=32, loadSize=32, n_downsample_G=3, n_adaptive_layers=2)
MUL = dict(ic.NSHOT2, **SMALL)
# seeds: the per-reference attention masses of the key-derived weights are close to 1 / n_shot each; these are seeds whose eager masses
# differ by 3e-3 ... 1e-2 relative on every frame (assert_frames asserts > 1e-3), so an equal ref_idx is not a tie broken by luck
SECOND_SEQUENCE_SEED, FINETUNE_SEED = 437, 418
CONFIGS = {
    'mul': (MUL, 413),
    'concat': (dict(MUL, use_label_ref='concat'), 420),
    'nshot3': (dict(MUL, n_shot=3), 433),
    'inorm': (dict(MUL, norm_G='spectralspadeinstance'), 440),
}


# ------------------------------------------------------------------------------------------------ 1: softmax with group sums
def _gsum_input(rows, c, scale, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, c, generator=g)
    if scale == 'x30':
        x = x * 30
    elif scale == 'dominant':
        x[torch.arange(rows), torch.randint(0, c, (rows,), generator=g)] += 40.0
    return x


def check_softmax_gsum(device, rows, c, groups, scale):
    """y has the bits of the call without gsum; every gsum within L 2^-24 gsum of the float64 sum of the kernel's own y over its slice
    (L = C / groups: the any-order fp32 summation bound); every row of gsum sums to 1 within C 2^-24"""
    ops = _mod('ops')
    x = _gsum_input(rows, c, scale, 17 * rows + c + groups).to(device)
    x4 = x.view(1, rows, 1, c).permute(0, 3, 1, 2)                      # [1, C, rows, 1] on channel-last memory
    y0 = ops.softmax_channels(x4)
    y, mass = ops.softmax_channels(x4, groups=groups)
    assert tuple(mass.shape) == (1, rows, 1, groups) and y.shape == y0.shape
    assert torch.equal(y, y0)
    L = c // groups
    y2 = y.permute(0, 2, 3, 1).reshape(rows, groups, L).double().cpu()
    want = y2.sum(2)
    got = mass.reshape(rows, groups).double().cpu()
    err = (got - want).abs()
    bound = L * U * got
    print('softmax gsum rows %d C %d groups %d %s: max err / bound %.3f, max |row sum - 1| / (C u) %.3f'
          % (rows, c, groups, scale, float((err / bound.clamp_min(1e-300)).max()), float((got.sum(1) - 1).abs().max() / (c * U))))
    assert bool((err <= bound).all()), float((err - bound).max())
    assert bool(((got.sum(1) - 1).abs() <= c * U).all()), float((got.sum(1) - 1).abs().max())
    want_y = torch.softmax(x.double().cpu(), dim=1)
    assert float((y2.reshape(rows, c) - want_y).abs().max()) <= 1e-6


def check_softmax_gsum_bad_args(device):
    """groups that do not divide C (or < 1) with a gsum: FSV_ERR_BAD_ARG, nothing written"""
    lib = _mod('lib')
    bad = lib.ENUMS['FSV_ERR_BAD_ARG']
    x = torch.randn(3, 200).to(device)
    y = torch.zeros_like(x)
    gs = torch.zeros(3, 8, device=device)

    def call(groups, gsum):
        return lib.call_status("fsv_softmax_rows_fwd", lib.ptr(x), lib.ptr(y), 3, 200, groups, lib.ptr(gsum), lib.stream_ptr())
    assert call(7, gs) == bad
    assert call(0, gs) == bad and call(-2, gs) == bad
    assert float(y.abs().max()) == 0.0 and float(gs.abs().max()) == 0.0
    assert call(7, None) == 0 and float(y.abs().max()) > 0.0           # groups is not read without gsum
    assert call(8, gs) == 0 and float(gs.abs().max()) > 0.0
    ops = _mod('ops')
    import pytest
    with pytest.raises(ValueError):
        ops.softmax_channels(x.view(1, 3, 1, 200).permute(0, 3, 1, 2), groups=7)
    xg = x.view(1, 3, 1, 200).permute(0, 3, 1, 2).clone().requires_grad_(True)
    with pytest.raises(ValueError):
        ops.softmax_channels(xg, groups=2)
    ops.softmax_channels(xg).sum().backward()                          # groups=0: today's function, backward included
    assert xg.grad is not None


# ------------------------------------------------------------------------------------------------ 2: uint8 frames in
def _from_u8_torch(x):
    """the dataset's arithmetic, evaluated where the dataset evaluates it: on the host.  (On a device tensor ATen turns the division
    by a scalar into a multiplication by its fp32 reciprocal, which rounds some of the 256 byte values differently: that is not
    ToTensor's v / 255.)"""
    return ((x.cpu().float().div(255) - 0.5) / 0.5).to(x.device)


def check_image_from_u8(device):
    ops = _mod('ops')
    every = torch.arange(256, dtype=torch.uint8).view(1, 1, 256, 1).to(device)           # [N, H, W, C] = [1, 1, 256, 1]
    got = ops.image_from_u8(every)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 1, 1, 256)
    assert torch.equal(got.reshape(-1), _from_u8_torch(every).reshape(-1))
    assert float(got.min()) == -1.0 and float(got.max()) == 1.0
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (2, 9, 7, 6), generator=g, dtype=torch.uint8).to(device)   # 756 bytes: vector body and no tail
    got = ops.image_from_u8(x)
    assert tuple(got.shape) == (2, 6, 9, 7) and got.stride() == (9 * 7 * 6, 1, 7 * 6, 6)   # [N, C, H, W] logical, NHWC storage
    assert torch.equal(got, _from_u8_torch(x).permute(0, 3, 1, 2))
    odd = torch.randint(0, 256, (3, 5, 3), generator=g, dtype=torch.uint8).to(device)     # 45 bytes: a scalar tail
    assert torch.equal(ops.image_from_u8(odd), _from_u8_torch(odd).permute(2, 0, 1))
    again = ops.image_from_u8(torch.flip(x, dims=[0]), out=got)                             # in place, same tensor
    assert again is got and torch.equal(got, _from_u8_torch(torch.flip(x, dims=[0])).permute(0, 3, 1, 2))
    # a generated frame out (ops.image_u8) and in again: within one quantisation step
    img = (torch.rand(2, 3, 9, 7, generator=g) * 2 - 1).to(device).contiguous(memory_format=torch.channels_last)
    back = ops.image_from_u8(ops.image_u8(img))
    assert back.shape == img.shape and float((back - img).abs().max()) <= 2.0 / 255.0
    import pytest
    with pytest.raises(ValueError):
        ops.image_from_u8(img)


def check_from_u8_alignment(device):
    """dir 3 reads 32-bit words and stores float4: a misaligned x or y is FSV_ERR_BAD_ARG (nothing launched), and image_from_u8
    refuses a misaligned `out`"""
    lib, ops = _mod('lib'), _mod('ops')
    import ctypes
    import pytest
    bad = lib.ENUMS['FSV_ERR_BAD_ARG']
    x = torch.zeros(64, dtype=torch.uint8, device=device)
    y = torch.full((36,), 7.0, device=device)
    xp, yp = x.data_ptr(), y.data_ptr()
    assert xp % 4 == 0 and yp % 16 == 0

    def call(xa, ya):
        return lib.call_status("fsv_cast_half", ctypes.c_void_p(xa), ctypes.c_void_p(ya), 32, 3, lib.stream_ptr())
    assert call(xp + 1, yp) == bad and call(xp, yp + 4) == bad
    assert float((y - 7.0).abs().max()) == 0.0
    assert call(xp, yp) == 0 and float(y[:32].max()) == -1.0 and float(y[32:].min()) == 7.0
    with pytest.raises(ValueError, match='aligned'):
        ops.image_from_u8(x[:32].view(2, 4, 4), out=y[1:33].view(2, 4, 4).permute(2, 0, 1))


# ------------------------------------------------------------------------------------------------ session scenarios
def setup_pair(device, kw, scale=1.0):
    opt, twin = ic.tiny_setup(device, scale=scale, **kw)
    _, model = ic.tiny_setup(device, scale=scale, **kw)
    return opt, twin, model


def watch_attention(netG, log):
    """record what the eager attention of `netG` gives per frame: the per-reference masses as the eager path forms them
    (generator.py:366) and the float64 value of atn_vis, from the attention tensor itself"""
    orig = netG.attention_module

    def wrapped(x, label, label_ref, attention=None):
        out, atn, vis = orig(x, label, label_ref, attention)
        if attention is None and not torch.is_grad_enabled():
            b, n = label.shape[0], netG.n_shot
            h, w = atn.shape[2:]
            log.append(dict(mass=atn.reshape(b, n, -1).sum(2).double().cpu(),
                            vis64=atn.double().reshape(b, n, -1, h, w).sum(2)[-1:, 0:1].cpu(), hw=atn.shape[1] // n))
        return out, atn, vis
    netG.attention_module = wrapped
    return orig


def run_eager(twin, seq):
    """-> (frames, ref_idx per frame, attention records per frame)"""
    labels, rl, ri = seq
    log = []
    orig = watch_attention(twin.netG, log)
    try:
        twin.reset_inference()
        outs, idx, per_frame = [], [], []
        for lab in labels:
            outs.append(ic._keep(twin.inference(lab, rl, ri))[0])
            idx.append(twin.netG._atn[1].clone())
            per_frame.append(log[-1])            # (the frame's own pass is the last one: --finetune runs others before it)
    finally:
        del twin.netG.attention_module
    assert twin.netG.attention_module.__func__ is orig.__func__
    return outs, idx, per_frame


def run_session(sess, seq, report=None, refs_after_frame0=None):
    labels, rl, ri = seq
    sess.reset()
    outs, idx, reps, u8s = [], [], [], []
    for t, lab in enumerate(labels):
        if report:
            report()
        r = refs_after_frame0 if (refs_after_frame0 is not None and t > 0) else (rl, ri)
        kept, u8 = ic._keep(sess(lab, r[0], r[1]))
        reps.append(report() if report else None)
        outs.append(kept)
        u8s.append(u8)
        idx.append(sess.model.netG._atn[1].clone())
    return outs, idx, reps, u8s


def assert_frames(eager, got, what, device=None):
    """everything but atn_vis (the last output) bit-equal; ref_idx equal, and not by a tie; atn_vis within hw 2^-24 of the float64
    sum of the (bit-equal) attention tensor"""
    e_out, e_idx, e_log = eager
    s_out, s_idx = got[0], got[1]
    assert len(e_out) == len(s_out)
    for t, (a, b) in enumerate(zip(e_out, s_out)):
        assert len(a) == len(b) == 6
        bad = ic.same_bits(a[:5], b[:5])
        assert not bad, '%s: frame %d, outputs %s differ from the eager path' % (what, t, bad)
        assert torch.equal(e_idx[t], s_idx[t]), (what, t, e_idx[t], s_idx[t])
        top = torch.sort(e_log[t]['mass'], dim=1, descending=True)[0]
        gap = float(((top[:, 0] - top[:, 1]) / top[:, 0]).min())
        vis64, hw = e_log[t]['vis64'], e_log[t]['hw']
        err = (b[5].double().cpu() - vis64).abs()
        print('%s frame %d: relative gap of the two largest reference masses %.2e, atn_vis err / bound %.3f'
              % (what, t, gap, float((err / (hw * U * vis64)).max())))
        assert gap > 1e-3, 'the references tie: ref_idx would be equal by luck (choose another seed)'
        assert b[5].shape == a[5].shape and bool((err <= hw * U * vis64).all()), float(err.max())
        if t == 0:
            assert torch.equal(a[5], b[5])           # frame 0 is the eager path itself


_scen = {}


def scenario(name, device, report=None):
    """ONE run shared by the tests of a configuration: four frames eager on a twin, four through a kept session; on the 'mul'
    configuration also four through an unkept session (the launch counts) and a second sequence on other references"""
    key = (name, str(device))
    r = _scen.get(key)
    if r is None:
        infer = _mod('infer')
        kw, seed = CONFIGS[name]
        opt, twin, model = setup_pair(device, kw)
        seq = ic.tiny_sequence(opt, 4, device, seed)
        sess = infer.InferenceSession(model, opt, warmup=1, keep_references=True)
        sess.keep_graph = device.type == 'cuda'
        eager = run_eager(twin, seq)
        got = run_session(sess, seq, report)
        r = _scen[key] = dict(opt=opt, twin=twin, model=model, seq=seq, sess=sess, eager=eager, got=got, caps=sess.n_captures,
                              nodes=sess.graph_nodes(), graph=sess._graph)
    return r


def check_frames(name, device, report=None):
    """3: four frames of a kept session against the eager path"""
    r = scenario(name, device, report)
    sess = r['sess']
    assert sess.keep_references and sess._kept.ready
    assert all(bool(torch.isfinite(x).all()) for x in ic._flat(r['eager'][0]) if x is not None)
    assert_frames(r['eager'], r['got'], name)
    assert ic.same_bits(r['eager'][0][2], r['eager'][0][3]), 'frames of the sequence must differ'
    ic.assert_captured(sess, device)
    n = len(sess._kept.xmats)
    assert n == (1 if r['opt'].use_label_ref == 'concat' else 2)


def check_fold_norms(device):
    """3: fold_norms=True together with keep_references, against the bar fold_norms has in infer_session_checks (1e-3 of the image's
    range) - here to the eager frames"""
    infer = _mod('infer')
    r = scenario('mul', device)
    kw, _ = CONFIGS['mul']
    _, model = ic.tiny_setup(device, **kw)
    sess = infer.InferenceSession(model, r['opt'], fold_norms=True, warmup=1, keep_references=True)
    assert sess.folded_sites
    outs, idx, _, _ = run_session(sess, r['seq'])
    for t, (a, b) in enumerate(zip(r['eager'][0], outs)):
        rel = ic._rel(b[0].cpu(), a[0].cpu())
        print('fold_norms + keep_references frame %d: %.2e' % (t, rel))
        assert rel <= 1e-3, (t, rel)
        assert torch.equal(idx[t], r['eager'][1][t])
    ic.assert_captured(sess, device)
    sess.close()


def check_inputs_u8(device):
    """3: inputs_u8=True on uint8 bytes == a session fed ops.image_from_u8 of the same bytes; class-index labels refuse"""
    infer, ops = _mod('infer'), _mod('ops')
    kw, seed = CONFIGS['mul']
    opt, a, b = setup_pair(device, kw)
    g = torch.Generator().manual_seed(seed)
    h = opt.fineSize
    labels = [torch.randint(0, 256, (1, 1, h, h, opt.input_nc), generator=g, dtype=torch.uint8).to(device) for _ in range(3)]
    rl = torch.randint(0, 256, (1, opt.n_shot, h, h, opt.input_nc), generator=g, dtype=torch.uint8).to(device)
    ri = torch.randint(0, 256, (1, opt.n_shot, h, h, 3), generator=g, dtype=torch.uint8).to(device)
    for keep in (True, False):
        s8 = infer.InferenceSession(a, opt, warmup=1, keep_references=keep, inputs_u8=True, frames_u8=True)
        sf = infer.InferenceSession(b, opt, warmup=1, keep_references=keep)
        o8, _, _, u8 = run_session(s8, (labels, rl, ri))
        of, _, _, _ = run_session(sf, ([ops.image_from_u8(x) for x in labels], ops.image_from_u8(rl), ops.image_from_u8(ri)))
        for t, (x, y) in enumerate(zip(o8, of)):
            assert not ic.same_bits(x, y), (keep, t)
            assert u8[t] is not None and torch.equal(u8[t], ops.image_u8(y[0]))
        assert ic.same_bits(o8[1], o8[2])
        ic.assert_captured(s8, device)
        s8.close()
        sf.close()
    import pytest
    street = mc.tiny_opt(dataset_mode='fewshot_street', label_nc=20, input_nc=3)
    street.isTrain = False
    with pytest.raises(ValueError, match='label_nc'):
        infer.InferenceSession(a, street, inputs_u8=True)


# ------------------------------------------------------------------------------------------------ 4: lifetime
def check_two_sequences(device):
    """a second sequence on other references through the same session: equal to its own eager run, different from the first; the
    kept buffers were refilled in place and the graph is the same object"""
    r = scenario('mul', device)
    sess, opt = r['sess'], r['opt']
    if 'eager2' not in r:
        seq2 = ic.tiny_sequence(opt, 4, device, SECOND_SEQUENCE_SEED)
        ptrs = [t.data_ptr() for t in [sess._kept.kmat] + sess._kept.xmats]
        r['eager2'] = run_eager(r['twin'], seq2)
        r['got2'] = run_session(sess, seq2)
        r['ptrs'] = (ptrs, [t.data_ptr() for t in [sess._kept.kmat] + sess._kept.xmats])
    assert_frames(r['eager2'], r['got2'], 'mul (second sequence)')
    assert ic.same_bits(r['eager'][0][1], r['eager2'][0][1]), 'the second sequence must differ from the first'
    assert ic.same_bits(r['got'][0][1], r['got2'][0][1])
    assert r['ptrs'][0] == r['ptrs'][1]
    assert sess._graph is r['graph'] and sess.n_captures == r['caps'] and sess.capture_failures == []
    assert sess.graph_nodes() == r['nodes']
    if device.type == 'cuda':
        assert r['caps'] == 1 and r['nodes'] and r['nodes'].get('kernel', 0) > 0


def check_steady_references_are_not_read(device):
    """the documented difference to model.inference(): a kept session reads the references at frame 0 only - other references on
    the steady frames change nothing; the default session follows them"""
    infer = _mod('infer')
    r = scenario('mul', device)
    opt, seq = r['opt'], r['seq']
    other = ic.tiny_sequence(opt, 1, device, CONFIGS['mul'][1] + 23)[1:]
    kw, _ = CONFIGS['mul']
    _, model = ic.tiny_setup(device, **kw)
    kept = infer.InferenceSession(model, opt, warmup=1, keep_references=True)
    outs, _, _, _ = run_session(kept, seq, refs_after_frame0=other)
    for t, (a, b) in enumerate(zip(r['got'][0], outs)):
        assert not ic.same_bits(a[:5], b[:5]), t
    kept.close()
    plain = infer.InferenceSession(model, opt, warmup=1)
    assert not plain.keep_references
    outs, _, _, _ = run_session(plain, seq, refs_after_frame0=other)
    assert not ic.same_bits(r['got'][0][0][:5], outs[0][:5])
    assert ic.same_bits(r['got'][0][2][:5], outs[2][:5]), 'the default session must follow the references of every frame'
    plain.close()


def check_refreeze(device):
    """an in-place weight change + refreeze(): the kept references are dropped, the next call is a frame 0 and the frames follow the
    new weights"""
    infer = _mod('infer')
    kw, seed = CONFIGS['mul']
    opt, twin, model = setup_pair(device, kw)
    seq = ic.tiny_sequence(opt, 3, device, seed)
    sess = infer.InferenceSession(model, opt, warmup=1, keep_references=True)
    old = run_session(sess, seq)
    with torch.no_grad():
        for net in (twin.netG, model.netG):
            for k, p in net.named_parameters():
                if k.startswith(('ref_', 'atn_', 'up_')) and p.dim() > 1:
                    p.mul_(0.9)
    sess.refreeze()
    assert sess.t is None and not sess._kept.ready and sess._kept.kmat is None and sess._graph is None
    labels, rl, ri = seq
    # (no reset(): the call after refreeze() is a frame 0 by itself)
    outs, idx = [], []
    for lab in labels:
        outs.append(ic._keep(sess(lab, rl, ri))[0])
        idx.append(model.netG._atn[1].clone())
    assert sess.t == 2
    assert_frames(run_eager(twin, seq), (outs, idx), 'after refreeze()')
    assert ic.same_bits(old[0][1], outs[1]), 'the new weights must change the frames'
    sess.close()


def check_close(device):
    """close() leaves no session attribute on the model; the eager path then gives the bits of a model that never had a session"""
    infer = _mod('infer')
    r = scenario('mul', device)
    kw, _ = CONFIGS['mul']
    _, model = ic.tiny_setup(device, **kw)
    sess = infer.InferenceSession(model, r['opt'], warmup=1, keep_references=True, fold_norms=True)
    assert model.netG._kept_refs is sess._kept
    run_session(sess, r['seq'])
    sess.close()
    assert not hasattr(model.netG, '_kept_refs')
    assert not [k for m in model.modules() for k in m.__dict__ if 'kept' in k]
    assert model.netG._frozen_x is None
    for m in model.modules():
        assert getattr(m, '_sig_frozen', None) is None and getattr(m, '_fsv_fold', None) is None
    for t in list(model.parameters()) + list(model.buffers()):
        assert not hasattr(t, '_fsv_frozen') and not hasattr(t, '_fsv_frozen_stats')
    outs, _, _ = run_eager(model, r['seq'])
    ic.assert_same_frames(r['eager'][0], outs, 'eager inference after close()')
    # with one reference the flag is a no-op
    opt1, one = ic.tiny_setup(device, temporal=False, **ic.TINY)
    s1 = infer.InferenceSession(one, opt1, keep_references=True)
    assert not s1.keep_references and not hasattr(one.netG, '_kept_refs')
    s1.close()


def check_finetune(device):
    """--finetune with keep_references: the adaptation steps run inside frame 0, before anything is kept.  Two finetune runs do not
    give the same bits (Adam turns rounding-level gradient differences into +-lr steps), so the eager frames are those of the SAME
    model behind the session: with the weights the session's frame 0 left, and --finetune switched off, model.inference() must give
    the session's frames - frame 0 (generated after the adaptation) and the steady ones (from what was kept after it)"""
    import random
    infer = _mod('infer')
    kw = dict(CONFIGS['mul'][0], finetune=True)
    opt, model = ic.tiny_setup(device, **kw)
    opt.finetune_iterations = 2
    seq = ic.tiny_sequence(opt, 3, device, FINETUNE_SEED)
    before = model.netG.conv_img.weight.detach().clone()
    random.seed(7)
    sess = infer.InferenceSession(model, opt, warmup=1, keep_references=True)
    got = run_session(sess, seq)
    assert sess._kept.ready and sess.t == 2
    assert not torch.equal(before, model.netG.conv_img.weight.detach()), 'the adaptation steps did not run'
    owned = [p for p in model.netG.parameters() if getattr(p, '_fsv_cache', None) is not None]
    assert owned and all(not hasattr(p, '_fsv_frozen') for p in owned)
    sess.close()
    opt.finetune = False
    assert_frames(run_eager(model, seq), got, 'finetune')


# ------------------------------------------------------------------------------------------------ 5: launch accounting
FAMILIES = (('convolution', ('fsv_conv', 'fsv_hconv', 'fsv_up_')), ('weight layout', ('fsv_prep_weight',)),
            ('normalisation', ('fsv_norm', 'fsv_colsum')), ('SPADE', ('fsv_spade',)), ('softmax', ('fsv_softmax',)),
            ('spectral', ('fsv_sn_',)))
# profiles/infer_nshot_notes.md: library launches of a steady frame of the 'mul' configuration on the emulator
KEPT_LAUNCHES = 202              # (the unkept session frame recorded next to it: 226)


def by_family(rep):
    out, rest = {}, dict(rep)
    for fam, prefixes in FAMILIES:
        keys = [k for k in rest if k.lstrip('(').startswith(prefixes)]
        out[fam] = sum(rest.pop(k) for k in keys)
    out['other'] = sum(rest.values())
    return out


def check_launch_accounting(device, report):
    """a kept steady frame issues fewer library launches than an unkept session frame, by at least 1 + n_downsample_A convolutions
    (the key encoder alone); the kept count is the one recorded in profiles/infer_nshot_notes.md"""
    infer = _mod('infer')
    r = scenario('mul', device)
    kw, _ = CONFIGS['mul']
    _, model = ic.tiny_setup(device, **kw)
    counts = []
    for flags in (dict(keep_references=True), {}):       # (sessions of this check's own: the shared run may have taken no reports)
        sess = infer.InferenceSession(model, r['opt'], warmup=1, **flags)
        _, _, reps, _ = run_session(sess, r['seq'], report)
        sess.close()
        assert reps[2] == reps[3], 'the frames are not steady'
        counts.append(reps[3])
    kept, unkept = counts
    fk, fu = by_family(kept), by_family(unkept)
    print('library launches per steady frame: kept %d %s' % (sum(kept.values()), fk))
    print('library launches per steady frame: unkept %d %s' % (sum(unkept.values()), fu))
    print('kernels the kept frame does not launch:', {k: v - kept.get(k, 0) for k, v in unkept.items() if v != kept.get(k, 0)})
    A = model.netG.n_downsample_A
    assert fu['convolution'] - fk['convolution'] >= 1 + A, (fu, fk)
    assert sum(kept.values()) < sum(unkept.values())
    assert fk['weight layout'] < fu['weight layout']            # kmat / xmat are not re-arranged per frame
    assert fk['softmax'] == fu['softmax']
    assert sum(kept.values()) == KEPT_LAUNCHES, (sum(kept.values()), sum(unkept.values()))
