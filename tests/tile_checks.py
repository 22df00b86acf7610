"""Forced-tile parity of the fp32 gather-GEMM and weight-gradient kernels: every tile the launcher instantiates (the plan only
ever picks a few per shape) against F.conv2d on ragged geometries - partial row / column tiles, K not a multiple of 32, taps
that leave the image, split-K with atomics, stride 2, per-sample weights.  Shared by test_tiles_emu.py (SIMT emulator) and the
GPU suite; `python tests/tile_checks.py` runs it on cuda:0."""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import op_checks as oc  # noqa: E402

# (n, cin, h, w, cout, k, stride, pad)
GEOMS = [(2, 8, 9, 11, 40, 3, 1, 1),          # K = 72 (tail chunk), ragged M and N
         (1, 36, 7, 5, 130, 3, 1, 1),         # Cin not a multiple of 32: a chunk spans two taps; N > 128
         (2, 64, 6, 6, 64, 1, 1, 0),          # 1x1
         (1, 16, 10, 9, 33, 4, 2, 2),         # discriminator geometry (k4 s2 p2)
         (1, 4, 13, 12, 96, 3, 1, 1),         # Cin = 4: eight taps per chunk
         (3, 32, 1, 40, 64, 1, 1, 0),         # one image row (nn.Linear as a 1x1 convolution): 32-pixel steps cross images
         (2, 8, 3, 5, 64, 3, 1, 1)]           # 15 pixels per image: the weight-gradient kernel's scalar-twin geometry
FWD_TILES = (0, 1, 2, 4, 9)
# force_tile-only variants that the launch plan never picks (prefetch distance 2, csrc/conv_igemm.hip): checked on the emulator
# only until they have been measured on hardware; (variant, the plan's tile with the same dimensions)
# kernel variants of the plan's tile shapes (csrc/conv_igemm.hip fsv_conv_variant): 10 - 12 prefetch distance 2, 13 - 15 the same with
# in-place A fragments, 16 - 18 in-place A fragments on the prefetch-distance-1 tiles; (variant, the base tile of the same shape)
EXPERIMENTAL_FWD_TILES = ((10, 9), (11, 0), (12, 1), (13, 9), (14, 0), (15, 1), (16, 0), (17, 4), (18, 2), (20, 4))
# 21 / 22: global loads straight into LDS; they pair the k of an MFMA step as (k, k + 2) - same products, another order of the fp32
# chain - so they are held to F.conv2d at the kernels' tolerance, not to the base tile's bits
REORDERED_FWD_TILES = (21, 22, 27)
WGRAD_TILES = (0, 1, 2, 3, 4)


def tile_table():
    """id -> (bm, bn, shape, pf, af, mode) of every tile id the library knows (fsv_conv_tile_info)"""
    from importlib import import_module
    oc.pkg()
    return import_module('few-shot-vid2vid_amd.profile').tile_table()


def _fwd_case(device, geom, tile, split, seed):
    ops, conv = oc.pkg()
    n, cin, h, w, cout, k, s, p = geom
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / (cin * k * k) ** 0.5)
    b = torch.randn(cout, generator=g)
    ref = F.leaky_relu(F.conv2d(x, wt, b, stride=s, padding=p), 0.2)
    ge = conv.Geom(k, k, s, p)
    wf, kpad, ldw = conv.prep_weight(wt.to(device), 0, ge)
    nchunks = (k * k * cin + 31) // 32
    y = conv.conv_forward(conv.to_nhwc(x.to(device)), wf, ldw, cout, ge, bias=b.to(device), act=conv.ACT_LRELU,
                          force_tile=tile, force_split=min(split, nchunks))
    oc.assert_close('tile %d split %d %s' % (tile, split, geom), y, ref, 2e-5)


def check_forward_tiles(device, tiles=FWD_TILES, geoms=GEOMS):
    for gi, geom in enumerate(geoms):
        for tile in tiles:
            bn = tile_table()[tile][1]
            if geom[4] < bn // 2 and bn > 32:
                continue                       # a tile twice as wide as the layer: not a configuration the plan can produce
            for split in (1, 3):
                _fwd_case(device, geom, tile, split, 100 + gi)


def check_variant_equals_plan_tile(device, variant, base, geoms=GEOMS, splits=(1, 2, 3, 5)):
    """a variant that only moves the global loads in time must reproduce the plan's tile bit for bit (same fma chains)"""
    ops, conv = oc.pkg()
    for gi, geom in enumerate(geoms):
        n, cin, h, w, cout, k, s, p = geom
        g = torch.Generator().manual_seed(300 + gi)
        x = conv.to_nhwc(torch.randn(n, cin, h, w, generator=g).to(device))
        wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / (cin * k * k) ** 0.5)
        ge = conv.Geom(k, k, s, p)
        wf, kpad, ldw = conv.prep_weight(wt.to(device), 0, ge)
        nchunks = (k * k * cin + 31) // 32
        for split in splits:
            sp = min(split, nchunks)
            a = conv.conv_forward(x, wf, ldw, cout, ge, force_tile=variant, force_split=sp)
            b = conv.conv_forward(x, wf, ldw, cout, ge, force_tile=base, force_split=sp)
            assert torch.equal(a.cpu(), b.cpu()), (variant, base, geom, split)


def check_per_sample(device, tiles=(1, 4, 9)):
    """batch_conv form: one weight matrix per sample (grid.z = sample)"""
    ops, conv = oc.pkg()
    g = torch.Generator().manual_seed(7)
    n, cin, h, w, cout = 3, 16, 9, 10, 72
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(n, cout, cin, 1, 1, generator=g) * 0.2
    ref = torch.cat([F.conv2d(x[i:i + 1], wt[i]) for i in range(n)])
    ge = conv.Geom(1, 1, 1, 0)
    wf, kpad, ldw = conv.prep_weight(wt.to(device), 0, ge)
    for tile in tiles:
        y = conv.conv_forward(conv.to_nhwc(x.to(device)), wf, ldw, cout, ge, per_sample=True, force_tile=tile)
        oc.assert_close('per-sample tile %d' % tile, y, ref, 2e-5)


def check_wgrad_tiles(device, tiles=WGRAD_TILES, geoms=GEOMS):
    ops, conv = oc.pkg()
    for gi, geom in enumerate(geoms):
        n, cin, h, w, cout, k, s, p = geom
        g = torch.Generator().manual_seed(200 + gi)
        x = torch.randn(n, cin, h, w, generator=g)
        wt = torch.zeros(cout, cin, k, k, requires_grad=True)
        y = F.conv2d(x, wt, stride=s, padding=p)
        dy = torch.randn(y.shape, generator=g)
        y.backward(dy)
        ge = conv.Geom(k, k, s, p)
        for tile in tiles:
            for split in (1, 2):
                dw = conv.conv_wgrad(conv.to_nhwc(x.to(device)), conv.to_nhwc(dy.to(device)), ge, (cout, cin, k, k),
                                     force_tile=tile, force_split=split)
                oc.assert_close('wgrad tile %d split %d %s' % (tile, split, geom), dw, wt.grad, 2e-5)


def _status(fn):
    """fsv_status a library call inside fn() fails with (0: it does not fail)"""
    import re
    from importlib import import_module
    oc.pkg()
    try:
        fn()
    except import_module('few-shot-vid2vid_amd.lib').FsvError as e:
        return int(re.search(r'fsv_status (-?\d+)', str(e)).group(1))
    return 0


def _walk_paths(device):
    """the four dispatchers of the fp32 gather-GEMM as name -> (run(tile) -> outputs, F.conv2d references), on the smallest shapes
    that still have a partial tile on both axes (a K tail chunk too where Cin allows); inputs and references are made once"""
    ops, conv = oc.pkg()
    g = torch.Generator().manual_seed(500)

    def problem(n, cin, h, w, cout, k):
        x = torch.randn(n, cin, h, w, generator=g)
        wt = torch.randn(cout, cin, k, k, generator=g) * (1.0 / (cin * k * k) ** 0.5)
        ge = conv.Geom(k, k, 1, k // 2)
        wf, _, ldw = conv.prep_weight(wt.to(device), 0, ge)
        return x, wt, conv.to_nhwc(x.to(device)), wf, ldw, cout, ge

    def single(prob, up=False):
        x, wt, xd, wf, ldw, cout, ge = prob
        ref = F.conv2d(F.interpolate(x, scale_factor=2) if up else x, wt, padding=ge.pad)
        return (lambda tile: [conv.conv_forward(xd, wf, ldw, cout, ge, force_tile=tile, force_split=1, up=up)]), [ref]

    group = [problem(2, 8, 9, 11, 40, 3), problem(1, 16, 5, 7, 136, 1), problem(3, 4, 4, 6, 24, 3)]

    def run_group(tile):
        with conv.launch_group(True, force_tile=tile):
            return [conv.conv_forward(xd, wf, ldw, cout, ge) for _, _, xd, wf, ldw, cout, ge in group]
    return {'plain': single(problem(2, 8, 9, 11, 40, 3)),
            'up': single(problem(1, 8, 3, 5, 40, 3), up=True),
            'group': (run_group, [F.conv2d(x, wt, padding=ge.pad) for x, wt, _, _, _, _, ge in group]),
            'scalar': single(problem(1, 6, 7, 5, 40, 3))}


def check_table_walk(device, ids=None):
    """Every id of the tile-variant table (fsv_conv_tile_info; product library: the knock-out rows of a diagnostic build are wrong
    by construction) forced through the four dispatchers of csrc/conv_igemm.hip - plain float4 launch, folded up-sampling, grouped
    launch, scalar gather: each result against F.conv2d at the kernels' 2e-5 and, unless the row loads straight into LDS (mode 2:
    another order of the fp32 chain), bit-equal to the same unsplit call with the id's shape forced.  ids=None: all of them, then
    check_table_refusals."""
    table = tile_table()
    assert all(table[t[2]][2] == t[2] for t in table.values()), 'every shape is a row that is its own shape'
    paths = _walk_paths(device)
    base = {}
    for tile in sorted(table) if ids is None else ids:
        shape, mode = table[tile][2], table[tile][5]
        for name, (run, refs) in paths.items():
            outs = run(tile)
            for i, (y, ref) in enumerate(zip(outs, refs)):
                oc.assert_close('table walk: id %d, %s launch, problem %d' % (tile, name, i), y, ref, 2e-5)
            if mode != 2:
                if (name, shape) not in base:
                    base[name, shape] = [y.cpu() for y in run(shape)]
                assert all(torch.equal(y.cpu(), b) for y, b in zip(outs, base[name, shape])), (tile, shape, name)
    if ids is None:
        check_table_refusals(device, paths)


def check_table_refusals(device, paths=None):
    """an id that is no row - the gaps between the ids and the one past the last - gets FSV_ERR_BAD_ARG from all four dispatchers"""
    table = tile_table()
    for tile in [t for t in range(max(table) + 2) if t not in table]:
        for name, (run, _) in (paths or _walk_paths(device)).items():
            assert _status(lambda: run(tile)) == -1, 'id %d is no row of the table: the %s launch must refuse it' % (tile, name)


def run_all(device):
    check_table_walk(device)
    check_forward_tiles(device)
    check_per_sample(device)
    check_wgrad_tiles(device)
    # the kernel variants the plan's shapes run as: against F.conv2d and (unsplit: split launches add through atomics, whose
    # order is not reproducible on hardware) bit-equal to the base tile of the same shape
    for variant, base in EXPERIMENTAL_FWD_TILES:
        check_forward_tiles(device, tiles=(variant,))
        check_variant_equals_plan_tile(device, variant, base, splits=(1,))
    check_forward_tiles(device, tiles=REORDERED_FWD_TILES)


if __name__ == '__main__':
    run_all(torch.device('cuda:0'))
    print('TILES_GPU_OK')
