"""A/B of the forward of the two DEEP conv3x3(nearest_x2(x)) layers of the bench step (B = 2), in the manner of tools/tile_ab.py:
every form is captured as a hipGraph of 20 back-to-back launches and the forms are replayed interleaved, median of 5, us per call.

  gather        the single 9-tap gather through the up-sampling index (ConvP::up) with the plan's ordered K split: 36 products
  sub tT/sS     fsv_conv_up_subpixel_fwd - the four parity classes as ONE grouped launch + one placed finishing pass, 16 products -
                with tile shape T and split S forced; `sub auto` is its own plan
  4x tT/sS      the same four class GEMMs as four PLAIN launches, each with its own ordered split and finishing pass, into four
                DENSE tensors (timing only: a placed launch cannot split, so this form could not place its result)
Warm: the operands of a layer stay in the caches between its 20 launches; inside the step they are cold."""
import json, os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fsv2v_amd  # noqa
from importlib import import_module
conv = import_module('few-shot-vid2vid_amd.conv')
ops = import_module('few-shot-vid2vid_amd.ops')
dev = torch.device('cuda:0')
SPLITS = tuple(int(t) for t in os.environ.get('FSV_AB_SPLITS', '1,2,4').split(','))
TILES = tuple(int(t) for t in os.environ.get('FSV_AB_TILES', '0,1,4,9').split(','))
shapes = [('M2048 N512 K9216 (source 16x16)', 2, 1024, 16, 16, 512), ('M8192 N256 K9216 (source 32x32)', 2, 1024, 32, 32, 256)]
NREP = 20
for name, n, cin, h, w, cout in shapes:
    x = conv.to_nhwc(torch.randn(n, cin, h, w, device=dev)); wt = torch.randn(cout, cin, 3, 3, device=dev) * 0.01
    b = torch.randn(cout, device=dev)
    g = conv.Geom(3, 3, 1, 1)
    w9, _, ldw9 = conv.prep_weight(wt, 0, g)
    v = ops._tap_sums(wt, ops._SUBPIXEL_ROWS)
    cls = [(ry, rx) for ry in (0, 1) for rx in (0, 1)]
    khs = [2 * ry + iy for ry, rx in cls for iy in (0, 1) for _ in (0, 1)]
    kws = [2 * rx + ix for ry, rx in cls for _ in (0, 1) for ix in (0, 1)]
    wall, _, ldw = conv.prep_weight(v, 0, g, khs, kws, None)
    forms = {'gather': lambda: conv.conv_forward(x, w9, ldw9, cout, g, bias=b, act=conv.ACT_LRELU, up=True),
             'sub auto': lambda: ops._up_subpixel_deep_forward(x, None, cout, b, conv.ACT_LRELU, 1.0, None, cached=(wall, ldw))}
    plans = {'gather': conv.planned(4 * n * h * w, cout, 9 * cin // 32, 1), 'sub auto': ops.up_subpixel_plan(n, h, w, cin, cout)[:2]}

    def four(t, s):
        for c, (ry, rx) in enumerate(cls):
            conv.gather_gemm(x, wall[0, c * 4 * cin:(c + 1) * 4 * cin], ldw, cout, h, w, [ry - 1, ry - 1, ry, ry], [rx - 1, rx, rx - 1, rx],
                             1, 1, bias=b, act=conv.ACT_LRELU, force_tile=t, force_split=s)
    for t in TILES:
        for s in SPLITS:
            forms['sub t%d/s%d' % (t, s)] = (lambda t=t, s=s: ops._up_subpixel_deep_forward(
                x, None, cout, b, conv.ACT_LRELU, 1.0, None, cached=(wall, ldw), force_tile=t, force_split=s))
            forms['4x t%d/s%d' % (t, s)] = (lambda t=t, s=s: four(t, s))
    graphs = {}
    for key, f in forms.items():
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            f(); f()
        torch.cuda.current_stream().wait_stream(s); torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(NREP):
                f()
        graphs[key] = gr
    res = {k: [] for k in graphs}
    for rnd in range(5):
        for k, gr in graphs.items():
            gr.replay(); torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); gr.replay(); e1.record(); torch.cuda.synchronize()
            res[k].append(e0.elapsed_time(e1) / NREP * 1e3)
    print(json.dumps({'case': name, 'unit': 'us per call', 'plans': {k: list(p) for k, p in plans.items()},
                      **{k: round(sorted(u)[len(u) // 2], 1) for k, u in res.items()}}), flush=True)
