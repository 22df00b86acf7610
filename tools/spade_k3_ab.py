"""In-box timing of the 3x3 SPADE (--spade_ks 3) at the shapes of the pose 512x512 B = 2 and street 1024x512 workloads, isolated, warm:

  fused      fsv_spade_k3_fwd as training runs it (h + the gamma | beta side output the backward reads)
  fused-h    the same launch without the side output (a forward that keeps no graph)
  gemm       the first launch of the two-launch form: the gather-GEMM writing gamma | beta ([P][2C] per map, all maps); the
             element-wise modulation that would follow is NOT counted (a lower bound of the two-launch form)
  bwd-elem   the element-wise backward chain on the stored gamma | beta (the backward the store design runs)

Backward designs: store = bwd-elem + (fused - fused-h); recompute >= gemm + bwd-elem (gamma | beta recomputed by the 9 * Ch-deep
GEMM - a fused twin does the same matrix work).  Prints one JSON line per shape.   python tools/spade_k3_ab.py [--reps 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

PEAK = 157.3e12
SHAPES = [  # (name, n, c, ch list, h, w, up)
    ('pose L0 bn_0/bn_s', 2, 64, [32, 32, 32], 512, 512, 1), ('pose L0 bn_1', 2, 32, [32, 32, 32], 512, 512, 0),
    ('pose L1 bn_0/bn_s', 2, 128, [64, 64, 64], 256, 256, 1), ('pose L1 bn_1', 2, 64, [64, 64, 64], 256, 256, 0),
    ('pose L2 bn_0/bn_s', 2, 256, [128], 128, 128, 1), ('pose L2 bn_1', 2, 128, [128], 128, 128, 0),
    ('street L0 bn_0/bn_s', 1, 64, [32], 512, 1024, 1), ('street L0 bn_1', 1, 32, [32], 512, 1024, 0),
    ('street L1 bn_0/bn_s', 1, 128, [64], 256, 512, 1), ('street L1 bn_1', 1, 64, [64], 256, 512, 0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    ops = import_module('few-shot-vid2vid_amd.ops')
    conv = import_module('few-shot-vid2vid_amd.conv')
    lib = import_module('few-shot-vid2vid_amd.lib')
    import spade_k3_checks as sk
    dev = torch.device('cuda:0')
    real = lib.call

    def timer(names, times):
        def timed(name, *a):
            if name.startswith(names):
                real(name, *a)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    rc = real(name, *a)
                e1.record()
                torch.cuda.synchronize()
                times[name] = times.get(name, 0.0) + e0.elapsed_time(e1) * 1e3 / args.reps
                return rc
            return real(name, *a)
        return timed

    for (label, n, c, chs, h, w, up) in SHAPES:
        x, maps, ws, dy = sk.make_case(n, c, chs, h, w, True, bool(up), 11)
        cl = lambda t: t.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        xd, md = cl(x), [cl(m) for m in maps]
        wd = [tuple(t.to(dev).requires_grad_(True) for t in wt) for wt in ws]
        dyd = dy.to(dev)
        y = ops.spade_mod(xd, md, wd, None, None, act=conv.ACT_LRELU, up=bool(up))      # warm
        y.backward(dyd)
        t_train, t_eval, t_gemm = {}, {}, {}
        lib.call = timer(('fsv_spade_k3_fwd', 'fsv_spade_bwd_elem'), t_train)
        try:
            y = ops.spade_mod(xd, md, wd, None, None, act=conv.ACT_LRELU, up=bool(up))
            y.backward(dyd)
            lib.call = timer(('fsv_spade_k3_fwd',), t_eval)
            with torch.no_grad():
                ops.spade_mod(xd, md, wd, None, None, act=conv.ACT_LRELU, up=bool(up))
            lib.call = timer(('fsv_conv_gather',), t_gemm)
            g3 = conv.Geom(3, 3, 1, 1)
            with torch.no_grad():
                for m, (wg, wb, bg, bb) in zip(md, wd):
                    wt, _, ldw = conv.prep_weight(torch.cat([wg, wb], dim=-4), 0, g3)
                    conv.conv_forward(m, wt, ldw, 2 * c, g3, bias=torch.cat([bg, bb], dim=-1).contiguous(), per_sample=wg.dim() == 5)
        finally:
            lib.call = real
        flops = 2.0 * n * h * w * 2 * c * 9 * sum(chs)
        fused, fused_h = t_train['fsv_spade_k3_fwd'], t_eval['fsv_spade_k3_fwd']
        gemm, belem = sum(t_gemm.values()) or float('nan'), t_train['fsv_spade_bwd_elem']
        rec = dict(shape=label, P=n * h * w, C=c, K='+'.join(map(str, chs)), up=up, gflop=flops / 1e9,
                   fused_us=round(fused, 1), fused_h_us=round(fused_h, 1), gemm_two_launch_lower_bound_us=round(gemm, 1),
                   bwd_elem_us=round(belem, 1), frac_peak_fused_h=round(flops / (fused_h * 1e-6) / PEAK, 3),
                   frac_peak_gemm=round(flops / (gemm * 1e-6) / PEAK, 3),
                   bwd_store_us=round(belem + fused - fused_h, 1), bwd_recompute_lower_bound_us=round(gemm + belem, 1))
        print(json.dumps(rec), flush=True)
        del xd, md, wd, y
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
