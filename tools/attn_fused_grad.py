"""The differentiable streaming few-shot attention (csrc/attention.hip fsv_attention_fused_fwd_lse, csrc/attention_bwd.hip,
FSV_ATTN_FUSED_GRAD) on one MI355X.

(a) The kernels alone at the production shape (B = 1, hw = 128 x 128, C = C0 = C1 = 128, both maps, `--shots` references): the
forward with statistics, then fsv_attention_fused_bwd asked for one gradient group at a time - dq (delta + the query-owning launch +
the sum of its key ranges), dv0 + dv1 (one key-owning launch), dk (delta + the other key-owning launch) - and for all of them;
`--kernel_iters` calls each between two device events after a warm-up.  TFLOP/s counts the FLOP a launch executes, energies and dp
recomputed (units of 2 N hw^2 128: dq 4, dv 3, dk 4, forward 3), against the 157.3 TFLOP/s fp32-matrix peak.

(b) One eager training iteration (D step + G step, lr as built) of fewshot_pose `--size` with the C3 flags, n_shot 2, at every batch
size of `--batches`: the variants `switches off`, `FSV_ATTN_FUSED` and `both` alternate in ONE process on ONE model in blocks of
`--block` iterations (the switches are read per call); every iteration sits between two device events, one synchronise per block.
Reported per variant: median and min - max ms / iteration, the medians of its blocks, torch.cuda.max_memory_allocated over its
blocks; the verdict judges the difference of the medians by the spread of the switch-off variant's own block medians.

python tools/attn_fused_grad.py [--size 512] [--shots 2,3] [--kernel_iters 10] [--batches 1,2] [--steps 24] [--block 8] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_TFLOPS = 157.3
VARIANTS = (('switches off', None, None), ('FSV_ATTN_FUSED', '1', None), ('both', '1', '1'))


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    evs[0].record()
    for i in range(iters):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(iters)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--shots', default='2,3')
    ap.add_argument('--kernel_iters', type=int, default=10)
    ap.add_argument('--batches', default='1,2')
    ap.add_argument('--steps', type=int, default=24)
    ap.add_argument('--block', type=int, default=8)
    ap.add_argument('--out', default=None, help='also write the result as JSON to this file')
    args = ap.parse_args()
    import bench
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    M = import_module('few-shot-vid2vid_amd.model')
    ops = import_module('few-shot-vid2vid_amd.ops')
    lib = import_module('few-shot-vid2vid_amd.lib')
    dev = torch.device('cuda:0')
    size = args.size
    for k in ('FSV_ATTN_BAND_MB', 'FSV_ATTN_FUSED', 'FSV_ATTN_FUSED_GRAD'):
        os.environ.pop(k, None)
    side = size >> 2                   # n_downsample_A = 2
    res = dict(config='fewshot_pose %dx%d, C3 flags, n_shot 2, eager D + G iteration, seeded synthetic inputs' % (size, size))

    # ---- (a) the kernels alone ---------------------------------------------------------------------------------------------------------
    res['kernels'] = []
    hw, c = side * side, 128
    for n in [int(k) for k in args.shots.split(',') if k]:
        g = torch.Generator().manual_seed(n)
        cl = dict(memory_format=torch.channels_last)
        key = (0.25 * torch.randn(n, c, side, side, generator=g)).to(dev).contiguous(**cl)
        query = torch.randn(1, c, side, side, generator=g).to(dev).contiguous(**cl)
        vals = [torch.randn(n, c, side, side, generator=g).to(dev).contiguous(**cl) for _ in range(2)]
        douts = [torch.randn(1, c, side, side, generator=g).to(dev).contiguous(**cl) for _ in range(2)]
        outs = [torch.empty_like(query) for _ in range(2)]
        lse = torch.empty(hw, device=dev)
        mass = torch.empty(hw, n, device=dev)
        nsplit, floats = ops._attention_fused_plan(1, n, hw, c, [c, c], True, 0)
        ws = torch.empty(floats, device=dev)
        bsplit, bfloats = ops._attention_fused_bwd_plan(1, n, hw, c, [c, c], 0)
        bws = torch.empty(bfloats, device=dev)
        dq, dk, dv0, dv1 = torch.empty_like(query), torch.empty_like(key), torch.empty_like(key), torch.empty_like(key)

        def fwd():
            lib.call('fsv_attention_fused_fwd_lse', lib.ptr(query), lib.ptr(key), lib.ptr(vals[0]), lib.ptr(vals[1]), lib.ptr(outs[0]),
                     lib.ptr(outs[1]), lib.ptr(mass), lib.ptr(lse), 1, n, hw, c, c, c, nsplit, lib.ptr(ws), floats, lib.stream_ptr())

        def bwd(a, b, c0, c1):
            lib.call('fsv_attention_fused_bwd', lib.ptr(query), lib.ptr(key), lib.ptr(vals[0]), lib.ptr(vals[1]), lib.ptr(outs[0]),
                     lib.ptr(outs[1]), lib.ptr(douts[0]), lib.ptr(douts[1]), lib.ptr(lse), lib.ptr(a), lib.ptr(b), lib.ptr(c0),
                     lib.ptr(c1), 1, n, hw, c, c, c, bsplit, lib.ptr(bws), bfloats, lib.stream_ptr())
        unit = 2.0 * n * hw * hw * c
        for name, fn, units in (('forward with statistics', fwd, 3), ('backward: dq (%d key ranges)' % bsplit, lambda: bwd(dq, None, None, None), 4),
                                ('backward: dv0 + dv1', lambda: bwd(None, None, dv0, dv1), 3), ('backward: dk', lambda: bwd(None, dk, None, None), 4),
                                ('backward: all four gradients', lambda: bwd(dq, dk, dv0, dv1), 11)):
            ms = timed(fn, args.kernel_iters)
            med = statistics.median(ms)
            res['kernels'].append(dict(n_shot=n, what=name, shape='B=1 hw=%dx%d C=C0=C1=%d' % (side, side, c), median_ms=round(med, 3),
                                       min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), tflops=round(units * unit / med / 1e9, 1),
                                       of_fp32_matrix_peak=round(units * unit / med / 1e9 / PEAK_TFLOPS, 3)))
            print('n_shot %d, %s: %.3f ms' % (n, name, med), file=sys.stderr, flush=True)
        del key, query, vals, douts, outs, ws, bws, dq, dk, dv0, dv1
    torch.cuda.empty_cache()

    # ---- (b) the eager training iteration ----------------------------------------------------------------------------------------------
    res['iteration'] = []
    for b in [int(k) for k in args.batches.split(',') if k]:
        opt = bench.build_opt(size, b, workload='pose')
        opt.n_shot = 2
        torch.manual_seed(1)
        model = M.create_model(opt).to(dev)
        model.init_temporal_model()
        model = model.to(dev).train()
        opt_G, opt_D = model.build_optimizers()
        data = list(bench.make_data(b, size, 4321, dev))
        ds = [bench.make_data(b, size, 4321 + 100 * k, dev) for k in range(2)]
        data[4], data[5] = torch.cat([d[4] for d in ds], dim=1), torch.cat([d[5] for d in ds], dim=1)

        def step():
            M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
            g_losses, _, _ = model(data, mode='generator')
            M.loss_backward(opt, g_losses, opt_G, 0)

        def set_switches(fused, grad):
            for k, v in (('FSV_ATTN_FUSED', fused), ('FSV_ATTN_FUSED_GRAD', grad)):
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        for _, fused, grad in VARIANTS:              # warm-up: every variant once
            set_switches(fused, grad)
            step()
        torch.cuda.synchronize()
        per_step = [[] for _ in VARIANTS]
        per_block = [[] for _ in VARIANTS]
        peak = [0] * len(VARIANTS)
        done = 0
        while done < args.steps:
            for k, (_, fused, grad) in enumerate(VARIANTS):
                set_switches(fused, grad)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.block + 1)]
                evs[0].record()
                for i in range(args.block):
                    step()
                    evs[i + 1].record()
                torch.cuda.synchronize()
                ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.block)]
                per_step[k] += ms
                per_block[k].append(statistics.median(ms))
                peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
            done += args.block
        set_switches(None, None)
        rows = []
        for k, (name, _, _) in enumerate(VARIANTS):
            rows.append(dict(variant=name, median_ms=round(statistics.median(per_step[k]), 2), min_ms=round(min(per_step[k]), 2),
                             max_ms=round(max(per_step[k]), 2), block_medians_ms=[round(x, 2) for x in per_block[k]],
                             max_memory_allocated_GiB=round(peak[k] / 2.0 ** 30, 2)))
        spread = max(per_block[0]) - min(per_block[0])
        verdicts = {}
        for r in rows[1:]:
            d = r['median_ms'] - rows[0]['median_ms']
            verdicts[r['variant']] = ('slower by %.2f ms' % d if d > spread else 'faster by %.2f ms' % -d if d < -spread
                                      else 'within the switch-off variant\'s spread')
        res['iteration'].append(dict(batch=b, steps_per_variant=done, block=args.block, attention_GiB=round(b * 2 * side ** 4 * 4 / 2.0 ** 30, 2),
                                     variants=rows, switch_off_block_spread_ms=round(spread, 2), against_switch_off=verdicts))
        print('B=%d: %s' % (b, [(r['variant'], r['median_ms'], r['max_memory_allocated_GiB']) for r in rows]), file=sys.stderr, flush=True)
        del model, opt_G, opt_D, data, ds
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
