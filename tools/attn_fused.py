"""The streaming few-shot attention (few-shot-vid2vid_amd/csrc/attention.hip, InferenceSession(fused_attention=True)) on one MI355X.

Configuration: fewshot_pose 512x512, B = 1, the C3 flags (--adaptive_spade --warp_ref --spade_combine --remove_face_labels), temporal
branch initialised, seeded synthetic inputs, weights settled by a few training-mode passes - the set-up of tools/attn_band.py.

Per reference count (`--shots`, default 2,3,4) two InferenceSession(keep_references=True) on twin models with the same weights: the
unchanged path (one launch at n_shot 2, query bands under the automatic rule past it) and fused_attention=True.  All sessions
alternate in ONE process in blocks of `--block` steady frames; every frame sits between two device events, one synchronise per
block.  Reported per variant: median and min - max ms / frame, the medians of its blocks, the node census of the captured graph, the
memory the session allocated; per reference count the difference of the two medians, judged by the spread of the unchanged
variant's own block medians, and the largest difference of the generated frame between the two sessions.

The kernel alone at the production shape (B = 1, hw = 128 x 128, C = C0 = C1 = 128, both maps in one launch, with the masses):
`--kernel_iters` calls between two device events after a warm-up, per reference count, in TFLOP/s (2 N hw^2 (C + C0 + C1) FLOP)
against the 157.3 TFLOP/s fp32-matrix peak.

python tools/attn_fused.py [--frames 100] [--block 25] [--size 512] [--shots 2,3,4] [--kernel_iters 20] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--block', type=int, default=25)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--shots', default='2,3,4')
    ap.add_argument('--kernel_iters', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the result as JSON to this file')
    args = ap.parse_args()
    import bench
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    M = import_module('few-shot-vid2vid_amd.model')
    ops = import_module('few-shot-vid2vid_amd.ops')
    dev = torch.device('cuda:0')
    size = args.size
    for k in ('FSV_ATTN_BAND_MB', 'FSV_ATTN_FUSED'):
        os.environ.pop(k, None)
    shots = [int(k) for k in args.shots.split(',') if k]
    side = size >> 2                   # n_downsample_A = 2
    res = dict(config='fewshot_pose %dx%d B=1 C3 flags, temporal, kept session, seeded synthetic inputs' % (size, size))

    # ---- the kernel alone -------------------------------------------------------------------------------------------------------------
    res['kernel'] = []
    hw, c = side * side, 128
    for n in shots:
        g = torch.Generator().manual_seed(n)
        cl = dict(memory_format=torch.channels_last)
        key = torch.randn(n, c, side, side, generator=g).to(dev).contiguous(**cl)
        query = torch.randn(1, c, side, side, generator=g).to(dev).contiguous(**cl)
        vals = [torch.randn(n, c, side, side, generator=g).to(dev).contiguous(**cl) for _ in range(2)]
        with torch.no_grad():
            for _ in range(3):
                ops.attention_fused(query, key, vals, n)
            torch.cuda.synchronize()
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.kernel_iters + 1)]
            evs[0].record()
            for i in range(args.kernel_iters):
                ops.attention_fused(query, key, vals, n)
                evs[i + 1].record()
            torch.cuda.synchronize()
        ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.kernel_iters)]
        flop = 2.0 * n * hw * hw * 3 * c
        med = statistics.median(ms)
        res['kernel'].append(dict(n_shot=n, shape='B=1 hw=%dx%d C=C0=C1=%d, masses' % (side, side, c), median_ms=round(med, 3),
                                  min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), tflops=round(flop / med / 1e9, 1),
                                  of_fp32_matrix_peak=round(flop / med / 1e9 / PEAK_TFLOPS, 3)))
        print('kernel alone, n_shot %d: %.3f ms' % (n, med), file=sys.stderr, flush=True)
        del key, query, vals

    # ---- kept sessions: the unchanged path and the fused one ----------------------------------------------------------------------------
    def refs_of(n, seed):
        ds = [bench.make_data(1, size, seed + 100 * k, dev) for k in range(n)]
        return torch.cat([d[4] for d in ds], dim=1), torch.cat([d[5] for d in ds], dim=1)

    labels = [M.encode_label(bench.build_opt(size, 1, workload='pose'), bench.make_data(1, size, 100 + t, dev)[0]) for t in range(8)]
    variants, sessions, runs, info, frames8 = [], [], [], [], []
    for n in shots:
        state = None
        for fused in (False, True):
            opt = bench.build_opt(size, 1, workload='pose')
            opt.n_shot = n
            torch.manual_seed(1)
            model = M.create_model(opt).to(dev)
            model.init_temporal_model()
            model = model.to(dev)
            data = list(bench.make_data(1, size, 7, dev))
            data[4], data[5] = refs_of(n, 7)
            if state is None:
                with torch.no_grad():
                    for _ in range(3):
                        model(data, mode='generator')
                state = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
            model.netG.load_state_dict(state)
            model.eval()
            opt.isTrain = False
            model.isTrain = False
            ref_l, ref_i = M.encode_label(opt, data[4]), data[5]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            s = model.inference_session(warmup=2, keep_references=True, fused_attention=fused)
            s.keep_graph = True
            run = lambda t, s=s, ref_l=ref_l, ref_i=ref_i: s(labels[t % len(labels)], ref_l, ref_i)
            for t in range(8):               # frame 0, the warm-up frames, the capture, first replays
                out = run(t)
            torch.cuda.synchronize()
            frames8.append(out[0].detach().clone())
            name = 'n_shot %d, %s' % (n, 'fused' if fused else 'unchanged path')
            variants.append((name, n, fused))
            info.append(dict(peak_extra_GiB=round((torch.cuda.max_memory_allocated() - base) / 2.0 ** 30, 2),
                             attention_GiB=round(n * side ** 4 * 4 / 2.0 ** 30, 2)))
            sessions.append(s)
            runs.append(run)
            print('%s: captured (%s)' % (name, s.launch_mode()), file=sys.stderr, flush=True)

    per_frame = [[] for _ in variants]
    per_block = [[] for _ in variants]
    done, t = 0, 9
    while done < args.frames:
        for k in range(len(variants)):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.block + 1)]
            evs[0].record()
            for i in range(args.block):
                runs[k](t + i)
                evs[i + 1].record()
            torch.cuda.synchronize()
            ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.block)]
            per_frame[k] += ms
            per_block[k].append(statistics.median(ms))
        done += args.block
        t += args.block
    res.update(frames=done, block=args.block, variants=[], comparison=[])
    for k, (name, n, fused) in enumerate(variants):
        s = sessions[k]
        res['variants'].append(dict(
            name=name, n_shot=n, fused_attention=fused, median_ms=round(statistics.median(per_frame[k]), 3),
            min_ms=round(min(per_frame[k]), 3), max_ms=round(max(per_frame[k]), 3),
            block_medians_ms=[round(x, 3) for x in per_block[k]], graph_nodes=s.graph_nodes(), launch=s.launch_mode(),
            captures=s.n_captures, capture_failures=s.capture_failures, **info[k]))
    for k in range(0, len(variants), 2):
        u, f = res['variants'][k], res['variants'][k + 1]
        spread = max(u['block_medians_ms']) - min(u['block_medians_ms'])
        d = f['median_ms'] - u['median_ms']
        a, b = frames8[k].double(), frames8[k + 1].double()
        res['comparison'].append(dict(
            n_shot=u['n_shot'], unchanged_ms=u['median_ms'], fused_ms=f['median_ms'], unchanged_block_spread_ms=round(spread, 3),
            verdict=('fused slower by %.3f ms' % d if d > spread else 'fused faster by %.3f ms' % -d if d < -spread
                     else 'within the unchanged variant\'s spread'),
            frame_max_abs_difference=float((a - b).abs().max()), frame_range=float(a.abs().max())))
    for s in sessions:
        s.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
