"""The streaming few-shot attention on the f16 matrix cores (few-shot-vid2vid_amd/csrc/attention_h.hip,
InferenceSession(fused_attention='half')) against the fp32 streaming path, on one MI355X, in ONE process.

The kernel alone at the production shape (B = 1, hw = 128 x 128, C = C0 = C1 = 128, both maps in one launch, with the masses), per
reference count (`--shots`, default 2,3,4): fsv_attention_fused_fwd (ops.attention_fused) and fsv_attention_fused_fwd_h
(ops.attention_fused_half on operands prepared once) ALTERNATE call by call, every call between two device events, after a warm-up;
the prep launch (ops.attention_half_prepare) the same way.  Reported: median and min - max ms of each, the ratio of the medians,
and the worst difference of the half outputs and masses to the fp32 kernel's at that real size, relative to each output's range
(the tests stay small: this is the real-size check).

The kept session per frame (fewshot_pose 512x512, B = 1, the C3 flags, temporal branch, seeded synthetic inputs, weights settled by
a few training-mode passes - the set-up of tools/attn_fused.py): InferenceSession(keep_references=True) with fused_attention=True
and with fused_attention='half' on twin models with the same weights, alternating in blocks of `--block` steady frames, every frame
between two device events, one synchronise per block.  Reported per variant: median and min - max ms / frame, the block medians,
the node census of the captured graph; per reference count the difference of the medians, judged by the spread of the fp32
variant's own block medians, and the largest difference of the generated frame.

python tools/attn_half.py [--what kernel,session] [--frames 100] [--block 25] [--size 512] [--shots 2,3,4] [--kernel_iters 20]
                          [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def _timed(fns, iters):
    """the callables alternate; -> [ms per call] per callable, each call between two device events"""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(iters * len(fns) + 1)]
    evs[0].record()
    for i in range(iters):
        for j, fn in enumerate(fns):
            fn()
            evs[i * len(fns) + j + 1].record()
    torch.cuda.synchronize()
    return [[evs[i * len(fns) + j].elapsed_time(evs[i * len(fns) + j + 1]) for i in range(iters)] for j in range(len(fns))]


def _stats(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='kernel,session')
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
    for k in ('FSV_ATTN_BAND_MB', 'FSV_ATTN_FUSED', 'FSV_ATTN_FUSED_HALF'):
        os.environ.pop(k, None)
    shots = [int(k) for k in args.shots.split(',') if k]
    what = args.what.split(',')
    side = size >> 2                   # n_downsample_A = 2
    res = dict(config='fewshot_pose %dx%d B=1 C3 flags, temporal, kept session, seeded synthetic inputs' % (size, size))

    # ---- the kernels alone ---------------------------------------------------------------------------------------------------------
    res['kernel'] = []
    hw, c = side * side, 128
    for n in shots if 'kernel' in what else []:
        g = torch.Generator().manual_seed(n)
        cl = dict(memory_format=torch.channels_last)
        key = torch.randn(n, c, side, side, generator=g).to(dev).contiguous(**cl)
        query = torch.randn(1, c, side, side, generator=g).to(dev).contiguous(**cl)
        vals = [torch.randn(n, c, side, side, generator=g).to(dev).contiguous(**cl) for _ in range(2)]
        with torch.no_grad():
            prepared = ops.attention_half_prepare(key, vals, n)
            f32 = lambda: ops.attention_fused(query, key, vals, n)
            f16 = lambda: ops.attention_fused_half(query, prepared)
            prep = lambda: ops.attention_half_prepare(key, vals, n)
            _timed([f32, f16, prep], 3)
            ms32, ms16, msp = _timed([f32, f16, prep], args.kernel_iters)
            (a0, a1), am = f32()
            (b0, b1), bm = f16()
            torch.cuda.synchronize()
        diff = {name: float((x.double() - y.double()).abs().max() / x.double().abs().max())
                for name, x, y in (('o0', a0, b0), ('o1', a1, b1), ('mass', am, bm))}
        m32, m16 = statistics.median(ms32), statistics.median(ms16)
        res['kernel'].append(dict(n_shot=n, shape='B=1 hw=%dx%d C=C0=C1=%d, masses' % (side, side, c), fp32=_stats(ms32),
                                  half=_stats(ms16), prep=_stats(msp), half_over_fp32=round(m16 / m32, 3),
                                  half_to_fp32_worst_relative_difference=diff))
        print('kernel alone, n_shot %d: fp32 %.3f ms, half %.3f ms, prep %.3f ms, worst difference %s'
              % (n, m32, m16, statistics.median(msp), diff), file=sys.stderr, flush=True)
        del key, query, vals, prepared, a0, a1, am, b0, b1, bm

    # ---- kept sessions: the fp32 streaming attention and the half one ------------------------------------------------------------------
    def refs_of(n, seed):
        ds = [bench.make_data(1, size, seed + 100 * k, dev) for k in range(n)]
        return torch.cat([d[4] for d in ds], dim=1), torch.cat([d[5] for d in ds], dim=1)

    variants, sessions, runs, frames8 = [], [], [], []
    if 'session' in what:
        labels = [M.encode_label(bench.build_opt(size, 1, workload='pose'), bench.make_data(1, size, 100 + t, dev)[0])
                  for t in range(8)]
    for n in shots if 'session' in what else []:
        state = None
        for fused in (True, 'half'):
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
            s = model.inference_session(warmup=2, keep_references=True, fused_attention=fused)
            s.keep_graph = True
            run = lambda t, s=s, ref_l=ref_l, ref_i=ref_i: s(labels[t % len(labels)], ref_l, ref_i)
            for t in range(8):               # frame 0, the warm-up frames, the capture, first replays
                out = run(t)
            torch.cuda.synchronize()
            frames8.append(out[0].detach().clone())
            name = 'n_shot %d, %s' % (n, 'half' if fused == 'half' else 'fp32 streaming')
            variants.append((name, n, fused))
            sessions.append(s)
            runs.append(run)
            kept_half = s._kept.half is not None
            assert kept_half == (fused == 'half'), (name, kept_half)
            print('%s: captured (%s)' % (name, s.launch_mode()), file=sys.stderr, flush=True)

    per_frame = [[] for _ in variants]
    per_block = [[] for _ in variants]
    done, t = 0, 9
    while variants and done < args.frames:
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
            name=name, n_shot=n, fused_attention=fused, block_medians_ms=[round(x, 3) for x in per_block[k]],
            graph_nodes=s.graph_nodes(), launch=s.launch_mode(), captures=s.n_captures, capture_failures=s.capture_failures,
            **_stats(per_frame[k])))
    for k in range(0, len(variants), 2):
        u, f = res['variants'][k], res['variants'][k + 1]
        spread = max(u['block_medians_ms']) - min(u['block_medians_ms'])
        d = f['median_ms'] - u['median_ms']
        a, b = frames8[k].double(), frames8[k + 1].double()
        res['comparison'].append(dict(
            n_shot=u['n_shot'], fp32_ms=u['median_ms'], half_ms=f['median_ms'], fp32_block_spread_ms=round(spread, 3),
            verdict=('half slower by %.3f ms' % d if d > spread else 'half faster by %.3f ms' % -d if d < -spread
                     else 'within the fp32 variant\'s spread'),
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
