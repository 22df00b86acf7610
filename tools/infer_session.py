"""Frozen-weight inference against the eager test.py path on one MI355X (few-shot-vid2vid_amd/infer.py).

Configuration: fewshot_pose 512x512, B = 1, the C3 flags (--adaptive_spade --warp_ref --spade_combine --remove_face_labels), temporal
branch initialised, seeded synthetic inputs, weights settled by a few training-mode passes (eval-mode statistics and spectral vectors
that are not the initial ones), the SAME state in every variant.

Variants: eager `model.inference()`, InferenceSession, + fold_norms, + fold_norms + frames_u8 (the uint8 frame is copied to the host
in that variant, the fp32 image in the others: what a consumer of the frames pays).  They alternate in ONE process in blocks of
`--block` frames after warm-up, `--frames` steady frames each; every frame sits between two device events, one synchronise per block.
Reported per variant: median and min - max ms / frame over the frames, the medians of its blocks (their spread is the run-to-run
noise the comparison has to clear), the relative L2 distance of the eighth frame's image to the eager variant's (the sums of
split-K launches are not ordered outside FSV_DETERMINISTIC=1, so bit equality is the tests' business, not this tool's), the library calls the host issues for a steady frame (none when a graph is replayed) and the node census of the captured graph (for the eager
variant: of a throw-away capture of the same frame, never replayed).

python tools/infer_session.py [--frames 200] [--block 25] [--size 512] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--block', type=int, default=25)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--batch', type=int, default=1)
    ap.add_argument('--out', default=None, help='also write the result as JSON to this file')
    args = ap.parse_args()
    import bench
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    M = import_module('few-shot-vid2vid_amd.model')
    lib = import_module('few-shot-vid2vid_amd.lib')
    infer = import_module('few-shot-vid2vid_amd.infer')
    dev = torch.device('cuda:0')
    b, size = args.batch, args.size

    def build():
        opt = bench.build_opt(size, b, workload='pose')
        torch.manual_seed(1)
        model = M.create_model(opt).to(dev)
        model.init_temporal_model()
        return opt, model.to(dev)
    opt, first = build()
    data = bench.make_data(b, size, 7, dev)
    with torch.no_grad():
        for _ in range(3):
            first(data, mode='generator')
    state = {k: v.detach().clone() for k, v in first.netG.state_dict().items()}
    labels = [M.encode_label(opt, bench.make_data(b, size, 100 + t, dev)[0]) for t in range(8)]
    ref_l, ref_i = M.encode_label(opt, data[4]), data[5]

    names = ['eager', 'session', 'session+fold_norms', 'session+fold_norms+frames_u8']
    kws = [None, {}, dict(fold_norms=True), dict(fold_norms=True, frames_u8=True)]
    models, runs, sessions = [], [], []
    for name, kw in zip(names, kws):
        o, m = (opt, first) if not models else build()
        m.netG.load_state_dict(state)
        m.eval()
        o.isTrain = False
        m.isTrain = False
        models.append(m)
        if kw is None:
            m.reset_inference()
            sessions.append(None)
            runs.append(lambda lab, m=m: m.inference(lab, ref_l, ref_i))
        else:
            s = infer.InferenceSession(m, o, warmup=2, **kw)
            s.keep_graph = True
            sessions.append(s)
            runs.append(lambda lab, s=s: s(lab, ref_l, ref_i))

    host = {}

    def frame(k, t):
        out = runs[k](labels[t % len(labels)])
        u8 = getattr(out, 'image_u8', None)
        src = u8 if u8 is not None else out[0]
        if k not in host:
            host[k] = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        host[k].copy_(src, non_blocking=True)           # the frame leaves the device: a quarter of the bytes as uint8
        return out

    # warm-up: frame 0, the eager steady frames, the capture and a few replays
    last = []
    for k in range(len(names)):
        for t in range(8):
            out = frame(k, t)
        last.append(out[0].detach().clone())           # every variant has seen the same eight frames: the images are comparable
    torch.cuda.synchronize()
    rel_l2 = [float((x.double() - last[0].double()).norm() / last[0].double().norm()) for x in last]

    # library calls the host issues for a steady frame (torch own kernels are in the node census)
    real_call, real_status = lib.call, lib.call_status
    counts = []
    for k in range(len(names)):
        seen = [0]

        def call(name, *a):
            seen[0] += 1
            return real_call(name, *a)

        def status(name, *a):
            seen[0] += 1
            return real_status(name, *a)
        lib.call, lib.call_status = call, status
        try:
            frame(k, 8)
        finally:
            lib.call, lib.call_status = real_call, real_status
        counts.append(seen[0])
    torch.cuda.synchronize()

    nodes = []
    for k, s in enumerate(sessions):
        if s is not None:
            nodes.append(s.graph_nodes())
            continue
        m = models[k]
        keep_prevs, keep_t = m.prevs, m.t
        try:
            g = torch.cuda.CUDAGraph(keep_graph=True)
            with torch.cuda.graph(g):
                m.inference(labels[0], ref_l, ref_i)
            nodes.append(infer.count_graph_nodes(g))
            del g
        except Exception as ex:          # noqa: BLE001
            nodes.append('capture failed: %s' % str(ex).split('\n')[0][:120])
        m.prevs, m.t = keep_prevs, keep_t
    torch.cuda.synchronize()

    per_frame = [[] for _ in names]
    per_block = [[] for _ in names]
    done, t = 0, 9
    while done < args.frames:
        for k in range(len(names)):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.block + 1)]
            evs[0].record()
            for i in range(args.block):
                frame(k, t + i)
                evs[i + 1].record()
            torch.cuda.synchronize()
            ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.block)]
            per_frame[k] += ms
            per_block[k].append(statistics.median(ms))
        done += args.block
        t += args.block
    res = dict(config='fewshot_pose %dx%d B=%d C3 flags, temporal, seeded synthetic inputs' % (size, size, b), frames=done,
               block=args.block, variants=[])
    for k, name in enumerate(names):
        s = sessions[k]
        res['variants'].append(dict(
            name=name, median_ms=round(statistics.median(per_frame[k]), 3), min_ms=round(min(per_frame[k]), 3),
            max_ms=round(max(per_frame[k]), 3), block_medians_ms=[round(x, 3) for x in per_block[k]],
            frames_per_s=round(1e3 * b / statistics.median(per_frame[k]), 1), host_library_calls_per_frame=counts[k],
            graph_nodes=nodes[k], launch=(s.launch_mode() if s is not None else 'eager'),
            capture_failures=(s.capture_failures if s is not None else None), captures=(s.n_captures if s is not None else None),
            folded_sites=(len(s.folded_sites) if s is not None else None), frame7_rel_l2_to_eager=float('%.3e' % rel_l2[k])))
    e = res['variants'][0]
    spread = max(e['block_medians_ms']) - min(e['block_medians_ms'])
    res['eager_block_spread_ms'] = round(spread, 3)
    for v in res['variants'][1:]:
        v['against_eager'] = ('slower' if v['median_ms'] > e['median_ms'] + spread else
                              'faster' if v['median_ms'] < e['median_ms'] - spread else 'within the eager spread')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
