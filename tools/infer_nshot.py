"""The kept reference side of n_shot > 1 sequences against the per-frame reference encoding on one MI355X
(few-shot-vid2vid_amd/infer.py `keep_references`, `inputs_u8`).

Configuration: fewshot_pose 512x512, B = 1, the C3 flags (--adaptive_spade --warp_ref --spade_combine --remove_face_labels) plus
--n_shot 2, temporal branch initialised, seeded synthetic inputs, weights settled by a few training-mode passes, the SAME state in every
variant.

Variants: eager `model.inference()`, InferenceSession (the reference encoders, the key encoder and the operand re-arrangements stay in
the per-frame graph), + keep_references, + keep_references + inputs_u8 + frames_u8 (uint8 frames in and out: the inputs are converted
on the device, the uint8 frame is what is copied to the host).  They alternate in ONE process in blocks of `--block` frames after
warm-up, `--frames` steady frames each; every frame sits between two device events, one synchronise per block.  Reported per variant:
median and min - max ms / frame, the medians of its blocks (their spread is the run-to-run noise a comparison has to clear), the
relative L2 distance of the eighth frame's image to the eager variant's, the node census of the captured graph, and the size of the
attention tensor.  Verdict: the kept session against the unkept one, by the spread of the unkept variant's own block medians.

python tools/infer_nshot.py [--frames 200] [--block 25] [--size 512] [--n_shot 2] [--out FILE.json]"""
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
    ap.add_argument('--n_shot', type=int, default=2)
    ap.add_argument('--out', default=None, help='also write the result as JSON to this file')
    args = ap.parse_args()
    import bench
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    M = import_module('few-shot-vid2vid_amd.model')
    infer = import_module('few-shot-vid2vid_amd.infer')
    ops = import_module('few-shot-vid2vid_amd.ops')
    dev = torch.device('cuda:0')
    b, size, n = args.batch, args.size, args.n_shot

    def refs_of(seed):
        """[B, n_shot, C, H, W] references: n_shot seeded draws of the benchmark's data"""
        ds = [bench.make_data(b, size, seed + 100 * k, dev) for k in range(n)]
        return torch.cat([d[4] for d in ds], dim=1), torch.cat([d[5] for d in ds], dim=1)

    def build():
        opt = bench.build_opt(size, b, workload='pose')
        opt.n_shot = n
        torch.manual_seed(1)
        model = M.create_model(opt).to(dev)
        model.init_temporal_model()
        return opt, model.to(dev)
    opt, first = build()
    data = list(bench.make_data(b, size, 7, dev))
    data[4], data[5] = refs_of(7)
    with torch.no_grad():
        for _ in range(3):
            first(data, mode='generator')
    state = {k: v.detach().clone() for k, v in first.netG.state_dict().items()}

    def to_u8(x):                      # [..., C, H, W] in [-1, 1] -> [..., H, W, C] bytes
        return ops.image_u8(x.reshape((-1,) + tuple(x.shape[-3:]))).reshape(tuple(x.shape[:-3]) + (x.shape[-2], x.shape[-1], x.shape[-3]))
    # every variant sees the frames a uint8 pipeline delivers: the bytes, or their conversion
    labels8 = [to_u8(M.encode_label(opt, bench.make_data(b, size, 100 + t, dev)[0])) for t in range(8)]
    ref_l8, ref_i8 = to_u8(M.encode_label(opt, data[4])), to_u8(data[5])
    labels = [ops.image_from_u8(x) for x in labels8]
    ref_l, ref_i = ops.image_from_u8(ref_l8), ops.image_from_u8(ref_i8)

    names = ['eager', 'session', 'session+keep_references', 'session+keep_references+inputs_u8+frames_u8']
    kws = [None, {}, dict(keep_references=True), dict(keep_references=True, inputs_u8=True, frames_u8=True)]
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
            runs.append(lambda t, m=m: m.inference(labels[t], ref_l, ref_i))
        else:
            s = infer.InferenceSession(m, o, warmup=2, **kw)
            s.keep_graph = True
            sessions.append(s)
            if kw.get('inputs_u8'):
                runs.append(lambda t, s=s: s(labels8[t], ref_l8, ref_i8))
            else:
                runs.append(lambda t, s=s: s(labels[t], ref_l, ref_i))

    host = {}

    def frame(k, t):
        out = runs[k](t % len(labels))
        u8 = getattr(out, 'image_u8', None)
        src = u8 if u8 is not None else out[0]
        if k not in host:
            host[k] = torch.empty(src.shape, dtype=src.dtype, pin_memory=True)
        host[k].copy_(src, non_blocking=True)
        return out

    last = []
    for k in range(len(names)):
        for t in range(8):
            out = frame(k, t)
        last.append(out[0].detach().clone())
    torch.cuda.synchronize()
    rel_l2 = [float((x.double() - last[0].double()).norm() / last[0].double().norm()) for x in last]
    nodes = [s.graph_nodes() if s is not None else None for s in sessions]

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
    netG = models[0].netG
    side = size >> netG.n_downsample_A
    hw = side * side
    res = dict(config='fewshot_pose %dx%d B=%d C3 flags + n_shot %d, temporal, seeded synthetic inputs' % (size, size, b, n), frames=done,
               block=args.block, attention_tensor=dict(shape=[b, n * hw, side, side], MiB=round(b * n * hw * hw * 4 / 2 ** 20, 1)),
               variants=[])
    for k, name in enumerate(names):
        s = sessions[k]
        res['variants'].append(dict(
            name=name, median_ms=round(statistics.median(per_frame[k]), 3), min_ms=round(min(per_frame[k]), 3),
            max_ms=round(max(per_frame[k]), 3), block_medians_ms=[round(x, 3) for x in per_block[k]],
            frames_per_s=round(1e3 * b / statistics.median(per_frame[k]), 1), graph_nodes=nodes[k],
            launch=(s.launch_mode() if s is not None else 'eager'), capture_failures=(s.capture_failures if s is not None else None),
            captures=(s.n_captures if s is not None else None), frame7_rel_l2_to_eager=float('%.3e' % rel_l2[k])))
    u = res['variants'][1]
    spread = max(u['block_medians_ms']) - min(u['block_medians_ms'])
    res['unkept_session_block_spread_ms'] = round(spread, 3)
    for v in res['variants'][2:]:
        v['against_unkept_session'] = ('slower' if v['median_ms'] > u['median_ms'] + spread else
                                       'faster' if v['median_ms'] < u['median_ms'] - spread else 'within the unkept spread')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
