"""The attention of n_shot > 1 in query bands (few-shot-vid2vid_amd/networks.py attention_band_plan, FSV_ATTN_BAND_MB) on one MI355X.

Configuration: fewshot_pose 512x512, B = 1, the C3 flags (--adaptive_spade --warp_ref --spade_combine --remove_face_labels), temporal
branch initialised, seeded synthetic inputs, weights settled by a few training-mode passes - the set-up of tools/infer_nshot.py.

Variants, each an InferenceSession(keep_references=True) of its own model: n_shot 2 with the attention in one launch (the unbanded
code: the number of profiles/infer_nshot_notes.md), n_shot 2 forced into 2 and into 4 bands (FSV_ATTN_BAND_MB 1024 / 512; the
switch is read while the session's graph is captured, the replays repeat those launches), and `--more` reference counts (3, 4) under
the automatic rule - sizes the unbanded code refuses.  They alternate in ONE process in blocks of `--block` steady frames; every frame
sits between two device events, one synchronise per block.  Reported per variant: median and min - max ms / frame, the medians of its
blocks, the band plan, the node census of the captured graph, peak allocated memory.  Verdict for the forced variants: against the
unbanded one, by the spread of the unbanded variant's own block medians.

`--train_step B`: also ONE eager training iteration (D step + G step, lr as built) at batch B, n_shot 2 (4 GiB of attention at
B = 2: two sample bands, each saved for backward), timed over `--steps` iterations after one warm-up iteration.

python tools/attn_band.py [--frames 100] [--block 25] [--size 512] [--more 3,4] [--train_step 2] [--out FILE.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SWITCH = 'FSV_ATTN_BAND_MB'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=100)
    ap.add_argument('--block', type=int, default=25)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--more', default='3,4', help='reference counts past n_shot 2, under the automatic rule')
    ap.add_argument('--train_step', type=int, default=0, help='batch size of the eager training iteration (0: none)')
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the result as JSON to this file')
    args = ap.parse_args()
    import bench
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    M = import_module('few-shot-vid2vid_amd.model')
    infer = import_module('few-shot-vid2vid_amd.infer')
    net = import_module('few-shot-vid2vid_amd.networks')
    dev = torch.device('cuda:0')
    size = args.size
    os.environ.pop(SWITCH, None)

    def refs_of(b, n, seed):
        ds = [bench.make_data(b, size, seed + 100 * k, dev) for k in range(n)]
        return torch.cat([d[4] for d in ds], dim=1), torch.cat([d[5] for d in ds], dim=1)

    def build(b, n):
        opt = bench.build_opt(size, b, workload='pose')
        opt.n_shot = n
        torch.manual_seed(1)
        model = M.create_model(opt).to(dev)
        model.init_temporal_model()
        return opt, model.to(dev)

    plans = []
    orig_plan = net.attention_band_plan

    def logged_plan(*a):
        plans.append(orig_plan(*a))
        return plans[-1]
    net.attention_band_plan = logged_plan

    side = size >> 2                   # n_downsample_A = 2
    one_sample_mb = lambda n: n * side ** 4 * 4 / 2.0 ** 20
    variants = [('n_shot 2, one launch', 2, None), ('n_shot 2, forced into 2 bands', 2, repr(one_sample_mb(2) / 2)),
                ('n_shot 2, forced into 4 bands', 2, repr(one_sample_mb(2) / 4))]
    variants += [('n_shot %d, automatic rule' % int(k), int(k), None) for k in args.more.split(',') if k]
    labels = [M.encode_label(bench.build_opt(size, 1, workload='pose'), bench.make_data(1, size, 100 + t, dev)[0]) for t in range(8)]
    states, sessions, runs, info = {}, [], [], []
    for name, n, mb in variants:
        opt, model = build(1, n)
        data = list(bench.make_data(1, size, 7, dev))
        data[4], data[5] = refs_of(1, n, 7)
        if n not in states:              # (the settling passes are training-mode passes: banded by the automatic rule where needed)
            with torch.no_grad():
                for _ in range(3):
                    model(data, mode='generator')
            states[n] = {k: v.detach().clone() for k, v in model.netG.state_dict().items()}
        model.netG.load_state_dict(states[n])
        model.eval()
        opt.isTrain = False
        model.isTrain = False
        ref_l, ref_i = M.encode_label(opt, data[4]), data[5]
        s = infer.InferenceSession(model, opt, warmup=2, keep_references=True)
        s.keep_graph = True
        if mb is not None:
            os.environ[SWITCH] = mb
        del plans[:]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run = lambda t, s=s, ref_l=ref_l, ref_i=ref_i: s(labels[t % len(labels)], ref_l, ref_i)
        for t in range(8):               # frame 0, the warm-up frames, the capture, first replays
            run(t)
        torch.cuda.synchronize()
        os.environ.pop(SWITCH, None)
        info.append(dict(plan=plans[-1], peak_extra_GiB=round((torch.cuda.max_memory_allocated() - base) / 2.0 ** 30, 2),
                         attention_GiB=round(n * side ** 4 * 4 / 2.0 ** 30, 2)))
        sessions.append(s)
        runs.append(run)
        print('%s: captured, plan %s' % (name, info[-1]['plan']), file=sys.stderr, flush=True)

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
    res = dict(config='fewshot_pose %dx%d B=1 C3 flags, temporal, kept session, seeded synthetic inputs' % (size, size), frames=done,
               block=args.block, variants=[])
    for k, (name, n, mb) in enumerate(variants):
        s = sessions[k]
        res['variants'].append(dict(
            name=name, n_shot=n, FSV_ATTN_BAND_MB=mb, median_ms=round(statistics.median(per_frame[k]), 3),
            min_ms=round(min(per_frame[k]), 3), max_ms=round(max(per_frame[k]), 3),
            block_medians_ms=[round(x, 3) for x in per_block[k]], graph_nodes=s.graph_nodes(), launch=s.launch_mode(),
            captures=s.n_captures, capture_failures=s.capture_failures, **info[k]))
    u = res['variants'][0]
    spread = max(u['block_medians_ms']) - min(u['block_medians_ms'])
    res['unbanded_block_spread_ms'] = round(spread, 3)
    for v in res['variants'][1:3]:
        v['against_one_launch'] = ('slower by %.3f ms' % (v['median_ms'] - u['median_ms']) if v['median_ms'] > u['median_ms'] + spread
                                   else 'faster by %.3f ms' % (u['median_ms'] - v['median_ms'])
                                   if v['median_ms'] < u['median_ms'] - spread else 'within the unbanded spread')
    for s in sessions:
        s.close()
    del sessions, runs
    torch.cuda.empty_cache()

    if args.train_step:
        b = args.train_step
        opt, model = build(b, 2)
        model = model.train()
        opt_G, opt_D = model.build_optimizers()
        data = list(bench.make_data(b, size, 4321, dev))
        data[4], data[5] = refs_of(b, 2, 4321)
        del plans[:]

        def step():
            M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
            g_losses, _, _ = model(data, mode='generator')
            M.loss_backward(opt, g_losses, opt_G, 0)
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        evs[0].record()
        for i in range(args.steps):
            step()
            evs[i + 1].record()
        torch.cuda.synchronize()
        ms = [evs[i].elapsed_time(evs[i + 1]) for i in range(args.steps)]
        res['train_step'] = dict(config='eager D + G iteration, B=%d, n_shot 2' % b, ms_per_step=[round(x, 2) for x in ms],
                                 median_ms=round(statistics.median(ms), 2), plan=plans[-1] if plans else None,
                                 attention_GiB=round(b * 2 * side ** 4 * 4 / 2.0 ** 30, 2),
                                 peak_allocated_GiB=round(torch.cuda.max_memory_allocated() / 2.0 ** 30, 2))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
