"""Step time of the pose workload (bench.py's flags: 512x512, B = 2, adaptive_spade + warp_ref + spade_combine) with
--use_label_ref concat and, with --adaptive_conv, generated convolutions in the adaptive decoder blocks: D step + G step including
Adam, eager and as a replayed hipGraph.  bench.py itself is not changed: its build_opt is imported and the options are set on the
result.   python tools/adaptive_conv_step.py [--steps 10 --warmup 3] [--use_label_ref concat] [--adaptive_conv]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--use_label_ref', default='concat', help="'mul': the default configuration, for comparison")
    ap.add_argument('--adaptive_conv', action='store_true')
    args = ap.parse_args()
    import bench
    from importlib import import_module
    M = import_module('few-shot-vid2vid_amd.model')
    gs = import_module('few-shot-vid2vid_amd.graph_step')
    dev = torch.device('cuda:0')
    out = dict(workload='pose 512x512 B=2', use_label_ref=args.use_label_ref, adaptive_conv=args.adaptive_conv)
    for graphed in (False, True):
        opt = bench.build_opt(512, 2, workload='pose')
        opt.use_label_ref, opt.adaptive_conv = args.use_label_ref, args.adaptive_conv
        torch.manual_seed(0)
        model = M.create_model(opt).to(dev).train()
        opt_G, opt_D = model.build_optimizers()
        data = bench.make_data(2, 512, 1234, dev, opt)
        step = gs.GraphedIteration(model, opt, warmup=2) if graphed else None

        def one():
            if graphed:
                step(data)
            else:
                M.loss_backward(opt, model(data, mode='discriminator'), opt_D, 1)
                g, _, _ = model(data, mode='generator')
                M.loss_backward(opt, g, opt_G, 0)
        for _ in range(args.warmup + (2 if graphed else 0)):
            one()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(args.steps):
            one()
        torch.cuda.synchronize()
        out['graphed_ms' if graphed else 'eager_ms'] = round((time.time() - t0) * 1e3 / args.steps, 2)
        if graphed:
            out['launch_mode'] = step.launch_mode()
        del model, opt_G, opt_D, step
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
