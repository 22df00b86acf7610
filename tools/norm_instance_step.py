"""Step time of the pose workload (bench.py's flags: 512x512, B = 2, adaptive_spade + warp_ref + spade_combine) with
--norm_G spectralspadeinstance --norm_F spectralinstance next to the default norms in the same run: D step + G step including Adam,
eager and as a replayed hipGraph, and where the normalisation statistics of one eager step came from (producer epilogues finished by
fsv_norm_stats_finish, or reduction launches fsv_norm_stats_fused).  bench.py itself is not changed: its build_opt is imported and the
two options are set on the result.   python tools/norm_instance_step.py [--steps 10 --warmup 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

CONFIGS = {'default': {}, 'instance': dict(norm_G='spectralspadeinstance', norm_F='spectralinstance')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import bench
    from importlib import import_module
    M = import_module('few-shot-vid2vid_amd.model')
    gs = import_module('few-shot-vid2vid_amd.graph_step')
    lib = import_module('few-shot-vid2vid_amd.lib')
    dev = torch.device('cuda:0')
    for name, kw in CONFIGS.items():
        out = dict(workload='pose 512x512 B=2', norms=name, **kw)
        for graphed in (False, True):
            opt = bench.build_opt(512, 2, workload='pose')
            for k, v in kw.items():
                setattr(opt, k, v)
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
            else:
                # one more eager step with the library calls counted by name
                seen, real = {}, lib.call

                def counting(nm, *a):
                    seen[nm] = seen.get(nm, 0) + 1
                    return real(nm, *a)
                lib.call = counting
                try:
                    one()
                    torch.cuda.synchronize()
                finally:
                    lib.call = real
                out['stats_from_epilogues'] = seen.get('fsv_norm_stats_finish', 0)
                out['stats_reduction_launches'] = seen.get('fsv_norm_stats_fused', 0)
                out['library_calls'] = sum(seen.values())
            del model, opt_G, opt_D, step
            torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
