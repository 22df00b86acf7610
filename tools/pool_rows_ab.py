"""In-box timing of the pooled-row kernel (csrc/pool_rows.hip, --use_label_ref concat) at the encoder levels of the pose 512x512 B = 2
generator (and street 1024x512 B = 1 with --street), isolated, warm, both forms in the same process:

  new   fsv_pool_rows_fwd / _bwd: NHWC map <-> channel-major rows [B * C, 1024] in one launch each way
  old   the two-launch form it replaces: fsv_adaptive_avgpool_fwd / _bwd (NHWC pooled tensor) + the transposing copy torch runs
        for .reshape(B * C, 1024) forward and for the channels-last gradient backward

Bytes the kernel must move: the map once + the rows once.  Prints one JSON line per level and a sum.
python tools/pool_rows_ab.py [--reps 50] [--street]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

CH = [32, 64, 128, 256, 512, 1024]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--street', action='store_true')
    args = ap.parse_args()
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    ops = import_module('few-shot-vid2vid_amd.ops')
    dev = torch.device('cuda:0')

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    tot = dict(new_fwd_us=0.0, old_fwd_us=0.0, new_bwd_us=0.0, old_bwd_us=0.0)
    for i, c in enumerate(CH):
        b, h, w = (1, 512 >> i, 1024 >> i) if args.street else (2, 512 >> i, 512 >> i)
        g = torch.Generator().manual_seed(i)
        x = torch.randn(b, c, h, w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        drows = torch.randn(b * c, 1024, generator=g).to(dev)
        xg = x.clone().requires_grad_(True)
        rows_new = ops.pool_rows(xg, 32, 32)
        xo = x.clone().requires_grad_(True)
        pooled = ops.adaptive_avgpool(xo, 32, 32)
        rows_old = pooled.reshape(b * c, 1024)
        assert torch.allclose(rows_new, rows_old, rtol=1e-5, atol=1e-6)
        with torch.no_grad():
            nf = timed(lambda: ops.pool_rows(x, 32, 32))
            of = timed(lambda: ops.adaptive_avgpool(x, 32, 32).reshape(b * c, 1024))
        nb = timed(lambda: torch.autograd.grad(rows_new, xg, drows, retain_graph=True))
        ob = timed(lambda: torch.autograd.grad(rows_old, xo, drows, retain_graph=True))
        must = 4.0 * (x.numel() + drows.numel())
        rec = dict(level=i, B=b, C=c, H=h, W=w, must_move_MB=round(must / 1e6, 2),
                   new_fwd_us=round(nf, 1), old_fwd_us=round(of, 1), new_bwd_us=round(nb, 1), old_bwd_us=round(ob, 1),
                   new_fwd_GBps=round(must / nf / 1e3, 1), new_bwd_GBps=round(must / nb / 1e3, 1))
        for k in tot:
            tot[k] += rec[k]
        print(json.dumps(rec), flush=True)
        del x, xg, xo, rows_new, rows_old, pooled
        torch.cuda.empty_cache()
    print(json.dumps(dict(sum_over_levels={k: round(v, 1) for k, v in tot.items()})), flush=True)


if __name__ == '__main__':
    main()
