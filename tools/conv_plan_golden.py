"""Record what the fp32 gather-GEMM planners decide (csrc/conv_igemm.hip fsv_conv_plan / fsv_conv_group_plan) into
tests/golden/conv_plan.json; tests/test_tiles_emu.py holds the library to the record.  Both planners are host code, so the
emulator build answers exactly as the product does.  Run with no FSV_* variable set:

    python tools/conv_plan_golden.py            # rewrites the fixture: only when a plan is MEANT to change

Rows: every (M, N, K, z) shape of the pose-512 and street-1024x512 steps (the detail labels of profiles/r06_shape_profile_*.jsonl),
a grid over ragged and threshold sizes, forced tiles / splits on a thinner grid, and groups of 2, 5 and 17 problems."""
import itertools
import json
import os
import random
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['FSV2V_EMU'] = '1'
OUT = os.path.join(ROOT, 'tests', 'golden', 'conv_plan.json')
PROFILES = ('r06_shape_profile_pose_one_stream.jsonl', 'r06_shape_profile_street_amp.jsonl')
COUTS, MZS, CHUNKS, NSAMPS = (3, 8, 32, 33, 64, 65, 128, 512), (15, 128, 129, 1089, 8192, 262144), (1, 7, 8, 16, 72), (1, 2)
FORCED_TILES, FORCED_SPLITS = (-1, 0, 4, 9, 13, 21), (0, 1, 3)


def step_shapes():
    """(Mz, Cout, nchunks, nsamp) of every gather-GEMM launch the shape profiles of the two measured steps name"""
    shapes = set()
    for name in PROFILES:
        with open(os.path.join(ROOT, 'profiles', name)) as f:
            for line in f:
                m = re.search(r'conv\w*_kernel<[^>]*> M(\d+) N(\d+) K(\d+) z(\d+)', json.loads(line)['kernel'])
                if m:
                    mz, n, k, z = map(int, m.groups())
                    shapes.add((mz, n, k // 32, z))
    return sorted(shapes)


def main():
    assert not [k for k in os.environ if k.startswith('FSV_')], 'mint with no FSV_* variable set'
    import fsv2v_amd  # noqa: F401
    from importlib import import_module
    import_module('few-shot-vid2vid_amd.build').build_emu()
    conv = import_module('few-shot-vid2vid_amd.conv')
    steps = step_shapes()
    cases = [s + (-1, 0) for s in steps]
    cases += [(mz, co, ch, z, -1, 0) for co, mz, ch, z in itertools.product(COUTS, MZS, CHUNKS, NSAMPS)]
    cases += [(mz, co, ch, 1, ft, fs) for co, mz, ch in itertools.product((3, 33, 512), (129, 8192), (7, 72))
              for ft, fs in itertools.product(FORCED_TILES, FORCED_SPLITS) if (ft, fs) != (-1, 0)]
    cases = sorted(set(cases))
    plan = [list(c) + list(conv.planned(*c)) for c in cases]
    rng = random.Random(0)
    pool = [(mz, co, ch, z) for co, mz, ch, z in itertools.product(COUTS, MZS[:5], CHUNKS, NSAMPS)] + steps
    groups = []
    for n in (2, 5, 17):
        for cap in (32, 64, 1 << 30):              # the widest problem decides which tiles are candidates
            narrow = [s for s in pool if s[1] <= cap]
            for _ in range(6):
                g = [list(rng.choice(narrow)) for _ in range(n)]
                groups.append([g, conv.group_planned(g)])
    with open(OUT, 'w') as f:
        f.write('{"plan_columns": ["Mz", "Cout", "nchunks", "nsamp", "force_tile", "force_split", "tile", "nsplit"],\n "plan": [\n')
        f.write(',\n'.join('  ' + json.dumps(r) for r in plan))
        f.write('\n ],\n "group_columns": [["Mz", "Cout", "nchunks", "nsamp"], "tile"],\n "groups": [\n')
        f.write(',\n'.join('  ' + json.dumps(r) for r in groups))
        f.write('\n ]\n}\n')
    print('%s: %d plan rows (%d step shapes), %d groups' % (OUT, len(plan), len(steps), len(groups)))


if __name__ == '__main__':
    main()
