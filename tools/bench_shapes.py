"""Eval-step time of the MNIST-shaped flow (1 x 28 x 28: ragged tiles of the fused 3-1-3 kernels), fused and
on the generic GEMM chain, in one call.

    python tools/bench_shapes.py [--batch 64] [--steps 20] [--warmup 3] [--out profiles/r10/bench_shapes.jsonl] [arch ...]

arch: names of lib/synthetic.py CONFIGS, default ``mnist cifar10`` (both idim 512, n_blocks [2, 2, 2]; cifar10 is the
exact-tile yardstick measured beside it on the same machine).  Each arch runs twice: with the fused kernels, then with
INFLOW_NO_FUSED=1 (read when the engine nets are created, so a fresh model per run).  One density evaluation per step
(image_logpx, device probes as bench.py).  One JSON line per run: ms per step (median and min / max over the steps) and
the engine's launch profile of one step; the lines also go to --out.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'implicit-normalizing-flows_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lib import _hip, synthetic as syn  # noqa: E402
from lib.configs import build_flow  # noqa: E402
from lib.density import image_logpx  # noqa: E402
from lib.layers import set_probe_mode  # noqa: E402


def time_net(name, arch, x, steps, warmup, no_fused):
    os.environ['INFLOW_NO_FUSED'] = '1' if no_fused else '0'
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, 0, power_iters=5), strict=True)
    m = m.cuda().eval()
    run = lambda: image_logpx(m, x, arch['nvals'])
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        loss = run()[0]
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    _hip.profile_begin(100000)
    try:
        run()
        torch.cuda.synchronize()
    finally:
        stats = _hip.profile_end()
    top = sorted(stats, key=lambda s: -s['total_ms'])[:6]
    fused_ms = sum(s['total_ms'] for s in stats if 500 <= s['tag'] < 550)
    return {
        'net': name, 'input_size': list(arch['input_size']), 'batch': int(x.shape[0]), 'no_fused': int(no_fused),
        'ms_per_step_median': round(float(np.median(ms)), 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3),
        'bits_per_dim': round(float(loss), 6), 'fused_kernel_ms_profiled_step': round(fused_ms, 3),
        'top_kernels': [[_hip.tag_name(s['tag']), s['launches'], round(s['total_ms'], 3)] for s in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('archs', nargs='*', default=['mnist', 'cifar10'])
    args = ap.parse_args()
    set_probe_mode('device', seed=0)
    lines = []
    for name in args.archs:
        arch = syn.CONFIGS[name]
        x = syn.image_batch(args.batch, input_size=arch['input_size'], nvals=arch['nvals'], seed=0).cuda()
        for no_fused in (False, True):
            line = json.dumps(time_net(name, arch, x, args.steps, args.warmup, no_fused))
            print(line, flush=True)
            lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
