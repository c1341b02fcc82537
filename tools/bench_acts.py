"""Eval-step time of the CIFAR-10 flow per activation, and of the tabular / toy flows with the fused fc activations.

    python tools/bench_acts.py [--batch 64] [--steps 20] [--warmup 3] [--no-fc] [act ...]
    INFLOW_NO_FUSED=1 python tools/bench_acts.py ...      # the same nets on the generic GEMM chain

conv: dict(CIFAR10, act=a) at --batch, one density evaluation per step (image_logpx, device probes as bench.py); act is
one of swish, sin, elu, softplus, relu, and `<act>_nopre` is the same flow with preact=False (no leading activation).
All have fused 3-1-3 kernels; INFLOW_NO_FUSED=1 gives the generic path's time for the fused / generic ratio.
fc: POWER with act in {sin, elu} and TOY with act in {sin, softplus} at B = 10 000 (the fused fc kernels).
One JSON line per net: ms per step (median and min / max over the steps) and the engine's launch profile of one step.
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
from lib.density import image_logpx, tabular_logpx  # noqa: E402
from lib.layers import set_probe_mode  # noqa: E402


def time_net(name, arch, x, steps, warmup):
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, 0, power_iters=5), strict=True)
    m = m.cuda().eval()
    run = (lambda: image_logpx(m, x, arch['nvals'])) if arch['kind'] == 'conv' else (lambda: tabular_logpx(m, x))
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
    print(json.dumps({
        'net': name, 'batch': int(x.shape[0]), 'no_fused': os.environ.get('INFLOW_NO_FUSED', '0'),
        'ms_per_step_median': round(float(np.median(ms)), 3), 'ms_min': round(min(ms), 3), 'ms_max': round(max(ms), 3),
        'loss': round(float(loss), 6),
        'top_kernels': [[_hip.tag_name(s['tag']), s['launches'], round(s['total_ms'], 3)] for s in top]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--fc-batch', type=int, default=10000)
    ap.add_argument('--no-fc', action='store_true', help='conv flows only')
    ap.add_argument('acts', nargs='*', default=['swish', 'sin', 'sin_nopre', 'elu', 'softplus', 'relu'])
    args = ap.parse_args()
    set_probe_mode('device', seed=0)
    for a in args.acts:
        x = syn.image_batch(args.batch, seed=0).cuda()
        nopre = a.endswith('_nopre')
        arch = dict(syn.CIFAR10, act=a[:-len('_nopre')] if nopre else a, preact=not nopre)
        time_net('cifar10_' + a, arch, x, args.steps, args.warmup)
    for base, name, a in ((syn.POWER, 'power', 'sin'), (syn.POWER, 'power', 'elu'), (syn.TOY, 'toy', 'sin'),
                          (syn.TOY, 'toy', 'softplus')) if not args.no_fc else ():
        x = syn.tabular_batch(args.fc_batch, base['d'], seed=0).cuda()
        time_net('%s_%s' % (name, a), dict(base, act=a), x, args.steps, args.warmup)


if __name__ == '__main__':
    main()
