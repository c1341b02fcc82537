"""Eval-step time of the flows with fully connected blocks over more than 32 features.

    python tools/bench_widefc.py [--steps 20] [--warmup 3] [--fc-skinny 0] [--out profiles/r13/widefc_new_1.jsonl]

(INFLOW_LIB=<another build's libinflow.so> times that library; --fc-skinny 0 sets INF_OPT_FC_SKINNY to 0 on every engine
net of the flow after its first evaluation has created them, i.e. the generic GEMM chain on this build: §19's A/B.)

  * the CIFAR-10 architecture of run_cifar10.sh (idim 512, n_blocks [2, 2, 2], swish, B = 64) with ``--fc-end True``
    (two fc blocks over the flattened last scale, d = 3072, fc_idim 128) beside the same flow with fc_end False;
  * the tabular flows at d = 43 and d = 63 (4 blocks, 128 x 4, sin), B = 1000.

One density evaluation per step (device probes as bench.py).  One JSON line per flow: ms per step (median and min / max
over the steps) and the engine's launch profile of one step, with the share of the fc blocks' kernels (the wide output
stage 95x and the Broyden update 71x).  The lines also go to --out.  Nothing is compared or asserted.
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

FLOWS = [('cifar10_fc_end', dict(syn.CIFAR10, fc_end=True, fc_idim=128), 64), ('cifar10', syn.CIFAR10, 64),
         ('tab_d43', syn.TAB_D43, 1000), ('tab_d63', syn.TAB_D63, 1000)]


def time_flow(name, arch, B, steps, warmup, fc_skinny=None):
    m = build_flow(arch, B)
    m.load_state_dict(syn.make_state_dict(arch, 0, power_iters=5), strict=True)
    m = m.cuda().eval()
    if arch['kind'] == 'conv':
        x = syn.image_batch(B, input_size=arch['input_size'], nvals=arch['nvals'], seed=0).cuda()
        run = lambda: image_logpx(m, x, arch['nvals'])
    else:
        x = syn.tabular_batch(B, arch['d'], seed=0).cuda()
        run = lambda: tabular_logpx(m, x)
    if fc_skinny is not None:
        run()                                           # creates the engine nets
        for mod in m.modules():
            cache = mod.__dict__.get('_inf_native')
            for n in (cache.values() if isinstance(cache, dict) else ()):
                if isinstance(n, _hip.NativeNet):
                    n.set_option(_hip.INF_OPT_FC_SKINNY, fc_skinny)
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
    wide = sum(s['total_ms'] for s in stats if 950 <= s['tag'] <= 955)
    upd = sum(s['total_ms'] for s in stats if 710 <= s['tag'] <= 716)
    return {
        'flow': name, 'batch': B, 'ms_per_step_median': round(float(np.median(ms)), 3), 'ms_min': round(min(ms), 3),
        'ms_max': round(max(ms), 3), 'loss': round(float(loss), 6), 'fc_out_wide_ms_profiled_step': round(wide, 3),
        'broyden_update_ms_profiled_step': round(upd, 3),
        'top_kernels': [[_hip.tag_name(s['tag']), s['launches'], round(s['total_ms'], 3)] for s in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--fc-skinny', type=int, default=None, choices=[0, 1])
    args = ap.parse_args()
    set_probe_mode('device', seed=0)
    lines = []
    for name, arch, B in FLOWS:
        line = json.dumps(time_flow(name, arch, B, args.steps, args.warmup, args.fc_skinny))
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
