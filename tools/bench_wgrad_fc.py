"""Per-launch time of the fc nets' weight-gradient contractions at the shapes of a tab_d43 training step.

    python tools/bench_wgrad_fc.py [--reps 7] [--out FILE.jsonl]

One net of the d = 43 tabular flow (tools/bench_widefc_train.py's), batch 1000 (run_tabular.sh).  The calls are the ones
the step makes: inf_net_param_grad over 1000 columns (the recompute gradient) and inf_net_surrogate_grad over
n x 1000 columns for series lengths n = 3, 4, 7 (the forward-over-reverse pass of the series' gradient; 4000 is the one
count divisible by 32).  Each call runs --reps times under the launch profile; per column count one JSON line with, per
weight-gradient tag (8xx, lib/_hip tag_name), the launches of a call and the median over the repetitions of their summed
ms, and the sum over the tags.  Every call also makes one P = 1 dsigma/dW launch per layer on wgrad_kernel (890); where
the data terms run another kernel (the 4000-column call on every build), the 890 entry shows those alone.  The same
script runs on any build (INFLOW_LIB=<libinflow.so> times that library).  Nothing is compared or asserted.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'implicit-normalizing-flows_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lib import _hip, synthetic as syn  # noqa: E402
from lib.configs import build_flow, imblocks  # noqa: E402
from lib.layers import netgrad  # noqa: E402


def surrogate(native, net, x, w, e):
    """inf_net_surrogate_grad as inf_logdet_grad's pass uses it on an fc net: no per-sample value."""
    lib = native.lib
    cols = x.shape[0]
    ng, keep, grads = netgrad._alloc(net)
    gx = torch.empty_like(x)
    ws = _hip.workspace(x.device, lib.inf_grad_workspace_bytes(native.handle, cols))
    _hip.check(lib.inf_net_surrogate_grad(native.handle, _hip.ptr(x), _hip.ptr(w), _hip.ptr(e), None, _hip.ptr(gx),
                                          ctypes.byref(ng), cols, _hip.ptr(ws), ws.numel(), _hip.stream_of(x)),
               'inf_net_surrogate_grad')
    return grads, gx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    arch, B = syn.TAB_D43, 1000
    m = build_flow(arch, B)
    m.load_state_dict(syn.make_state_dict(arch, 0, power_iters=5), strict=True)
    m = m.cuda().train()
    net = imblocks(m)[0].nnet_x
    d = arch['d']
    native = _hip.native_net(net, (d,), torch.device('cuda:0'))
    native.refresh_if_needed(torch.cuda.current_stream().cuda_stream)
    layers = sum(1 for mod in net if hasattr(mod, 'compute_weight'))
    lines = []
    for what, cols in (('param_grad', 1000), ('surrogate_grad', 3000), ('surrogate_grad', 4000),
                       ('surrogate_grad', 7000)):
        x = syn.tabular_batch(cols, d, seed=1).cuda()
        w = syn.tabular_batch(cols, d, seed=2).cuda()
        e = torch.sign(syn.tabular_batch(cols, d, seed=3)).cuda()
        call = ((lambda: netgrad.param_grads(native, net, x, w)) if what == 'param_grad'
                else (lambda: surrogate(native, net, x, w, e)))
        call()
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.reps):
            _hip.profile_begin(20000)
            try:
                call()
                torch.cuda.synchronize()
            finally:
                runs.append({s['tag']: (s['launches'], s['total_ms']) for s in _hip.profile_end() if 800 <= s['tag'] < 900})
        tags = sorted(runs[0])
        by_tag = {str(t): [runs[0][t][0], round(float(np.median([r[t][1] for r in runs])), 4)] for t in tags}
        total = float(np.median([sum(v[1] for v in r.values()) for r in runs]))
        lines.append(json.dumps({'call': what, 'columns': cols, 'layers': layers, 'wgrad_by_tag': by_tag,
                                 'wgrad_ms_per_call_median': round(total, 4),
                                 'wgrad_launches_per_call': sum(v[0] for v in runs[0].values())}))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
