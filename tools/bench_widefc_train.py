"""Training-step time of the tabular flows wider than 16 features.

    python tools/bench_widefc_train.py [--steps 10] [--warmup 3] [--wide-grads 0] [--profile] [--out FILE.jsonl]

The flows of tools/bench_widefc.py at d = 43 and d = 63 (4 blocks, 128 x 4, sin; neumann_grad=False,
grad_in_forward=False as train_tabular.py builds them), B = 1000 (run_tabular.sh), in train mode.  One step is the
forward, the loss and ``loss.backward()``; no optimizer step (its arithmetic is torch's).  Device probes as bench.py; the
series lengths are drawn from numpy's generator seeded with the step's number, so two builds time the same steps.

--wide-grads 0 / 1 sets lib.layers.imblock.WIDE_FC_GRADS where the build has it; a build without the switch (the
parent of §21) takes the nets' gradients from autograd and ignores the option.  INFLOW_LIB=<libinflow.so> times that
library.  --profile adds one profiled step: the launch profile of the stepping thread and, since the profile is per
host thread and autograd runs the backward on its own, of every netgrad call on the thread that makes it; the
weight-gradient kernels' share (tags 8xx) and the generic wgrad_kernel's (890) are summed from both.

One JSON line per flow; the lines also go to --out.  Nothing is compared or asserted.
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
from lib.density import tabular_nats_graph  # noqa: E402
from lib.layers import imblock, netgrad, set_probe_mode  # noqa: E402

FLOWS = [('tab_d43', syn.TAB_D43, 1000), ('tab_d63', syn.TAB_D63, 1000)]
GRAD_CALLS = ('param_grads', 'surrogate_grads', 'logdet_grads')


def profiled_step(step):
    """One step with the launches of both threads recorded -> {tag: [launches, ms]}, netgrad calls made."""
    acc, calls = {}, []

    def add(stats):
        for s in stats:
            a = acc.setdefault(s['tag'], [0, 0.0])
            a[0] += s['launches']
            a[1] += s['total_ms']
    real = {n: getattr(netgrad, n) for n in GRAD_CALLS}

    def spy(name):
        def call(*a, **k):
            calls.append(name)
            _hip.profile_begin(100000)
            try:
                out = real[name](*a, **k)
                torch.cuda.synchronize()
            finally:
                add(_hip.profile_end())
            return out
        return call
    for n in GRAD_CALLS:
        setattr(netgrad, n, spy(n))
    _hip.profile_begin(100000)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        add(_hip.profile_end())
        for n, f in real.items():
            setattr(netgrad, n, f)
    return acc, calls


def time_flow(name, arch, B, steps, warmup, profile):
    m = build_flow(arch, B)
    m.load_state_dict(syn.make_state_dict(arch, 0, power_iters=5), strict=True)
    m = m.cuda().train()
    x = syn.tabular_batch(B, arch['d'], seed=0).cuda()
    state = {'i': 0, 'loss': None, 'n_ps': None}

    def step():
        np.random.seed(1000 + state['i'])
        state['i'] += 1
        for p in m.parameters():
            p.grad = None
        loss, _, _ = tabular_nats_graph(m, x)
        loss.backward()
        state['loss'] = loss
        state['n_ps'] = [b.last_n_power_series for b in m.modules() if isinstance(b, imblock.imBlock)]
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    state['i'] = 0
    ms, n_ps = [], []
    for _ in range(steps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        step()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
        n_ps.append(state['n_ps'])
    blk = next(b for b in m.modules() if isinstance(b, imblock.imBlock))
    out = {'flow': name, 'batch': B, 'ms_per_step_median': round(float(np.median(ms)), 3), 'ms_min': round(min(ms), 3),
           'ms_max': round(max(ms), 3), 'loss_last': round(float(state['loss']), 6),
           'engine_grads': bool(blk._engine_grads(x)), 'series_lengths': n_ps}
    if profile:
        state['i'] = 0
        acc, calls = profiled_step(step)
        total = sum(v[1] for v in acc.values())
        wgrad = sum(v[1] for t, v in acc.items() if 800 <= t < 900)
        top = sorted(acc.items(), key=lambda kv: -kv[1][1])[:12]
        out.update(profiled_step_series_lengths=state['n_ps'], netgrad_calls=len(calls),
                   kernel_ms_profiled_step=round(total, 3), wgrad_ms=round(wgrad, 3),
                   wgrad_kernel_890_ms=round(acc.get(890, [0, 0.0])[1], 3),
                   wgrad_kernel_890_launches=acc.get(890, [0, 0.0])[0],
                   wgrad_by_tag={str(t): [v[0], round(v[1], 3)] for t, v in sorted(acc.items()) if 800 <= t < 900},
                   top_kernels=[[_hip.tag_name(t), v[0], round(v[1], 3)] for t, v in top])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--wide-grads', type=int, default=None, choices=[0, 1])
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    if args.wide_grads is not None and hasattr(imblock, 'WIDE_FC_GRADS'):
        imblock.WIDE_FC_GRADS = bool(args.wide_grads)
    set_probe_mode('device', seed=0)
    lines = []
    for name, arch, B in FLOWS:
        line = json.dumps(time_flow(name, arch, B, args.steps, args.warmup, args.profile))
        print(line, flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
