"""A/B on one box: the bench workload (bench.py's model, batch, seeded inputs and weights, device probes, pipelined
readback) under several values of INF_OPT_SERIES_GROUP, the runs alternating in one process.  One JSON line per run,
then a summary line per variant with its min-max spread.

    python tools/ab_series_group.py [--variants off,auto,16] [--blocks 0,1] [--reps 5] [--steps 20] [--warmup 5]
                                    [--batch 64] [--config cifar10] [--dump-outputs DIR]

--variants: off (INF_SERIES_GROUP_OFF, the series as one group), auto (0, the rule inf_series_group) or a forced number
of samples per group.  --blocks: the imBlocks the variant applies to (the others stay ungrouped); empty: all.
Each line also carries ms_blocks: the time of the chosen imBlocks' forwards per step, from device events around them.
--dump-outputs DIR writes each variant's last step (log p per sample, z, bits/dim) as DIR/<variant>/<name>.npy.
INFLOW_LIB=<libinflow.so> runs another build.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(REPO, 'implicit-normalizing-flows_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from lib import _hip, distributed as dd, synthetic as syn  # noqa: E402
from lib.configs import build_flow, imblocks  # noqa: E402
from lib.density import image_logpx  # noqa: E402
from lib.layers import set_probe_mode  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--variants', default='off,auto')
ap.add_argument('--blocks', default='', help='imBlocks (indices) the variant applies to; empty: all')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--config', default='cifar10', choices=['cifar10', 'cifar10_small', 'celebahq256'])
ap.add_argument('--dump-outputs', default=None, metavar='DIR')
a = ap.parse_args()

arch = syn.CONFIGS[a.config]
B = a.batch
device = torch.device('cuda', 0)
torch.cuda.set_device(device)
sd = syn.make_state_dict(arch, 0, power_iters=30 if a.config != 'celebahq256' else 5)
model = build_flow(arch, B)
model.load_state_dict(sd, strict=True)
model = model.to(device).eval()
nsteps = a.warmup + a.steps
xs = torch.stack([syn.image_batch(B, arch['input_size'], arch['nvals'], seed=i) for i in range(min(nsteps, 4))]).to(device)
ndim = int(np.prod(arch['input_size']))
image_logpx(model, xs[0], arch['nvals'])          # creates the engine nets
blocks = imblocks(model)
chosen = [int(t) for t in a.blocks.split(',') if t != ''] or list(range(len(blocks)))
variants = [v for v in a.variants.split(',') if v]
VALUE = lambda v: {'off': _hip.INF_SERIES_GROUP_OFF, 'auto': 0}.get(v) if v in ('off', 'auto') else int(v)

# device events around the chosen blocks' forwards (recorded on the current stream, read after the run)
events = []
timing = {'on': False}


def _pre(mod, inp):
    if timing['on']:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events.append([e, None])


def _post(mod, inp, out):
    if timing['on']:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events[-1][1] = e


for i in chosen:
    blocks[i].register_forward_pre_hook(_pre)
    blocks[i].register_forward_hook(_post)


def nets_of(blk):
    return [n for net in (blk.nnet_x, blk.nnet_z) for n in net.__dict__.get('_inf_native', {}).values()]


def run(variant):
    for i, blk in enumerate(blocks):
        for n in nets_of(blk):
            n.set_option(_hip.INF_OPT_SERIES_GROUP, VALUE(variant) if i in chosen else _hip.INF_SERIES_GROUP_OFF)
    set_probe_mode('device', seed=12345)
    np.random.seed(0)
    torch.manual_seed(0)
    returned = {}

    def steps(first, count):
        pending, last = None, None
        for i in range(first, first + count):
            _, logpx, z = image_logpx(model, xs[i % xs.shape[0]], arch['nvals'])
            returned['logpx'], returned['z'] = logpx, z
            out = dd.global_logpx_pair(logpx)
            if pending is not None:
                last = dd.bits_per_dim(*pending.get(), ndim)
            pending = out
        return dd.bits_per_dim(*pending.get(), ndim) if pending is not None else last

    steps(0, a.warmup)
    torch.cuda.synchronize()
    del events[:]
    timing['on'] = True
    t0 = time.perf_counter()
    bpd = steps(a.warmup, a.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    timing['on'] = False
    ms_blocks = sum(e0.elapsed_time(e1) for e0, e1 in events) / a.steps
    returned['bits_per_dim'] = np.float64(bpd)
    return B * a.steps / dt, dt / a.steps * 1e3, ms_blocks, float(bpd), returned


res = {v: [] for v in variants}
blk_ms = {v: [] for v in variants}
for r in range(a.reps):
    for variant in variants:
        v, ms, msb, bpd, ret = run(variant)
        res[variant].append(v)
        blk_ms[variant].append(msb)
        print(json.dumps({'variant': variant, 'blocks': chosen, 'rep': r, 'value': round(v, 3), 'unit': 'samples/s',
                          'ms_per_step': round(ms, 3), 'ms_blocks': round(msb, 3), 'steps': a.steps, 'warmup': a.warmup,
                          'batch': B, 'config': a.config, 'bits_per_dim': round(bpd, 6),
                          'broyden_steps': [b.last_broyden['nstep'] for b in blocks]}), flush=True)
        if a.dump_outputs and r == a.reps - 1:
            d = os.path.join(a.dump_outputs, variant)
            os.makedirs(d, exist_ok=True)
            for k, t in ret.items():
                np.save(os.path.join(d, k + '.npy'), t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
for variant in variants:
    s, m = sorted(res[variant]), sorted(blk_ms[variant])
    print(json.dumps({'summary': variant, 'median': round(s[len(s) // 2], 1), 'min': round(s[0], 1),
                      'max': round(s[-1], 1), 'spread': round(s[-1] - s[0], 1), 'ms_blocks_median': round(m[len(m) // 2], 3),
                      'ms_blocks_min': round(m[0], 3), 'ms_blocks_max': round(m[-1], 3), 'runs': len(s)}), flush=True)
