"""A/B on one box: the bench workload (bench.py's model, batch, seeded inputs and weights, device probes, pipelined
readback) with the default eval schedule against the same with INF_OPT_EVAL_OVERLAP = 0 on some imBlocks, the runs
alternating in one process.  One JSON line per run, then a summary line per variant.

    python tools/ab_overlap_blocks.py [--seq-blocks 2,3] [--reps 5] [--steps 20] [--warmup 5] [--batch 64]
                                      [--config cifar10] [--dump-outputs DIR]

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
ap.add_argument('--seq-blocks', default='2,3', help='imBlocks (indices) run on the sequential schedule in the variant')
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
seq = [int(t) for t in a.seq_blocks.split(',') if t != '']


def nets_of(blk):
    return [n for net in (blk.nnet_x, blk.nnet_z) for n in net.__dict__.get('_inf_native', {}).values()]


def run(variant):
    for i, blk in enumerate(blocks):
        for n in nets_of(blk):
            n.set_option(_hip.INF_OPT_EVAL_OVERLAP, 0 if (variant == 'seq' and i in seq) else 1)
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
    t0 = time.perf_counter()
    bpd = steps(a.warmup, a.steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    returned['bits_per_dim'] = np.float64(bpd)
    return B * a.steps / dt, dt / a.steps * 1e3, float(bpd), returned


res = {'default': [], 'seq': []}
for r in range(a.reps):
    for variant in ('default', 'seq'):
        v, ms, bpd, ret = run(variant)
        res[variant].append(v)
        print(json.dumps({'variant': variant, 'seq_blocks': seq if variant == 'seq' else [], 'rep': r,
                          'value': round(v, 3), 'unit': 'samples/s', 'ms_per_step': round(ms, 3), 'steps': a.steps,
                          'warmup': a.warmup, 'batch': B, 'config': a.config, 'bits_per_dim': round(bpd, 6),
                          'broyden_steps': [b.last_broyden['nstep'] for b in blocks]}), flush=True)
        if a.dump_outputs and r == a.reps - 1:
            d = os.path.join(a.dump_outputs, variant)
            os.makedirs(d, exist_ok=True)
            for k, t in ret.items():
                np.save(os.path.join(d, k + '.npy'), t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
for variant, v in res.items():
    s = sorted(v)
    print(json.dumps({'summary': variant, 'median': round(s[len(s) // 2], 1), 'min': round(s[0], 1),
                      'max': round(s[-1], 1), 'runs': len(s)}), flush=True)
