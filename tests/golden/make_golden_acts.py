"""Golden vectors for the activation table's other entries and for bias-free layers, from the reference itself
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_acts.py [case ...]

Same harness as make_golden.py (its import shims, model builders and capture hooks, reused by import) and, for the
training case, make_golden_train.py's.  The reference's ``ImplicitFlow(activation_fn=...)`` takes eight names
(lib/implicit_flow.py:8-17); make_golden.py covers swish and sin, this file the other six on the same architectures
(lib/synthetic.py ``CONFIGS['cifar10_small_elu']`` and so on), and one imBlock whose first conv has no bias.

Every case runs the reference TWICE, with 1 and with 8 torch threads, and is written only if the two runs agree in
every block's Broyden ``nstep`` / ``lowest_step`` and series lengths: a trajectory that a change of summation order
moves is no fixture.  torch's two thread counts can give the same bits, so for the activations with a kink in
the derivative (ReLU) or in the second derivative (LipschitzCube) that check alone proves little: a hidden unit whose
pre-activation lies within fp32 rounding of the kink flips its saved derivative under any other summation order, and
the power series moves by a discrete amount (act_relu_full_b2 with input seed 3: one unit of block 5 moves that
block's log-det by 5.8e-3 nats when x is scaled by 1 + 2e-7 N(0, 1)).  Those cases therefore also run on PERTURB
copies of the input, x (1 + 2e-7 N(0, 1)), and are written only if every block keeps its trajectory and its log-det
within 5e-4 nats (a quarter of the 2e-3 the tests allow).  Seeds below are the first ones tried unless noted.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims + reference import + hooks)
import make_golden_train as mgt  # noqa: E402  (backward-solve and Neumann hooks)

torch = mg.torch
syn = mg.syn
layers = mg.layers
base_layers = mg.base_layers

FC_ACTS = {'sin': base_layers.Sin, 'swish': base_layers.Swish, 'elu': torch.nn.ELU, 'softplus': torch.nn.Softplus}


def _fc_model(arch):
    """make_golden.fc_model with the activation looked up in FC_ACTS (train_tabular.py:292-336)."""
    d = arch['d']
    dims = [d] + list(arch['dims']) + [d]

    def build_nnet():
        nnet = []
        for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
            if i > 0:
                nnet.append(FC_ACTS[arch['act']]())
            nnet.append(base_layers.get_linear(a, b, coeff=arch['coeff'], n_iterations=None, atol=1e-3, rtol=1e-3,
                                               domain=2, codomain=2, zero_init=(b == d)))
        return torch.nn.Sequential(*nnet)

    blocks = [layers.imBlock(build_nnet(), build_nnet(), n_dist=arch['n_dist'], n_power_series=None,
                             exact_trace=arch.get('exact_trace', False), brute_force=arch['brute_force'], n_samples=1,
                             n_exact_terms=arch['n_exact_terms'], neumann_grad=False, grad_in_forward=False,
                             eps_forward=arch['eps_forward'])
              for _ in range(arch['n_blocks'])]
    return layers.SequentialFlow(blocks)


# run_case / run_train_case look the fc builder up in make_golden's namespace: stable() installs the builder above
# there for the duration of a case and puts make_golden's own back


def _trajectory(path):
    g = np.load(path)
    out = []
    for i in range(int(g['nblocks'])):
        out.append(tuple(np.asarray(g[k]).tolist() if k in g else None
                         for k in ('b%d_nstep' % i, 'b%d_lowest_step' % i, 'b%d_n_power_series' % i,
                                   'b%d_bwd_nstep' % i, 'b%d_bwd_lowest_step' % i)))
    return out, float(g['loss'])


PERTURB = 3          # perturbed copies of the input for the kinked activations
PERTURB_REL = 2e-7   # ~ 2 fp32 ulps
PERTURB_LOGDET = 5e-4


def _logdets(path):
    g = np.load(path)
    return [np.asarray(g['b%d_logdet' % i], np.float64) for i in range(int(g['nblocks'])) if 'b%d_logdet' % i in g]


def perturbed(x, k):
    return x * (1 + PERTURB_REL * torch.randn(x.shape, generator=torch.Generator().manual_seed(1000 + k)))


def stable(name, run, x=None):
    """run(x) writes tests/golden/<name>.npz (every run overwrites it; the last one, 8 threads on the unperturbed
    input, is the fixture); it runs with 1 and with 8 threads and the file is kept only when both give the same
    trajectory.  With x given (the kinked activations) it also runs on PERTURB perturbed copies of x
    first, each of which must keep the trajectory and every block's log-det within PERTURB_LOGDET."""
    path = os.path.join(HERE, name + '.npz')
    got, lds = [], []
    own_builder = mg.fc_model
    mg.fc_model = _fc_model
    try:
        torch.set_num_threads(8)
        for k in range(PERTURB if x is not None else 0):
            run(perturbed(x, k))
            got.append(_trajectory(path))
            lds.append(_logdets(path))
        for nt in (1, 8):
            torch.set_num_threads(nt)
            run(x) if x is not None else run()
            got.append(_trajectory(path))
            lds.append(_logdets(path))
    finally:
        mg.fc_model = own_builder
    worst = max([float(np.abs(a - b).max()) for ld in lds[:-1] for a, b in zip(ld, lds[-1])] or [0.])
    if any(t[0] != got[-1][0] for t in got) or worst > PERTURB_LOGDET:
        os.remove(path)
        raise SystemExit('%s: not stable (choose another seed): trajectories %s, worst log-det move %.2e'
                         % (name, ['same' if t[0] == got[-1][0] else 'DIFFERS' for t in got], worst))
    print('   %s: stable over 1 / 8 threads%s, |d loss| %.2e' % (
        name, ' and %d perturbed inputs (worst log-det move %.1e)' % (PERTURB, worst) if x is not None else '',
        abs(got[-1][1] - got[-2][1])))


# ---- one imBlock with a bias-free first conv -----------------------------------------------------------------
NOBIAS = dict(shape=(3, 8, 8), hidden=64, coeff=0.9, B=4, eps_forward=1e-6, n_exact_terms=10)


def nobias_block():
    """imBlock on (3, 8, 8): get_conv2d(3 -> 64, 3x3, bias=False), ReLU, get_conv2d(64 -> 3, 3x3), both branches."""
    p = NOBIAS

    def nnet():
        conv = lambda a, b, bias: base_layers.get_conv2d(a, b, 3, 1, 1, coeff=p['coeff'], n_iterations=None, atol=1e-3,
                                                         rtol=1e-3, domain=2, codomain=2, bias=bias)
        return torch.nn.Sequential(conv(3, p['hidden'], False), torch.nn.ReLU(), conv(p['hidden'], 3, True))
    return layers.imBlock(nnet(), nnet(), n_dist='poisson', n_power_series=None, exact_trace=False, brute_force=False,
                          n_samples=1, n_exact_terms=p['n_exact_terms'], neumann_grad=True, grad_in_forward=True,
                          eps_forward=p['eps_forward'])


def run_nobias(name, seed, x_seed, init_seed):
    """The block keeps its own random initialisation (torch.manual_seed(init_seed)) after 40 power iterations; the
    state dict is stored in the fixture ('sd:' keys), as the iResBlock fixtures do."""
    p = NOBIAS
    torch.manual_seed(init_seed)
    blk = nobias_block()
    x = torch.randn(p['B'], *p['shape'], generator=torch.Generator().manual_seed(x_seed)) * 0.5
    with torch.no_grad():
        blk(x[:2].clone(), restore=True)
        for m in blk.modules():
            if hasattr(m, 'compute_weight') and hasattr(m, 'u'):
                m.compute_weight(update=True, n_iterations=40)
    blk.eval()
    out = {'sd:' + k: v.detach().numpy().copy() for k, v in blk.state_dict().items()}
    mg.REC.clear()
    np.random.seed(seed)
    torch.manual_seed(seed)
    with torch.no_grad():
        z, delta = blk(x, torch.zeros(p['B'], 1))
    logpz = (-0.5 * np.log(2 * np.pi) - z.pow(2) / 2).view(p['B'], -1).sum(1, keepdim=True)
    logpx = logpz - delta
    loss = -torch.mean(logpx)
    r = mg.REC[0]
    out.update(x=x.detach().numpy().astype(np.float32), seed=np.int64(seed), loss=np.float64(loss.item()),
               logpx=logpx.detach().view(-1).numpy().astype(np.float64),
               z=z.detach().reshape(p['B'], -1).numpy().astype(np.float32),
               nblocks=np.int64(1), b0_nstep=np.int64(r['nstep']), b0_lowest_step=np.int64(r['lowest_step']),
               b0_prot_break=np.int64(r['prot_break']), b0_n_power_series=np.asarray(r['n_power_series']),
               b0_logdet=r['logdet'], b0_z=r['z'])
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-22s loss=%.8f nstep=%d lowest=%d nps=%s -> %s (%d KB)' % (
        name, loss.item(), r['nstep'], r['lowest_step'], r['n_power_series'], os.path.basename(path),
        os.path.getsize(path) // 1024))


# No 'zero' flow: the reference itself cannot evaluate one.  Its Zero module returns torch.zeros_like(x), which is not
# connected to x in the autograd graph, so basic_logdet_estimator's torch.autograd.grad raises ("One of the
# differentiated Tensors appears to not have been used in the graph").  The engine's Zero kernels are checked against
# fp64 torch on single nets instead (tests/test_gpu_acts.py).
KINKED = ('relu', 'lcube')
# input seed of the relu full fixture: 3 (every other image fixture's) moves block 5's log-det by 5.8e-3 under the
# perturbation check, 4 .. 11 move one by 0.7e-3 .. 1.3e-3 (at idim 512 some unit always sits near the kink); 12 is the
# first that keeps every block within 5e-4 (worst move 1.8e-6)
RELU_FULL_X_SEED = 12


def _image_case(name, arch_name, x_seed, kinked):
    run = lambda x=None: mg.run_case(name, syn.CONFIGS[arch_name],
                                     syn.image_batch(2, seed=x_seed) if x is None else x, seed=7)
    return lambda: stable(name, run, syn.image_batch(2, seed=x_seed) if kinked else None)


CASES = {}
for _a in [a for a in syn.NEW_ACTS if a != 'zero']:
    CASES['act_%s_small_b2' % _a] = _image_case('act_%s_small_b2' % _a, 'cifar10_small_' + _a, 3, _a in KINKED)
for _a in ('elu', 'softplus', 'relu'):
    CASES['act_%s_full_b2' % _a] = _image_case('act_%s_full_b2' % _a, 'cifar10_' + _a,
                                               RELU_FULL_X_SEED if _a == 'relu' else 3, _a in KINKED)
CASES['act_elu_power_b64'] = lambda: stable('act_elu_power_b64', lambda: mg.run_case(
    'act_elu_power_b64', syn.CONFIGS['power_elu'], syn.tabular_batch(64, 6, seed=3), seed=7))
CASES['act_softplus_toy_b64'] = lambda: stable('act_softplus_toy_b64', lambda: mg.run_case(
    'act_softplus_toy_b64', syn.CONFIGS['toy_softplus'], syn.checkerboard_batch(64, seed=3), seed=7))
CASES['nobias_relu_b4'] = lambda: stable('nobias_relu_b4', lambda: run_nobias('nobias_relu_b4', seed=7, x_seed=3,
                                                                             init_seed=11))
CASES['act_elu_small_train_b2'] = lambda: stable('act_elu_small_train_b2', lambda: mgt.run_train_case(
    'act_elu_small_train_b2', syn.CONFIGS['cifar10_small_elu'], syn.image_batch(2, seed=21), seed=5))

if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        CASES[n]()
