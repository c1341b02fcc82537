"""Deterministic synthetic weights and inputs for the BASELINE.json configs.

No dataset or checkpoint is reachable offline, so every test, fixture and bench run
uses weights made here: random-init weights of the reference architectures, keyed
exactly like the reference's ``state_dict`` (so the same dict loads into the
reference model, into the oracle, and into this package's drop-in modules).

Per-key values come from ``numpy.random.Generator(PCG64([seed, crc32(key)]))``,
so they are identical on every machine and independent of module walk order.
The spectral-norm vectors ``u``/``v`` of every ``InducedNorm*`` layer are the
result of a float64 power iteration, so ``scale`` ~= the layer's operator norm and
``W / max(1, scale/coeff)`` caps every layer at ``coeff`` like a trained model
(reference: ``mixed_lipschitz.py:267-274,320-326,378-386``).

This module imports only numpy/torch (no package-relative imports) so the
golden-fixture script can load it by path next to the reference's own ``lib``.
"""
import zlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

# ---------------------------------------------------------------------------------------
# Architectures (BASELINE.json configs).  Keys follow the reference constructors.
# ---------------------------------------------------------------------------------------

# run_cifar10.sh:1-3 + train_img.py defaults (n_dist poisson, factor_out False,
# sn_tol 1e-3, init layer LogitTransform(0.05) at train_img.py:243).
CIFAR10 = dict(
    kind='conv', input_size=(3, 32, 32), n_blocks=[2, 2, 2], idim=512, kernels='3-1-3',
    act='swish', preact=True, actnorm=True, init_alpha=0.05, coeff=0.9, n_dist='poisson',
    n_exact_terms=10, n_exact_terms_test=20, threshold=30, eps_forward=1e-6, nvals=256,
    lamb=2.0, geom_p=0.5,
)

# Reduced CIFAR-shaped config for fast parity cases (same code path, idim 64).
CIFAR10_SMALL = dict(CIFAR10, idim=64)

# CelebA-HQ 256, 5 bits: C3 architecture with 4 scales.
CELEBAHQ256 = dict(CIFAR10, input_size=(3, 256, 256), n_blocks=[2, 2, 2, 2], nvals=32)

# --data mnist at --imagesize 28 (train_img.py:256-258: one channel, LogitTransform(1e-6)): scales of 28x28, 14x14 and
# 7x7, none of which cuts into whole 32- or 64-pixel tiles (the fused kernels' ragged tiles).
MNIST = dict(CIFAR10, input_size=(1, 28, 28), init_alpha=1e-6)
# One block per scale at idim 256: the fixture of tests/golden/make_golden_ragged.py.
MNIST_SMALL = dict(MNIST, n_blocks=[1, 1, 1], idim=256)

# run_tabular.sh:1-2 (POWER): 20 blocks, 6-128x4-6, sin, coeff .99, epsf 1e-5, geometric.
POWER = dict(
    kind='fc', d=6, dims=[128, 128, 128, 128], n_blocks=20, act='sin', coeff=0.99,
    n_dist='geometric', n_exact_terms=2, n_exact_terms_test=20, threshold=30, eps_forward=1e-5,
    lamb=2.0, geom_p=0.5, brute_force=False,
)

# run_toy.sh:1 (checkerboard): 6 blocks, 2-128-128-2, sin, coeff .99, brute force.
TOY = dict(
    kind='fc', d=2, dims=[128, 128], n_blocks=6, act='sin', coeff=0.99, n_dist='geometric',
    n_exact_terms=2, n_exact_terms_test=20, threshold=30, eps_forward=1e-6, lamb=2.0,
    geom_p=0.5, brute_force=True,
)

# POWER with exact_trace=True (implicit_block.py:323-343): a parity case for the exact-trace series.
POWER_EXACT = dict(POWER, exact_trace=True)

CONFIGS = {'cifar10': CIFAR10, 'cifar10_small': CIFAR10_SMALL, 'celebahq256': CELEBAHQ256,
           'power': POWER, 'toy': TOY, 'power_exact': POWER_EXACT, 'mnist': MNIST, 'mnist_small': MNIST_SMALL}

# The activation table's other entries (implicit_flow.py ACT_FNS) on the architectures above: the fixtures of
# tests/golden/make_golden_acts.py.  Only Swish has a parameter, so these state dicts hold no '.beta' keys.
NEW_ACTS = ('elu', 'softplus', 'relu', 'lcube', 'identity', 'zero')
for _a in NEW_ACTS:
    CONFIGS['cifar10_small_' + _a] = dict(CIFAR10_SMALL, act=_a)
for _a in ('elu', 'softplus', 'relu'):
    CONFIGS['cifar10_' + _a] = dict(CIFAR10, act=_a)
CONFIGS['power_elu'] = dict(POWER, act='elu')
CONFIGS['toy_softplus'] = dict(TOY, act='softplus')
del _a

# Sin, the default activation of the reference's image driver (train_img.py --act), on the image architectures: with the
# leading activation of preact (the architectures' own setting) and without.  The fixtures of
# tests/golden/make_golden_sin.py.
CONFIGS['cifar10_small_sin'] = dict(CIFAR10_SMALL, act='sin')
CONFIGS['cifar10_sin'] = dict(CIFAR10, act='sin')
CONFIGS['cifar10_small_sin_nopre'] = dict(CIFAR10_SMALL, act='sin', preact=False)
CONFIGS['cifar10_sin_nopre'] = dict(CIFAR10, act='sin', preact=False)

# Mixed induced norms (--vnorms): layer i of every net is bounded in the l_p[i] -> l_p[i+1] norm, 'f' standing for
# inf.  An arch without the key is all-2.  '13f1' gives 1 -> 3, 3 -> inf and inf -> 1: every normalisation form of
# csrc/power.hip (one-hot v, power u and v, one-hot u on the 1x1 conv, both sign vectors) on layers that the
# reference's factories build as InducedNorm layers (lipschitz.py:510-531; '122f' would give its closed-form
# LopConv2d, which is not provided).  The fixtures of tests/golden/make_golden_vnorms.py.
CONFIGS['cifar10_small_13f1'] = dict(CIFAR10_SMALL, vnorms='13f1')
CONFIGS['cifar10_13f1'] = dict(CIFAR10, vnorms='13f1')
CONFIGS['fc_2332'] = dict(POWER, dims=[32, 32], n_blocks=4, vnorms='2332')

# Fully connected blocks over more than 32 features (the fixtures of tests/golden/make_golden_widefc.py).
# Image flows on 3 x 8 x 8 (two scales, d = 192 flattened at both): ImplicitFlow(fc_end=True) -- its class default -- ends
# the last scale in two imBlock(FCNet, FCNet) of width fc_idim, each followed by an ActNorm1d; ImplicitFlow(fc=True)
# makes every block and every ActNorm fully connected.  Tabular flows at the widths of MINIBOONE (43) and BSDS300 (63).
FCEND_SMALL = dict(CIFAR10_SMALL, input_size=(3, 8, 8), n_blocks=[1, 1], fc_end=True, fc_idim=128)
FC_IMG_SMALL = dict(CIFAR10_SMALL, input_size=(3, 8, 8), n_blocks=[1, 1], fc=True)
TAB_D43 = dict(POWER, d=43, n_blocks=4)
TAB_D63 = dict(POWER, d=63, n_blocks=4)
CONFIGS.update(fcend_small=FCEND_SMALL, fc_img_small=FC_IMG_SMALL, tab_d43=TAB_D43, tab_d63=TAB_D63)
# fc_end with Sin and preact: the conv block and the two fc blocks (d = 192) all lead with a Sin but the first one's nets
CONFIGS['fcend_small_sin'] = dict(FCEND_SMALL, act='sin')


# Layers of the mixed-norm power-iteration fixtures (make_golden_vnorms.py): the smallest shapes that reach every
# normalisation path of csrc/power.hip.  (name, kind, cin, cout, k, hw, [(domain, codomain), ...]); the first pair
# of each also runs in tolerance mode.
_INF = float('inf')
VNORM_LAYERS = [
    ('lin7x5', 'linear', 5, 7, 1, None, [(1, 2), (2, _INF), (1, _INF), (3, 3), (_INF, 1), (2, 5)]),       # < one wave
    ('lin130x70', 'linear', 70, 130, 1, None, [(1, 2), (2, _INF), (1, _INF), (3, 3), (_INF, 1), (2, 5)]),
    ('conv1', 'conv', 3, 5, 1, (4, 4), [(1, _INF), (1, 2), (2, _INF)]),                  # the stale-buffer rule
    ('conv3_6x5', 'conv', 3, 5, 3, (6, 5), [(1, 2), (2, _INF), (3, 3), (_INF, 1)]),
    # nu = 73728 (thread-per-output apply), nv = 18432 (wave-per-output apply), both >= PI_MULTI_MIN
    ('conv3_96', 'conv', 2, 8, 3, (96, 96), [(1, 2), (2, _INF), (3, 3)]),
]
VNORM_SAMPLE = 4096      # vectors longer than this are stored as a seeded sample + vec_summary


def vnorm_layer_inputs(name, seed):
    """(W, u0, v0) of a VNORM_LAYERS entry: kaiming-uniform-like W x 3 (sigma well above 1) and N(0, 1) start vectors
    (the iteration normalises them on its first step), float32, keyed numpy PCG64."""
    _, kind, cin, cout, k, hw, _ = next(l for l in VNORM_LAYERS if l[0] == name)
    rng = _rng(seed, 'vnorm.' + name)
    bound = 3.0 / np.sqrt(cin * k * k)
    shape = (cout, cin) if kind == 'linear' else (cout, cin, k, k)
    W = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    P = 1 if (kind == 'linear' or k == 1) else hw[0] * hw[1]
    u0 = rng.standard_normal(cout * P).astype(np.float32)
    v0 = rng.standard_normal(cin * P).astype(np.float32)
    return _t(W), _t(u0), _t(v0)


def vnorm_sample_index(name, n):
    """Seeded positions of the stored sample of a long vector."""
    return np.sort(_rng(11, 'vnorm.idx.' + name).choice(n, VNORM_SAMPLE, replace=False))


def layer_norms(arch):
    """[(domain, codomain)] per weight layer of a net (implicit_flow.py:292-299, train_tabular.py:283-295), or None
    for an arch without 'vnorms'."""
    if arch.get('vnorms') is None:
        return None
    ps = [float('inf') if c == 'f' else float(c) for c in arch['vnorms']]
    return list(zip(ps[:-1], ps[1:]))


def _rng(seed, key):
    return np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(key.encode())]))


def n_scales(input_size, n_blocks):
    """implicit_flow.py:141-148 (number of 2x halvings while h, w >= 4), capped by len(n_blocks)."""
    _, h, w = input_size
    n = 0
    while h >= 4 and w >= 4:
        n += 1
        h //= 2
        w //= 2
    return min(len(n_blocks), n)


def conv_flow_layout(arch):
    """Chain layout of ImplicitFlow(factor_out=False) (implicit_flow.py:101-139,411-434) with fc = arch.get('fc', False)
    and fc_end = arch.get('fc_end', False).

    Returns a list of scales; each scale is a list of (kind, info) in chain order with kind in
    {'logit', 'actnorm', 'imblock', 'squeeze', 'fc_actnorm', 'fc_imblock'}.  imblock info holds the (C,H,W) it acts on
    and its net layer list [(act,), ('conv', cin, cout, k), ...] with act = arch['act'].  The fc kinds (fc / fc_end
    flows only): 'fc_imblock' is an imBlock of two FCNet over the flattened (C,H,W) (net: [(act,), ('linear', a, b),
    ...] under the key '<net>.nnet', a leading activation whenever preact), 'fc_actnorm' an FCWrapper(ActNorm1d(n))
    (keys under '.fc_module').
    """
    c, h, w = arch['input_size']
    ks = list(map(int, arch['kernels'].split('-')))
    fc, fc_end = arch.get('fc', False), arch.get('fc_end', False)
    scales = []
    ns = n_scales(arch['input_size'], arch['n_blocks'])

    def fc_block(width):                      # FCNet (implicit_flow.py:437-474): len(ks) - 1 hidden layers
        d = c * h * w
        net = [(arch['act'],)] if arch['preact'] else []
        last = d
        for _ in range(len(ks) - 1):
            net += [('linear', last, width), (arch['act'],)]
            last = width
        net.append(('linear', last, d))
        return ('fc_imblock', dict(shape=(c, h, w), net=net))

    def actnorm():
        return ('fc_actnorm', dict(n=c * h * w)) if fc else ('actnorm', dict(c=c))

    for i in range(ns):
        chain = []
        first = (i == 0)
        if first:
            chain.append(('logit', dict(alpha=arch['init_alpha'])))
            if arch['actnorm']:
                chain.append(actnorm())
        for b in range(arch['n_blocks'][i]):
            if fc:
                chain.append(fc_block(arch['idim']))
                if arch['actnorm']:
                    chain.append(actnorm())
                continue
            first_block = first and b == 0
            net = []
            if not first_block and arch['preact']:
                net.append((arch['act'],))
            net.append(('conv', c, arch['idim'], ks[0]))
            net.append((arch['act'],))
            for k in ks[1:-1]:
                net.append(('conv', arch['idim'], arch['idim'], k))
                net.append((arch['act'],))
            net.append(('conv', arch['idim'], c, ks[-1]))
            chain.append(('imblock', dict(shape=(c, h, w), net=net)))
            if arch['actnorm']:
                chain.append(('actnorm', dict(c=c)))
        if i < ns - 1:
            chain.append(('squeeze', dict(factor=2)))
            c, h, w = c * 4, h // 2, w // 2
        elif fc_end:                          # two fc blocks at the end of the last scale (implicit_flow.py:429-433)
            for _ in range(2):
                chain.append(fc_block(arch.get('fc_idim', 128)))
                if arch['actnorm']:
                    chain.append(('fc_actnorm', dict(n=c * h * w)))
        scales.append(chain)
    return scales


def fc_flow_layout(arch):
    """SequentialFlow([imBlock(build_nnet, build_nnet)]*n) (train_tabular.py:292-336, train_toy.py:146-171,224-242).

    build_nnet interleaves activations before every linear except the first.
    """
    d = arch['d']
    dims = [d] + list(arch['dims']) + [d]
    net = []
    for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        if i > 0:
            net.append((arch['act'],))
        net.append(('linear', a, b))
    return [('imblock', dict(shape=(d,), net=net)) for _ in range(arch['n_blocks'])]


# ---------------------------------------------------------------------------------------
# Power iteration (float64) for the InducedNorm u/v buffers; norms = (domain, codomain), None for 2 -> 2.
# ---------------------------------------------------------------------------------------

def _normalize(x, p, is_u):
    """normalize_u (codomain p) / normalize_v (domain p) of mixed_lipschitz.py:414-444 on a float64 array, p != 2."""
    if p == (float('inf') if is_u else 1.0):            # one-hot, +1 whatever the sign
        out = np.zeros_like(x)
        out[np.argmax(np.abs(x))] = 1.0
        return out
    sign = np.where(x < 0, -1.0, 1.0)
    if p == (1.0 if is_u else float('inf')):            # the limit of the power form: the sign vector
        return sign
    a = np.abs(x) / np.abs(x).max()
    a = a ** ((p - 1) if is_u else 1 / (p - 1))
    q = p / (p - 1) if is_u else p
    return sign * a / (a ** q).sum() ** (1 / q)


def _power_conv(W, hw, k, rng, iters, norms=None):
    Wt = torch.from_numpy(W.astype(np.float64))
    cin = W.shape[1]
    dom, cod = norms or (2.0, 2.0)
    nv = (lambda t: t / t.norm()) if dom == 2 else (lambda t: torch.from_numpy(_normalize(t.numpy(), dom, False)))
    nu = (lambda t: t / t.norm()) if cod == 2 else (lambda t: torch.from_numpy(_normalize(t.numpy(), cod, True)))
    v = torch.from_numpy(rng.standard_normal(cin * hw[0] * hw[1]))
    v = nv(v)
    pad = k // 2
    for _ in range(iters):
        u = F.conv2d(v.view(1, cin, *hw), Wt, padding=pad).reshape(-1)
        u = nu(u)
        v = F.conv_transpose2d(u.view(1, W.shape[0], *hw), Wt, padding=pad).reshape(-1)
        v = nv(v)
    sigma = float(torch.dot(u, F.conv2d(v.view(1, cin, *hw), Wt, padding=pad).reshape(-1)))
    return u.numpy(), v.numpy(), sigma


def _power_mat(W, rng, iters, norms=None):
    W = W.astype(np.float64)
    dom, cod = norms or (2.0, 2.0)
    nv = (lambda t: t / np.linalg.norm(t)) if dom == 2 else (lambda t: _normalize(t, dom, False))
    nu = (lambda t: t / np.linalg.norm(t)) if cod == 2 else (lambda t: _normalize(t, cod, True))
    v = rng.standard_normal(W.shape[1])
    v = nv(v)
    for _ in range(iters):
        u = W @ v
        u = nu(u)
        v = W.T @ u
        v = nv(v)
    return u, v, float(u @ (W @ v))


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).clone()


def _conv_entries(sd, key, cin, cout, k, hw, seed, power_iters, norms=None):
    rng = _rng(seed, key)
    bound = 1.0 / np.sqrt(cin * k * k)        # kaiming_uniform(a=sqrt(5)) bound (mixed_lipschitz.py:188-193)
    W = rng.uniform(-bound, bound, size=(cout, cin, k, k)).astype(np.float32)
    b = rng.uniform(-bound, bound, size=(cout,)).astype(np.float32)
    if k == 1:
        u, v, s = _power_mat(W.reshape(cout, cin), rng, power_iters, norms)
    else:
        u, v, s = _power_conv(W, hw, k, rng, power_iters, norms)
    sd[key + '.weight'] = _t(W)
    sd[key + '.bias'] = _t(b)
    sd[key + '.initialized'] = torch.tensor(1)
    sd[key + '.spatial_dims'] = torch.tensor([float(hw[0]), float(hw[1])])
    sd[key + '.scale'] = torch.tensor(np.float32(s))
    sd[key + '.u'] = _t(u)
    sd[key + '.v'] = _t(v)


def _linear_entries(sd, key, fin, fout, seed, power_iters, norms=None):
    rng = _rng(seed, key)
    bound = 1.0 / np.sqrt(fin)
    W = rng.uniform(-bound, bound, size=(fout, fin)).astype(np.float32)
    b = rng.uniform(-bound, bound, size=(fout,)).astype(np.float32)
    u, v, s = _power_mat(W, rng, power_iters, norms)
    sd[key + '.weight'] = _t(W)
    sd[key + '.bias'] = _t(b)
    sd[key + '.scale'] = torch.tensor(np.float32(s))
    sd[key + '.u'] = _t(u)
    sd[key + '.v'] = _t(v)


def _net_entries(sd, prefix, net, hw, seed, power_iters, norms=None):
    norms = iter(norms or [None] * len(net))
    for j, layer in enumerate(net):
        key = '%s.%d' % (prefix, j)
        if layer[0] == 'conv':
            _conv_entries(sd, key, layer[1], layer[2], layer[3], hw, seed, power_iters, next(norms))
        elif layer[0] == 'linear':
            _linear_entries(sd, key, layer[1], layer[2], seed, power_iters, next(norms))
        elif layer[0] == 'swish':
            sd[key + '.beta'] = _t([_rng(seed, key).uniform(0.3, 0.8)])


def _imblock_entries(sd, prefix, info, arch, seed, power_iters, sub=''):
    """sub: '.nnet' for the FCNet branches of an fc block inside an image flow (their layers sit one level down)."""
    hw = info['shape'][1:] if len(info['shape']) == 3 and not sub else None
    sd[prefix + '.lamb'] = torch.tensor(float(arch['lamb']))
    sd[prefix + '.last_n_samples'] = torch.zeros(1)
    sd[prefix + '.last_firmom'] = torch.zeros(1)
    sd[prefix + '.last_secmom'] = torch.zeros(1)
    for net in ('nnet_x', 'nnet_z'):
        _net_entries(sd, prefix + '.' + net + sub, info['net'], hw, seed, power_iters, layer_norms(arch))
    # frozen copies (implicit_block.py:136-141), refreshed from the nets every forward (:228-229)
    for net in ('nnet_x', 'nnet_z'):
        for k in list(sd.keys()):
            if k.startswith(prefix + '.' + net + '.'):
                sd[k.replace(prefix + '.' + net + '.', prefix + '.' + net + '_copy.', 1)] = sd[k].clone()


def make_state_dict(arch, seed=0, power_iters=30):
    """State dict of the reference model for ``arch`` (keys as reference ``ImplicitFlow`` /
    ``SequentialFlow`` produce them), filled with deterministic random-init weights."""
    sd = OrderedDict()
    if arch['kind'] == 'conv':
        for i, chain in enumerate(conv_flow_layout(arch)):
            for j, (kind, info) in enumerate(chain):
                prefix = 'transforms.%d.chain.%d' % (i, j)
                if kind == 'actnorm':
                    rng = _rng(seed, prefix)
                    sd[prefix + '.weight'] = _t(rng.uniform(-0.3, 0.3, size=info['c']))
                    sd[prefix + '.bias'] = _t(rng.uniform(-0.3, 0.3, size=info['c']))
                    sd[prefix + '.initialized'] = torch.tensor(1)
                elif kind == 'imblock':
                    _imblock_entries(sd, prefix, info, arch, seed, power_iters)
                elif kind == 'fc_actnorm':
                    rng = _rng(seed, prefix)
                    sd[prefix + '.fc_module.weight'] = _t(rng.uniform(-0.3, 0.3, size=info['n']))
                    sd[prefix + '.fc_module.bias'] = _t(rng.uniform(-0.3, 0.3, size=info['n']))
                    sd[prefix + '.fc_module.initialized'] = torch.tensor(1)
                elif kind == 'fc_imblock':
                    _imblock_entries(sd, prefix, info, arch, seed, power_iters, sub='.nnet')
    else:
        for j, (kind, info) in enumerate(fc_flow_layout(arch)):
            _imblock_entries(sd, 'chain.%d' % j, info, arch, seed, power_iters)
    return sd


# ---------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------

def image_batch(B, input_size=(3, 32, 32), nvals=256, seed=0):
    """Dequantised synthetic images: (randint(0, nvals) + U[0,1)) / nvals (train_img.py:161-169)."""
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randint(0, nvals, (B,) + tuple(input_size), generator=g).float()
    x = x + torch.rand((B,) + tuple(input_size), generator=g)
    return x / nvals


def tabular_batch(B, d=6, seed=0):
    """Standardised tabular rows (POWER is standardised, tabular.py:155-161)."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn(B, d, generator=g)


def checkerboard_batch(B, seed=0):
    """2-D checkerboard sampler (lib/toy_data.py:104-108) on a private RandomState."""
    rs = np.random.RandomState(seed)
    x1 = rs.rand(B) * 4 - 2
    x2_ = rs.rand(B) - rs.randint(0, 2, B) * 2
    x2 = x2_ + (np.floor(x1) % 2)
    return torch.from_numpy(np.concatenate([x1[:, None], x2[:, None]], 1) * 2).float()


# Layers of the power-iteration fixtures (tests/golden/make_golden_edges.py power_iter_layers):
POWER_ITER_LAYERS = [   # (arch, key, kind, cin, cout, k, hw, n_iterations, perturbation scale)
    ('cifar10', 'transforms.0.chain.2.nnet_x.0', 'conv', 3, 512, 3, (32, 32), None, 0.5),
    ('cifar10', 'transforms.0.chain.2.nnet_x.2', 'conv', 512, 512, 1, (32, 32), None, 0.5),
    ('cifar10', 'transforms.0.chain.2.nnet_x.4', 'conv', 512, 3, 3, (32, 32), None, 0.5),
    ('cifar10', 'transforms.1.chain.0.nnet_z.1', 'conv', 12, 512, 3, (16, 16), None, 1.0),
    ('cifar10', 'transforms.2.chain.2.nnet_z.5', 'conv', 512, 48, 3, (8, 8), None, 1.0),
    ('cifar10', 'transforms.2.chain.0.nnet_x.3', 'conv', 512, 512, 1, (8, 8), 7, 0.05),
    ('cifar10', 'transforms.0.chain.4.nnet_z.1', 'conv', 3, 512, 3, (32, 32), None, 0.05),
    ('power', 'chain.0.nnet_x.0', 'linear', 6, 128, 1, None, None, 0.05),
    ('power', 'chain.3.nnet_z.2', 'linear', 128, 128, 1, None, None, 0.5),
]


# Broyden's protective break (broyden.py:169-172) and the Banach fallback it triggers (implicit_block.py:74-75,
# 57-65,17-28), on a single fc imBlock over d = 6 (tests/golden/make_golden_edges.py prot_break_b6):
#   nnet_x == 0 (zero weights and biases), so x_embed == x bit for bit;
#   nnet_z(z) = W2 sin(2 pi W1 z) / (2 pi) with a nilpotent coupling chain z0 -> z1 -> z2 -> z3:
#     f1 = C s(K z0), f2 = D s(z1), f3 = D s(z2), s(t) = sin(2 pi t) / (2 pi);
#   x ~ 1e-9 N(0, 1) with eps_forward 1e-13.
# Broyden's first step goes to z = -g(0) = -x, where |f1| ~ C / (2 pi) against an initial residual ~ |x|: the
# residual grows by ~1e8 (> 1e6: prot_break, with two orders of margin).  The Banach iteration z <- x - f(z) then
# settles one chain level per iteration and stops with an exactly-zero change after 3 iterations.  Samples whose
# z0 is exactly 0 never see the K coupling: their (linear, tiny) solve converges in Broyden (per-sample mode keeps
# their Broyden result).  J_f is nilpotent, so the exact log-dets are 0 up to rounding.
PROT_BREAK = dict(d=6, hidden=8, K=1e9, C=6.0, D=0.9, coeff=1e12, eps_forward=1e-13, x_scale=1e-9,
                  zero_rows=(1, 4), B=6)


def prot_break_nets_state():
    """State dict of the prot_break imBlock's nets (InducedNormLinear(6, 8), Sin, InducedNormLinear(8, 6)) and their
    frozen copies; u / v are the exact top singular vectors (sigma = K and C, far below coeff: W_eff == W)."""
    p = PROT_BREAK
    d, h = p['d'], p['hidden']
    W1 = np.zeros((h, d), np.float32)
    W2 = np.zeros((d, h), np.float32)
    W1[0, 0], W1[1, 1], W1[2, 2] = p['K'], 1.0, 1.0
    W2[1, 0], W2[2, 1], W2[3, 2] = p['C'], p['D'], p['D']
    e = lambda n, i: _t(np.eye(n, dtype=np.float32)[i])
    sd = OrderedDict()
    sd['lamb'] = torch.tensor(2.0)
    sd['last_n_samples'] = torch.zeros(1)
    sd['last_firmom'] = torch.zeros(1)
    sd['last_secmom'] = torch.zeros(1)
    for net in ('nnet_x', 'nnet_z'):
        zero = net == 'nnet_x'
        sd[net + '.0.weight'] = _t(np.zeros_like(W1) if zero else W1)
        sd[net + '.0.bias'] = torch.zeros(h)
        sd[net + '.0.scale'] = torch.tensor(0. if zero else float(p['K']))
        sd[net + '.0.u'], sd[net + '.0.v'] = e(h, 0), e(d, 0)
        sd[net + '.2.weight'] = _t(np.zeros_like(W2) if zero else W2)
        sd[net + '.2.bias'] = torch.zeros(d)
        sd[net + '.2.scale'] = torch.tensor(0. if zero else float(p['C']))
        sd[net + '.2.u'], sd[net + '.2.v'] = e(d, 1), e(h, 0)
    for k in list(sd.keys()):
        if k.startswith('nnet_'):
            sd[k.replace('nnet_x.', 'nnet_x_copy.', 1).replace('nnet_z.', 'nnet_z_copy.', 1)] = sd[k].clone()
    return sd


def prot_break_batch(seed=5):
    p = PROT_BREAK
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(p['B'], p['d'], generator=g) * p['x_scale']
    for r in p['zero_rows']:
        x[r, 0] = 0.
    return x


# A deep variant with the POWER nets' shape (6-128-128-128-128-6, Sin), so the fused fc paths and the device-resident
# block kernel (fcblock.hip) take it: nnet_x == 0; nnet_z has one coupling path z0 -> unit 0 of every hidden layer ->
# f1 with gain G per layer and C at the output, every matrix holding a single magnitude (which the scaled fp16 split
# represents to 2^-23 relative).  With x ~ 1e-9, Broyden's first step z = -x gives f1 ~ C s(G^4 x0) ~ 0.6 x0 / 1e-9
# against |g(0)| ~ 1e-9: the residual grows by ~1e8 (prot_break).  f1 depends on z0 only, which the Banach iteration
# fixes at x0 on its first pass, so it stops with an exactly-zero change on the next; the samples with x0 == 0
# converge in Broyden (per-sample rule).  J_f is nilpotent: the exact log-dets are 0 up to rounding.
PROT_BREAK_DEEP = dict(d=6, hidden=128, n_hidden=3, G=100.0, C=6.0, coeff=1e12, eps_forward=1e-13, x_scale=1e-9,
                       zero_rows=(1, 4), B=6)


def prot_break_deep_nets_state():
    """State dict of the deep prot_break imBlock (Sequential of InducedNormLinear / Sin, keys 0, 2, 4, 6, 8, and the
    frozen copies); u / v are the exact top singular vectors (sigma = G, G, G, G, C, far below coeff: W_eff == W)."""
    p = PROT_BREAK_DEEP
    d, h, nh = p['d'], p['hidden'], p['n_hidden']
    shapes = [(h, d)] + [(h, h)] * nh + [(d, h)]
    e = lambda n, i: _t(np.eye(n, dtype=np.float32)[i])
    sd = OrderedDict()
    sd['lamb'] = torch.tensor(2.0)
    sd['last_n_samples'] = torch.zeros(1)
    sd['last_firmom'] = torch.zeros(1)
    sd['last_secmom'] = torch.zeros(1)
    for net in ('nnet_x', 'nnet_z'):
        zero = net == 'nnet_x'
        for l, (o, i) in enumerate(shapes):
            W = np.zeros((o, i), np.float32)
            last = l == len(shapes) - 1
            gain = p['C'] if last else p['G']
            if not zero:
                W[1 if last else 0, 0] = gain
            k = '%s.%d.' % (net, 2 * l)
            sd[k + 'weight'] = _t(W)
            sd[k + 'bias'] = torch.zeros(o)
            sd[k + 'scale'] = torch.tensor(0. if zero else float(gain))
            sd[k + 'u'], sd[k + 'v'] = e(o, 1 if last else 0), e(i, 0)
    for k in list(sd.keys()):
        if k.startswith('nnet_'):
            sd[k.replace('nnet_x.', 'nnet_x_copy.', 1).replace('nnet_z.', 'nnet_z_copy.', 1)] = sd[k].clone()
    return sd


def prot_break_deep_batch(seed=6):
    p = PROT_BREAK_DEEP
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn(p['B'], p['d'], generator=g) * p['x_scale']
    for r in p['zero_rows']:
        x[r, 0] = 0.
    return x


def line_search_problem(kind, k=1.0):
    """(arch, state_dict) of the line-search fixtures (tests/golden/make_golden_edges.py line_search_case): the root
    problem of block 0.  'cifar_small': CIFAR10_SMALL as is.  'power' / 'toy': block 0's nets (nnet_x, nnet_z) with every
    InducedNormLinear weight x k under a Lipschitz cap of 1000 (W_eff == W), a harder root problem on which the Armijo
    search accepts backtracked steps."""
    if kind == 'cifar_small':
        return CIFAR10_SMALL, make_state_dict(CIFAR10_SMALL, 0)
    arch = POWER if kind == 'power' else TOY
    sd = make_state_dict(arch, 0)
    for key in list(sd):
        if key.startswith(('chain.0.nnet_x.', 'chain.0.nnet_z.')) and key.endswith('.weight'):
            sd[key] = sd[key] * float(k)
    return dict(arch, coeff=1000.), sd


def perturbed_weight(sd, key, seed=1, scale=0.05):
    """sd[key + '.weight'] moved off its converged u / v (as after an optimiser step): W + scale * std(W) * N(0, 1),
    deterministic (numpy PCG64 keyed like the weights).  Power-iteration fixtures start from it."""
    W = sd[key + '.weight'].numpy().astype(np.float32)
    noise = _rng(seed + 1000, key).standard_normal(W.shape).astype(np.float32)
    return torch.from_numpy(W + np.float32(scale * float(W.std())) * noise)


def vec_summary(v, key):
    """Size-independent summary of a long vector for fixtures: sum, sum of squares, a seeded +-1 projection
    (numpy PCG64 keyed by `key`), and the first 64 entries."""
    v = np.asarray(v, dtype=np.float64).ravel()
    sign = _rng(7, key).integers(0, 2, v.size).astype(np.float64) * 2 - 1
    return np.array([v.sum(), (v * v).sum(), (v * sign).sum()]), v[:64].astype(np.float32)
