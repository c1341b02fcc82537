"""Host-side checks of Sin image flows with the leading activation of preact: the module -> engine-kind mapping of a
preact Sin flow's nets (lib._hip.net_entries), the synthetic state dicts of the Sin architectures (lib/synthetic.py),
and the fixtures of tests/golden/make_golden_sin.py.  No GPU."""
import os

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks

SIN_ARCHS = ['cifar10_small_sin', 'cifar10_sin', 'cifar10_small_sin_nopre', 'cifar10_sin_nopre']
FIXTURES = ['sin_small_b2', 'sin_full_b2', 'sin_small_train_b2', 'sin_fcend_small_b2']


def test_sin_archs_are_listed():
    for name in SIN_ARCHS:
        arch = syn.CONFIGS[name]
        assert arch['act'] == 'sin' and arch['kind'] == 'conv'
        assert arch['preact'] == (not name.endswith('_nopre'))
        assert arch['idim'] == (64 if '_small_' in name else 512)


@pytest.mark.parametrize('name', ['cifar10_small_sin', 'cifar10_small_sin_nopre'])
def test_net_entries_of_a_sin_flow(name):
    """Every net of the flow is conv 3x3, Sin, conv 1x1, Sin, conv 3x3; with preact every net but the first block's
    nets leads with a Sin (implicit_flow.py: the first resblock has no leading activation)."""
    arch = syn.CONFIGS[name]
    m = build_flow(arch, 2)
    C, S = _hip.INF_LAYER_CONV, _hip.INF_ACT_SIN
    blocks = imblocks(m)
    assert len(blocks) == sum(arch['n_blocks'])
    leads = []
    for b in blocks:
        for net in (b.nnet_x, b.nnet_z):
            kinds = [k for k, _ in _hip.net_entries(net)]
            assert kinds[-5:] == [C, S, C, S, C]
            assert kinds[:-5] in ([], [S])
            leads.append(len(kinds) == 6)
    if arch['preact']:
        assert leads == [False, False] + [True] * (len(leads) - 2)
    else:
        assert not any(leads)


@pytest.mark.parametrize('name', ['cifar10_small_sin', 'cifar10_small_sin_nopre'])
def test_state_dict_round_trip(name):
    """The synthetic state dict loads strictly, holds no Swish beta, and comes back from the model bit for bit."""
    arch = syn.CONFIGS[name]
    sd = syn.make_state_dict(arch, 0, power_iters=2)
    assert not any(k.endswith('.beta') for k in sd)
    m = build_flow(arch, 2)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert sorted(back) == sorted(sd)
    for k, v in sd.items():
        assert torch.equal(back[k].cpu(), v), k
    m2 = build_flow(arch, 2)
    m2.load_state_dict(back, strict=True)
    layout = syn.conv_flow_layout(arch)
    acts = {l[0] for chain in layout for kind, info in chain if kind == 'imblock' for l in info['net']
            if l[0] != 'conv'}
    assert acts == {'sin'}


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_arrays_present_and_finite(golden_dir, name):
    path = os.path.join(golden_dir, name + '.npz')
    assert os.path.getsize(path) <= 1 << 20
    g = np.load(path)
    arch = syn.CONFIGS[{'sin_full_b2': 'cifar10_sin', 'sin_fcend_small_b2': 'fcend_small_sin'}.get(name, 'cifar10_small_sin')]
    assert g['x'].shape == (2,) + tuple(arch['input_size'])
    nb = int(g['nblocks'])
    assert nb == sum(arch['n_blocks']) + (2 if arch.get('fc_end') else 0)
    for k in ('loss', 'seed', 'weight_seed'):
        assert k in g.files
    for i in range(nb):
        assert 'b%d_nstep' % i in g.files
    if name.endswith('train_b2'):
        assert any(k.startswith('g:') or k.startswith('gs:') for k in g.files)
        assert all('b%d_bwd_nstep' % i in g.files for i in range(nb))
    else:
        assert g['z'].shape == (2, int(np.prod(arch['input_size']))) and g['logpx'].shape == (2,)
        for i in range(nb):
            for k in ('lowest_step', 'prot_break', 'n_power_series', 'logdet', 'z'):
                assert 'b%d_%s' % (i, k) in g.files
            assert int(g['b%d_prot_break' % i]) == 0
    for k in g.files:
        a = np.asarray(g[k])
        if a.dtype.kind == 'f':
            assert np.isfinite(a).all(), k
