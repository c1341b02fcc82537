"""Host side of the wide fully connected flows: the configs lib/synthetic.py gained for them, their
layouts and state dicts against the modules this package builds and against the fixtures the reference wrote
(tests/golden/make_golden_widefc.py).  No GPU."""
import os

import numpy as np
import pytest
import torch

from lib import synthetic as syn
from lib.configs import build_flow, imblocks
from lib.implicit_flow import FCNet, FCWrapper
from lib.layers import ActNorm1d

NEW = ['fcend_small', 'fc_img_small', 'tab_d43', 'tab_d63']
FIXTURES = {'fcend_small': ['fcend_small_b4', 'fcend_small_inverse_b4'], 'fc_img_small': ['fc_img_small_b4'],
            'tab_d43': ['tab_d43_b64'], 'tab_d63': ['tab_d63_b64']}


@pytest.mark.parametrize('name', NEW)
def test_state_dict_round_trip(name):
    """make_state_dict's keys are exactly the module tree's, and after loading every tensor has the synthetic shape
    and value."""
    arch = syn.CONFIGS[name]
    m = build_flow(arch, 4)
    sd = syn.make_state_dict(arch, 0)
    own = m.state_dict()
    assert list(sd) and set(sd) == set(own)
    m.load_state_dict(sd, strict=True)          # (the conv layers size their u / v on loading)
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == tuple(sd[k].shape) and torch.equal(v, sd[k].to(v.dtype)), k
    assert all(torch.equal(a, b) for a, b in zip(syn.make_state_dict(arch, 0).values(), sd.values()))


def test_fc_end_layout():
    """ImplicitFlow(fc_end=True) on 3 x 8 x 8: two scales; the last one ends in two imBlock(FCNet, FCNet) over the
    flattened 12 x 4 x 4 = 192 features with 128-wide hidden layers and a leading activation (preact), each followed
    by FCWrapper(ActNorm1d(192))."""
    arch = syn.CONFIGS['fcend_small']
    layout = syn.conv_flow_layout(arch)
    assert [[k for k, _ in chain] for chain in layout] == [
        ['logit', 'actnorm', 'imblock', 'actnorm', 'squeeze'],
        ['imblock', 'actnorm', 'fc_imblock', 'fc_actnorm', 'fc_imblock', 'fc_actnorm']]
    info = layout[1][2][1]
    assert info['shape'] == (12, 4, 4)
    assert info['net'] == [('swish',), ('linear', 192, 128), ('swish',), ('linear', 128, 128), ('swish',),
                           ('linear', 128, 192)]
    m = build_flow(arch, 4)
    blocks = imblocks(m)
    assert [type(b.nnet_x) for b in blocks[2:]] == [FCNet, FCNet] and len(blocks) == 4
    chain = list(m.transforms[1].chain)
    assert isinstance(chain[3], FCWrapper) and isinstance(chain[3].fc_module, ActNorm1d)


def test_fc_layout():
    """ImplicitFlow(fc=True): every block and every ActNorm fully connected, width idim, d = 192 at both scales."""
    arch = syn.CONFIGS['fc_img_small']
    layout = syn.conv_flow_layout(arch)
    assert [[k for k, _ in chain] for chain in layout] == [
        ['logit', 'fc_actnorm', 'fc_imblock', 'fc_actnorm', 'squeeze'], ['fc_imblock', 'fc_actnorm']]
    assert [chain[i][1]['net'][1] for chain, i in ((layout[0], 2), (layout[1], 0))] == [('linear', 192, 64)] * 2
    assert all(isinstance(b.nnet_x, FCNet) for b in imblocks(build_flow(arch, 4)))


def test_existing_layouts_unchanged():
    """An arch without 'fc' / 'fc_end' keeps the layout kinds and the state-dict keys it had."""
    for name in ('cifar10_small', 'mnist_small', 'cifar10_small_elu'):
        arch = syn.CONFIGS[name]
        kinds = {k for chain in syn.conv_flow_layout(arch) for k, _ in chain}
        assert kinds <= {'logit', 'actnorm', 'imblock', 'squeeze'}, name
        assert not any('.nnet.' in k or '.fc_module.' in k for k in syn.make_state_dict(arch, 0)), name
    assert syn.CONFIGS['tab_d43']['dims'] == syn.POWER['dims'] and syn.CONFIGS['tab_d63']['d'] == 63


@pytest.mark.parametrize('name', NEW)
def test_fixtures_fit_the_configs(golden_dir, name):
    """Every fixture of the config: as many recorded blocks as the model has imBlocks, inputs and outputs of the
    config's sizes, and a trajectory for every block."""
    arch = syn.CONFIGS[name]
    n_blocks = len(imblocks(build_flow(arch, 4)))
    d = int(np.prod(arch['input_size'])) if arch['kind'] == 'conv' else arch['d']
    for fx in FIXTURES[name]:
        g = np.load(os.path.join(golden_dir, fx + '.npz'))
        assert int(g['nblocks']) == n_blocks, fx
        B = g['logpx'].shape[0]
        assert g['z'].reshape(B, -1).shape == (B, d), fx
        assert g['x'].reshape(B, -1).shape == (B, d), fx
        for i in range(n_blocks):
            assert int(g['b%d_nstep' % i]) >= 1 and int(g['b%d_prot_break' % i]) == 0, fx
            assert len(g['b%d_n_power_series' % i]) == 2, fx


def test_training_fixture_pins_no_backward_steps(golden_dir):
    """fcend_small_train_b2 holds the forward trajectory, the loss and gradient records of the flow's own parameters,
    and no backward-solve step counts (they are not stable in the reference itself)."""
    g = np.load(os.path.join(golden_dir, 'fcend_small_train_b2.npz'))
    m = build_flow(syn.CONFIGS['fcend_small'], 2)
    names = {n for n, _ in m.named_parameters()}
    recorded = {k.split(':', 1)[1] for k in g.files if k.startswith(('g:', 'gs:'))}
    assert recorded and recorded <= names
    assert not [k for k in g.files if '_bwd_' in k]
    assert int(g['nblocks']) == len(imblocks(m)) and all('b%d_nstep' % i in g.files for i in range(4))
