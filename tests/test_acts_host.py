"""Host-side checks of the activation table's other entries (nn.ELU, nn.Softplus, nn.ReLU, LipschitzCube, Identity,
Zero) and of bias-free layers: the module -> engine-kind mapping of lib._hip.net_entries, and the synthetic state dicts
of the architectures that carry them (lib/synthetic.py).  No GPU."""
import zlib

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow
from lib.implicit_flow import ACT_FNS
from lib.layers.base import get_conv2d, get_linear

KINDS = {'swish': _hip.INF_ACT_SWISH, 'sin': _hip.INF_ACT_SIN, 'elu': _hip.INF_ACT_ELU,
         'softplus': _hip.INF_ACT_SOFTPLUS, 'relu': _hip.INF_ACT_RELU, 'lcube': _hip.INF_ACT_LCUBE,
         'identity': _hip.INF_ACT_IDENTITY, 'zero': _hip.INF_ACT_ZERO}


def _conv(a, b, k, bias=True):
    return get_conv2d(a, b, k, 1, k // 2, coeff=0.9, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2,
                      bias=bias)


def test_kind_values_follow_the_header():
    """include/inflow.h InfLayerKind: the existing values unchanged, the new ones after INF_ACT_SIN."""
    assert (_hip.INF_LAYER_CONV, _hip.INF_LAYER_LINEAR, _hip.INF_ACT_SWISH, _hip.INF_ACT_SIN) == (1, 2, 3, 4)
    assert [KINDS[a] for a in ('elu', 'softplus', 'relu', 'lcube', 'identity', 'zero')] == [5, 6, 7, 8, 9, 10]
    assert sorted(KINDS) == sorted(ACT_FNS)


@pytest.mark.parametrize('lead', [False, True])
@pytest.mark.parametrize('act', sorted(KINDS))
def test_net_entries_maps_every_activation(act, lead):
    mods = [ACT_FNS[act](False)] if lead else []
    mods += [_conv(3, 8, 3), ACT_FNS[act](True), _conv(8, 8, 1), ACT_FNS[act](True), _conv(8, 3, 3)]
    entries = _hip.net_entries(torch.nn.Sequential(*mods))
    assert entries is not None
    C, A = _hip.INF_LAYER_CONV, KINDS[act]
    assert [k for k, _ in entries] == ([A] if lead else []) + [C, A, C, A, C]
    assert [m for _, m in entries] == mods
    fc = torch.nn.Sequential(get_linear(6, 16), ACT_FNS[act](True), get_linear(16, 6))
    assert [k for k, _ in _hip.net_entries(fc)] == [_hip.INF_LAYER_LINEAR, A, _hip.INF_LAYER_LINEAR]


def test_net_entries_accepts_bias_free_layers():
    seq = torch.nn.Sequential(_conv(3, 8, 3, bias=False), torch.nn.ReLU(), _conv(8, 3, 3))
    assert seq[0].bias is None
    entries = _hip.net_entries(seq)
    assert [k for k, _ in entries] == [_hip.INF_LAYER_CONV, _hip.INF_ACT_RELU, _hip.INF_LAYER_CONV]
    fc = torch.nn.Sequential(get_linear(6, 16, bias=False), torch.nn.ELU(), get_linear(16, 6, bias=False))
    assert [k for k, _ in _hip.net_entries(fc)] == [_hip.INF_LAYER_LINEAR, _hip.INF_ACT_ELU, _hip.INF_LAYER_LINEAR]
    # the tensor list behind the version stamps skips the missing biases
    assert all(t is not None for t in _hip.NativeNet._tensors_of(entries))
    assert len(_hip.NativeNet._tensors_of(entries)) == 3 + 4


@pytest.mark.parametrize('mod', [torch.nn.ELU(alpha=0.5), torch.nn.Softplus(beta=2), torch.nn.Softplus(threshold=10),
                                 torch.nn.LeakyReLU(), torch.nn.Tanh()])
def test_net_entries_refuses_other_parameter_values(mod):
    """Only the default parameter values have kernels; anything else is no engine net (native_net raises HipError)."""
    assert _hip.net_entries(torch.nn.Sequential(_conv(3, 8, 3), mod, _conv(8, 3, 3))) is None


def test_inplace_does_not_matter():
    for mod in (torch.nn.ELU(inplace=True), torch.nn.ReLU(inplace=True)):
        assert _hip.net_entries(torch.nn.Sequential(_conv(3, 8, 3), mod, _conv(8, 3, 3))) is not None


NEW_ARCHS = sorted(k for k in syn.CONFIGS if k.split('_')[-1] in syn.NEW_ACTS)


def test_new_archs_are_listed():
    want = ['cifar10_small_' + a for a in syn.NEW_ACTS] + ['cifar10_' + a for a in ('elu', 'softplus', 'relu')]
    assert sorted(want + ['power_elu', 'toy_softplus']) == NEW_ARCHS
    for name in NEW_ARCHS:
        assert syn.CONFIGS[name]['act'] == name.split('_')[-1]


@pytest.mark.parametrize('name', NEW_ARCHS)
def test_state_dict_of_new_archs_loads_strict(name):
    arch = syn.CONFIGS[name]
    B = 2
    sd = syn.make_state_dict(arch, 0, power_iters=2)
    assert not any(k.endswith('.beta') for k in sd)          # Swish is the only activation with a parameter
    m = build_flow(arch, B)
    m.load_state_dict(sd, strict=True)
    layout = syn.conv_flow_layout(arch) if arch['kind'] == 'conv' else None
    if layout is not None:
        acts = {l[0] for chain in layout for kind, info in chain if kind == 'imblock' for l in info['net']
                if l[0] != 'conv'}
        assert acts == {arch['act']}


def test_existing_arch_state_dict_is_unchanged(golden_dir):
    """conv_flow_layout now emits arch['act'] where it hard-coded 'swish': for the Swish archs the state dict must be
    the one the committed fixtures were made with.  Key list and the rng-drawn tensors (weights, biases, betas: numpy
    PCG64 keyed by name, the same bits on every machine) against checksums taken before the change, at the weight seed
    cifar_small_b4 records."""
    g = np.load(golden_dir + '/cifar_small_b4.npz')
    sd = syn.make_state_dict(syn.CIFAR10_SMALL, int(g['weight_seed']))
    assert len(sd) == 617
    assert zlib.crc32('\n'.join(sd.keys()).encode()) == 765472296
    want = {'transforms.0.chain.2.nnet_x.0.weight': 4105400389, 'transforms.0.chain.4.nnet_z.0.beta': 807662920,
            'transforms.2.chain.2.nnet_z.5.bias': 3842798968, 'transforms.2.chain.2.nnet_x_copy.3.weight': 321787641,
            'transforms.0.chain.1.weight': 1962306840}
    for k, crc in want.items():
        assert zlib.crc32(sd[k].numpy().tobytes()) == crc, k
    net = syn.conv_flow_layout(syn.CIFAR10_SMALL)[0][4][1]['net']
    assert [l[0] for l in net] == ['swish', 'conv', 'swish', 'conv', 'swish', 'conv']
