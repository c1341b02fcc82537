"""Mixed induced norms (--vnorms) on the host: the normalisations, construction with the reference's restarts, the
model surface and the oracle against the reference's fixtures (tests/golden/make_golden_vnorms.py).  CPU only."""
import os

import numpy as np
import pytest
import torch

from lib import synthetic as syn
from lib.configs import build_flow
from lib.implicit_flow import ImplicitFlow
from lib.layers.base import lipschitz_ops as lo
from oracle import inflow_oracle as orc

INF = float('inf')
X = [0.5, -2., 0., 1.]


@pytest.mark.parametrize('fn,p,want', [
    (lo.normalize_v, INF, [1., -1., 1., 1.]),
    (lo.normalize_u, 1, [1., -1., 1., 1.]),
    (lo.normalize_v, 3, [0.4389, -0.8778, 0., 0.6207]),
    (lo.normalize_u, 3, [0.0573, -0.9160, 0., 0.2290]),
    (lo.normalize_v, 1, [0., 1., 0., 0.]),
    (lo.normalize_u, INF, [0., 1., 0., 0.]),
])
def test_normalisations(fn, p, want):
    """The values of the reference's normalize_u / normalize_v on [0.5, -2, 0, 1] (4 decimals)."""
    got = fn(torch.tensor(X), p)
    assert got.dtype == torch.float32
    np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=5e-5)
    if p in (1, INF):
        assert got.tolist() == want                      # the one-hot and sign forms are exact


def test_one_hot_tie_goes_to_the_lowest_index_and_drops_the_sign():
    assert lo.normalize_v(torch.tensor([1., -3., 3., 0.]), 1).tolist() == [0., 1., 0., 0.]


@pytest.mark.parametrize('tag', ['1_inf', '3_3'])
def test_construction_matches_reference(golden_dir, tag):
    """InducedNormLinear(5, 7, domain, codomain) built on the CPU under the fixture's seed: the same draws, the same
    ten restarts under the reference's rule, so the same buffers.  One-hot vectors exactly, the rest within
    2e-5 max(1, |ref|_inf)."""
    g = np.load(os.path.join(golden_dir, 'vnorms_construct.npz'))
    dom, cod = float(g[tag + ':domain']), float(g[tag + ':codomain'])
    torch.manual_seed(int(g[tag + ':seed']))
    m = lo.InducedNormLinear(5, 7, domain=dom, codomain=cod)
    sd = m.state_dict()
    assert set(sd) == {k.split(':sd:')[1] for k in g.files if k.startswith(tag + ':sd:')}
    for name in ('weight', 'bias'):
        assert np.array_equal(sd[name].numpy(), g['%s:sd:%s' % (tag, name)]), name     # the same draws
    for name, hot in (('u', cod == INF), ('v', dom == 1), ('scale', False)):
        ref = g['%s:sd:%s' % (tag, name)]
        if hot:
            assert np.array_equal(sd[name].numpy(), ref), name
        else:
            np.testing.assert_allclose(sd[name].numpy(), ref, rtol=0, atol=2e-5 * max(1., float(np.abs(ref).max())))


def test_one_by_one_conv_keeps_the_reference_stale_buffers():
    """A 1x1 conv's update leaves the stored v (domain 1) and u (codomain inf) as they were, while `scale` receives
    sigma of the iterated vectors; the next update=False evaluation recomputes sigma from the stored buffers."""
    torch.manual_seed(0)
    m = lo.InducedNormConv2d(3, 5, 1, 1, 0, domain=1, codomain=INF, n_iterations=5)
    with torch.no_grad():
        m(torch.zeros(1, 3, 4, 4))
        m.u.copy_(torch.tensor([.1, .2, .3, .4, .5]))
        m.v.copy_(torch.tensor([.3, .2, .1]))
        u0, v0 = m.u.clone(), m.v.clone()
        m.compute_weight(update=True)
        assert torch.equal(m.u, u0) and torch.equal(m.v, v0)
        W = m.weight.view(5, 3)
        # the 1 -> inf norm is max |entry|; the one-hot forms drop the sign, so sigma is that entry, sign and all
        assert abs(abs(m.scale.item()) - W.abs().max().item()) < 1e-6
        m.compute_weight(update=False)
        assert abs(m.scale.item() - torch.dot(u0, W @ v0).item()) < 1e-6


def test_model_surface():
    """vnorms with a digit >= 3 in any position, and with 1 / f where the reference still builds InducedNorm layers,
    construct on the conv and the fc path, print their norms, and keep them per layer."""
    for vn in ('3222', '2322', '2232', '2223', '13f1'):
        m = ImplicitFlow((2, 3, 8, 8), n_blocks=[1], intermediate_dim=8, vnorms=vn, sn_atol=1e-3, sn_rtol=1e-3,
                         kernels='3-1-3', actnorm=False, factor_out=False)
        convs = [q for q in m.modules() if isinstance(q, lo.InducedNormConv2d)][:3]
        ps = [INF if c == 'f' else float(c) for c in vn]
        assert [(q.domain, q.codomain) for q in convs] == list(zip(ps[:-1], ps[1:]))
        assert 'domain=%.2f, codomain=%.2f' % (ps[0], ps[1]) in repr(convs[0])
    m = ImplicitFlow((2, 3, 4, 4), n_blocks=[1], intermediate_dim=8, vnorms='2352', sn_atol=1e-3, sn_rtol=1e-3,
                     kernels='3-1-3', actnorm=False, factor_out=False, fc=True)
    lins = [q for q in m.modules() if isinstance(q, lo.InducedNormLinear)][:3]
    assert [(q.domain, q.codomain) for q in lins] == [(2., 3.), (3., 5.), (5., 2.)]
    assert lins[0].compute_domain_codomain() == (2., 3.)


def test_still_refused():
    """A learnable order (tensor-valued domain, learn_p) is out of scope; so are the norm pairs for which the
    reference's factories build its closed-form LopLinear / LopConv2d, the default '122f' among them; so is a norm
    below 1."""
    with pytest.raises(NotImplementedError, match='learn_p'):
        lo.InducedNormLinear(4, 4, domain=torch.nn.Parameter(torch.tensor(0.)), codomain=2)
    with pytest.raises(NotImplementedError, match='learn_p'):
        lo.InducedNormConv2d(4, 4, 3, 1, 1, domain=2, codomain=torch.tensor(2.))
    with pytest.raises(NotImplementedError, match='learn_p'):
        ImplicitFlow((2, 3, 8, 8), n_blocks=[1], intermediate_dim=8, vnorms='2222', sn_atol=1e-3, sn_rtol=1e-3,
                     learn_p=True)
    for dom, cod in ((1, 1), (1, 2), (1, INF), (2, INF), (INF, INF)):
        with pytest.raises(NotImplementedError, match='Lop'):
            lo.get_linear(4, 4, domain=dom, codomain=cod)
        with pytest.raises(NotImplementedError, match='Lop'):
            lo.get_conv2d(4, 4, 3, 1, 1, domain=dom, codomain=cod)
        lo.InducedNormLinear(4, 4, domain=dom, codomain=cod)          # the layer itself takes any pair
    with pytest.raises(NotImplementedError, match='Lop'):
        ImplicitFlow((2, 3, 8, 8), n_blocks=[1], intermediate_dim=8, sn_atol=1e-3, sn_rtol=1e-3)   # vnorms='122f'
    with pytest.raises(ValueError):
        lo.InducedNormLinear(4, 4, domain=0.5, codomain=2)


FLOWS = [('vnorms_cifar_small_b4', 'cifar10_small_13f1'), ('vnorms_fc_b16', 'fc_2332')]


@pytest.mark.parametrize('name,arch_name', FLOWS)
def test_flow_state_dict_round_trip(name, arch_name):
    """The flow builds with its vnorms, loads the fixture's state dict (regenerated from its seed) with strict=True
    and gives it back unchanged."""
    arch = syn.CONFIGS[arch_name]
    sd = syn.make_state_dict(arch, 0)
    m = build_flow(arch, 4)
    m.load_state_dict(sd, strict=True)
    back = m.state_dict()
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    norms = syn.layer_norms(arch)
    layers = [q for q in m.modules() if isinstance(q, (lo.InducedNormConv2d, lo.InducedNormLinear))]
    assert {(q.domain, q.codomain) for q in layers} == set(norms)


@pytest.mark.parametrize('name,arch_name', FLOWS)
def test_oracle_matches_reference(golden_dir, name, arch_name):
    """The oracle takes sigma = u . (W v) from the stored buffers whatever the norm, so it referees the GPU tests of
    these flows: tolerances of test_oracle_golden.py.  (Passes without the feature.)"""
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    arch = syn.CONFIGS[arch_name]
    sd = syn.make_state_dict(arch, int(g['weight_seed']))
    layout = syn.conv_flow_layout(arch) if arch['kind'] == 'conv' else syn.fc_flow_layout(arch)
    flow = orc.build(arch, sd, layout, training=False)
    x = torch.from_numpy(g['x'])
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    if arch['kind'] == 'conv':
        loss, logpx, z = orc.image_bits_per_dim(flow, x, arch['nvals'])
    else:
        loss, logpx, z = orc.tabular_nats(flow, x)
    blocks = flow.blocks()
    assert len(blocks) == int(g['nblocks'])
    for i, b in enumerate(blocks):
        assert b.record['nstep'] == int(g['b%d_nstep' % i])
        assert b.record['lowest_step'] == int(g['b%d_lowest_step' % i])
        if 'b%d_n_power_series' % i in g:
            assert b.record['n_power_series'] == int(g['b%d_n_power_series' % i][0])
    assert abs(float(loss) - float(g['loss'])) < 1e-5
    np.testing.assert_allclose(logpx.view(-1).numpy(), g['logpx'], rtol=0, atol=2e-3)
    np.testing.assert_allclose(z.numpy().reshape(z.shape[0], -1), g['z'], rtol=0, atol=2e-4)
