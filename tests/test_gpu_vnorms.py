"""Mixed induced norms (--vnorms) on the engine: the p-norm normalisations of csrc/power.hip against the reference's
own ``compute_weight(update=True)`` (tests/golden/make_golden_vnorms.py), the batched call against the per-layer one,
and flows whose layers carry mixed norms against the reference's fixtures.

Tolerances are the project's (tests/test_gpu_parity.py): u, v, scale within 2e-5 max(1, |ref|_inf), one-hot vectors,
stale buffers and iteration counts exact; bits/dim within 1e-5, per-sample log p within 2e-3 nats; gradients as
tests/test_gpu_train.py.  Workspace and LDS are NaN-poisoned before direct engine calls.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.density import image_logpx, tabular_logpx, tabular_nats_graph
from lib.layers import set_probe_mode

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF = float('inf')
TOL = 2e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PI = np.load(os.path.join(GOLDEN, 'vnorms_power_iter.npz'))
CASES = [str(c) for c in PI['cases'] if c != 'cases']
LAYERS = {l[0]: l for l in syn.VNORM_LAYERS}


def _inputs(cid):
    """(layer tuple, W, u0, v0 on the device, domain, codomain, n_iterations or None) of a fixture case."""
    name = cid.split('/')[0]
    W, u0, v0 = syn.vnorm_layer_inputs(name, int(PI[cid + ':seed']))
    n_it = int(PI[cid + ':n_iterations'])
    return (LAYERS[name], W.to(DEV), u0.to(DEV), v0.to(DEV), float(PI[cid + ':domain']), float(PI[cid + ':codomain']),
            None if n_it < 0 else n_it)


def _desc(layer, W, u, v, scale, dom, cod):
    _, kind, cin, cout, k, hw, _ = layer
    spatial = kind == 'conv' and k > 1
    return _hip.PowerIterDesc(kind=2 if kind == 'linear' else 1, cin=cin, cout=cout, ksize=k,
                              height=hw[0] if spatial else 1, width=hw[1] if spatial else 1, weight=W.data_ptr(),
                              u=u.data_ptr(), v=v.data_ptr(), scale=scale.data_ptr(), domain=dom, codomain=cod)


def _poisoned(nbytes, stream):
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=DEV)
    ws.fill_(255)
    _hip.check(_hip.load().inf_debug_poison_lds(stream), 'poison_lds')
    return ws


def _iterate(layer, W, u0, v0, dom, cod, n_it, status=False):
    """inf_power_iteration from (u0, v0) on copies; returns (u, v, scale, iterations) or, with status, the status."""
    lib = _hip.load()
    u, v, scale = u0.clone(), v0.clone(), torch.full((), float('nan'), device=DEV)
    d = _desc(layer, W, u, v, scale, dom, cod)
    stream = _hip.stream_of(W)
    nbytes = lib.inf_power_iteration_workspace_bytes(ctypes.byref(d))
    if status and nbytes == 0:
        nbytes = 1 << 20
    ws = _poisoned(nbytes, stream)
    used = ctypes.c_int(-1)
    st = lib.inf_power_iteration(ctypes.byref(d), 200 if n_it is None else n_it, int(n_it is None), 1e-3, 1e-3,
                                 ctypes.byref(used), _hip.ptr(ws), ws.numel(), stream)
    torch.cuda.synchronize()
    if status:
        return st
    _hip.check(st, 'inf_power_iteration')
    return u, v, scale, used.value


@pytest.mark.parametrize('cid', CASES)
def test_power_iteration_matches_reference(cid):
    layer, W, u0, v0, dom, cod, n_it = _inputs(cid)
    u, v, scale, used = _iterate(layer, W, u0, v0, dom, cod, n_it)
    assert used == int(PI[cid + ':iters'])
    ref_scale = float(PI[cid + ':scale'])
    print('%s: scale %.8f ref %.8f' % (cid, scale.item(), ref_scale))
    assert abs(scale.item() - ref_scale) <= TOL * max(1., abs(ref_scale))
    name = cid.split('/')[0]
    for key, got, start in (('u', u, u0), ('v', v, v0)):
        got = got.cpu().numpy()
        pre = '%s:%s' % (cid, key)
        if pre + '_stale' in PI:                      # a 1x1 conv's buffer that the reference does not write back
            assert np.array_equal(got, start.cpu().numpy()), key
        elif pre + '_hot' in PI:
            want = np.zeros_like(got)
            want[int(PI[pre + '_hot'])] = 1.
            assert np.array_equal(got, want), key
        elif pre + '_sample' in PI:
            bound = TOL * max(1., float(PI[pre + '_absmax']))
            idx = syn.vnorm_sample_index(name + '.' + key, got.size)
            err = np.abs(got[idx].astype(np.float64) - PI[pre + '_sample']).max()
            print('  %s sample err %.2e bound %.2e' % (key, err, bound))
            assert err <= bound, key
            s, _ = syn.vec_summary(got, 'vnorm.' + name + '.' + key)
            ref = PI[pre + '_summary']
            # |d sum|, |d projection| <= n x the elementwise bound; |d sum of squares| <= 2 |ref|_1 bound + n bound^2
            assert abs(s[0] - ref[0]) <= got.size * bound and abs(s[2] - ref[2]) <= got.size * bound, key
            assert abs(s[1] - ref[1]) <= 2 * np.abs(got).sum() * bound + got.size * bound ** 2, key
        else:
            ref = PI[pre]
            err = np.abs(got.astype(np.float64) - ref).max()
            print('  %s err %.2e' % (key, err))
            assert err <= TOL * max(1., float(np.abs(ref).max())), key


@pytest.mark.parametrize('tol_mode', [False, True])
def test_batch_equals_per_layer(tol_mode):
    """inf_power_iteration_batch over all the fixture layers of one stopping mode, each with its own norms in its
    descriptor, against the per-layer call: iteration counts, u, v and scale bit for bit."""
    lib = _hip.load()
    cids = [c for c in CASES if c.endswith('/tol') == tol_mode]
    ins = [_inputs(c) for c in cids]
    single = [_iterate(*i) for i in ins]
    bufs = [(i[2].clone(), i[3].clone(), torch.full((), float('nan'), device=DEV)) for i in ins]
    descs = (_hip.PowerIterDesc * len(ins))()
    for j, (i, (u, v, s)) in enumerate(zip(ins, bufs)):
        descs[j] = _desc(i[0], i[1], u, v, s, i[4], i[5])
    stream = _hip.stream_of(ins[0][1])
    ws = _poisoned(lib.inf_power_iteration_batch_workspace_bytes(descs, len(ins)), stream)
    used = (ctypes.c_int * len(ins))()
    _hip.check(lib.inf_power_iteration_batch(descs, len(ins), 200 if tol_mode else 5, int(tol_mode), 1e-3, 1e-3, used,
                                             _hip.ptr(ws), ws.numel(), stream), 'inf_power_iteration_batch')
    torch.cuda.synchronize()
    for j, cid in enumerate(cids):
        assert used[j] == single[j][3], cid
        for a, b, what in zip(bufs[j], single[j][:3], 'uvs'):
            assert torch.equal(a, b), (cid, what)


def test_tie_goes_to_the_lowest_index():
    layer = ('tie', 'linear', 2, 2, 1, None, None)
    W = torch.tensor([[1., 0.], [1., 0.]], device=DEV)
    u0, v0 = torch.tensor([0., 1.], device=DEV), torch.tensor([1., 0.], device=DEV)
    u, v, scale, _ = _iterate(layer, W, u0, v0, 2., INF, 1)
    assert u.tolist() == [1., 0.]
    assert scale.item() == 1.


def test_zero_norms_stand_for_two_and_bad_norms_are_refused():
    layer = LAYERS['conv3_6x5']
    W, u0, v0 = (t.to(DEV) for t in syn.vnorm_layer_inputs('conv3_6x5', 0))
    a = _iterate(layer, W, u0, v0, 0., 0., 5)
    b = _iterate(layer, W, u0, v0, 2., 2., 5)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    for dom, cod in ((0.5, 2.), (2., 0.5), (float('nan'), 2.), (-INF, 2.), (2., -1.)):
        assert _iterate(layer, W, u0, v0, dom, cod, 5, status=True) == 1        # INF_ERR_INVALID


def test_modules_pass_their_norms():
    """compute_weight(update=True) and compute_one_iter of a device module against the same module on the host."""
    from lib.layers.base import lipschitz_ops as lo
    torch.manual_seed(2)
    for m in (lo.InducedNormLinear(9, 6, domain=3, codomain=INF, n_iterations=4),
              lo.InducedNormConv2d(3, 5, 3, 1, 1, domain=1, codomain=3, n_iterations=4)):
        with torch.no_grad():
            if isinstance(m, lo.InducedNormConv2d):
                m(torch.zeros(1, 3, 6, 5))
            m.weight.add_(0.3 * torch.randn_like(m.weight))
        dev = copy.deepcopy(m).to(DEV)
        with torch.no_grad():
            one_host, one_dev = m.compute_one_iter(), dev.compute_one_iter()
            assert abs(one_dev.item() - one_host.item()) <= TOL * max(1., abs(one_host.item()))
            m.compute_weight(update=True)
            dev.compute_weight(update=True)
        for name in ('u', 'v', 'scale'):
            ref = getattr(m, name)
            err = (getattr(dev, name).cpu() - ref).abs().max().item()
            assert err <= TOL * max(1., ref.abs().max().item()), name


# ---- flows ----------------------------------------------------------------------------------------------------
def _flow(arch_name, g):
    arch = syn.CONFIGS[arch_name]
    x = torch.from_numpy(g['x']).to(DEV)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    return arch, m.to(DEV), x


@pytest.mark.parametrize('name,arch_name', [('vnorms_cifar_small_b4', 'cifar10_small_13f1'),
                                            ('vnorms_fc_b16', 'fc_2332')])
def test_flow_matches_reference_fixture(name, arch_name):
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    arch, m, x = _flow(arch_name, g)
    m.eval()
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    loss, logpx, z = image_logpx(m, x, arch['nvals']) if arch['kind'] == 'conv' else tabular_logpx(m, x)
    torch.cuda.synchronize()
    blocks = imblocks(m)
    assert len(blocks) == int(g['nblocks'])
    for i, b in enumerate(blocks):
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'block %d nstep' % i
        assert b.last_broyden['lowest_step'] == int(g['b%d_lowest_step' % i]), 'block %d lowest_step' % i
        if 'b%d_n_power_series' % i in g:
            assert b.last_n_power_series == int(g['b%d_n_power_series' % i][0]), 'block %d series' % i
    print('loss %.8f ref %.8f |d| %.2e' % (loss.item(), float(g['loss']), abs(loss.item() - float(g['loss']))))
    assert abs(loss.item() - float(g['loss'])) <= 1e-5
    np.testing.assert_allclose(logpx.view(-1).cpu().numpy(), g['logpx'], rtol=0, atol=2e-3)


def test_training_gradients_match_reference():
    """vnorms_fc_train_b16: the loss and every parameter gradient of the reference's loss.backward(), at
    tests/test_gpu_train.py's bounds (|g - g_ref| <= 2e-3 max |g_ref| per tensor), with no torch forward of a net."""
    from lib.layers.base import lipschitz_ops as lo
    g = np.load(os.path.join(GOLDEN, 'vnorms_fc_train_b16.npz'))
    arch, m, x = _flow('fc_2332', g)
    m.train()
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    calls = []
    real = lo.InducedNormLinear.forward

    def spy(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    lo.InducedNormLinear.forward = spy
    try:
        loss, logpx, z = tabular_nats_graph(m, x)
        loss.backward()
    finally:
        lo.InducedNormLinear.forward = real
    torch.cuda.synchronize()
    for i, b in enumerate(imblocks(m)):
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'block %d forward nstep' % i
    assert abs(loss.item() - float(g['loss'])) <= 1e-5, (loss.item(), float(g['loss']))
    assert not calls, 'a net module ran its torch forward in the training step'
    named = dict(m.named_parameters())
    keys = [k for k in g.files if k.startswith('g:')]
    assert keys and not [k for k in g.files if k.startswith('gs:')]
    for key in keys:
        ref = g[key].astype(np.float64)
        p = named[key[2:]]
        assert p.grad is not None, key
        got = p.grad.detach().double().cpu().numpy().ravel()
        scale = max(np.abs(ref).max(), 1e-12)
        err = np.abs(got - ref).max()
        assert err <= 2e-3 * scale + 1e-9, '%s: max err %g vs scale %g' % (key, err, scale)


def test_update_lipschitz_batch_matches_per_layer():
    """update_lipschitz on the '13f1' flow after a weight perturbation (one batched engine call, the norms per layer)
    against compute_weight(update=True) layer by layer on a copy: counts, u, v and scale bit for bit, the 1x1 convs'
    stale u among them."""
    from lib.layers import base
    from lib.utils import update_lipschitz
    arch = syn.CONFIGS['cifar10_small_13f1']
    m = build_flow(arch, 2)
    sd = syn.make_state_dict(arch, 0)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    torch.manual_seed(3)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.02 * torch.randn_like(p))          # as after an optimiser step
    ref = copy.deepcopy(m)
    kinds = (base.InducedNormConv2d, base.InducedNormLinear)
    update_lipschitz(m)
    with torch.no_grad():
        for q in ref.modules():
            if isinstance(q, kinds):
                q.compute_weight(update=True)
    torch.cuda.synchronize()
    n = stale = 0
    for (key, a), b in zip(m.named_modules(), ref.modules()):
        if isinstance(a, kinds):
            assert a.last_power_iters == b.last_power_iters
            for name in ('u', 'v', 'scale'):
                assert torch.equal(getattr(a, name), getattr(b, name)), name
            if isinstance(a, base.InducedNormConv2d) and a.is_1x1 and a.codomain == INF:
                assert torch.equal(a.u.cpu(), sd[key + '.u']), key          # not written back
                stale += 1
            n += 1
    assert n > 0 and stale > 0
