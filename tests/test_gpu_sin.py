"""Sin conv and fc nets with a leading Sin (preact) on the MI355X engine, and Sin conv nets on the fused 3-1-3 kernels.
The oracle knows no leading Sin, so the references are fp64 torch evaluations of the same modules and fixtures from the
reference itself (tests/golden/make_golden_sin.py).

Tolerances (tests/test_gpu_acts.py's and tests/test_gpu_train.py's):
  * net forward / VJP against fp64:      |delta| <= 2e-5 * max(1, |ref|_inf)
  * fused against generic:                1e-5 * max(1, |ref|_inf)
  * engine parameter gradients / fp64:    2e-4 of the tensor's max, the surrogate's value 1e-5
  * fixtures: Broyden nstep / lowest_step and series lengths exact, loss within 1e-5, gradients 2e-3 of the tensor's max
Workspace and LDS are filled with NaN before every direct engine call (test_gpu_acts._engine).
"""
import copy
import os

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.density import image_bits_per_dim_graph, image_logpx
from lib.layers import imBlock, netgrad, set_probe_mode
from lib.layers.base import Sin, Swish
from test_gpu_acts import _check_flow, _close, _conv, _engine, _fp64, _golden, _lin
from test_gpu_train import _check_grads, _check_param

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# Layer-0 inputs of a leading Sin: its zeros (0, +-0.5), its extrema (+-0.25, where the short form's fold sits), and
# points several periods out, up to |x| ~ 40
SPECIAL = [0., 0.25, -0.25, 0.5, -0.5, 3.25, -7.5, 12.125, 39.75, -40., 17.3, -23.61, 5.0625, -31.4]


def _with_specials(x):
    x = x.clone()
    flat = x.view(x.shape[0], -1)
    vals = torch.tensor(SPECIAL)
    n = min(len(vals), flat.shape[1])          # d = 5 holds five of them: the values rotate over the samples
    for b in range(flat.shape[0]):
        flat[b, :n] = torch.roll(vals, -n * b)[:n]
    return x


@pytest.mark.parametrize('kind', ['conv', 'fc5', 'fc43'])
def test_generic_path_leading_sin_matches_fp64(kind, monkeypatch):
    """Generic path (INFLOW_NO_FUSED=1): the EP_ACT_SIN GEMM loader's leading Sin and the derivative multiply of
    conv_out / fc_out / fc_out_wide (d = 43 > 32), inf_net_forward and inf_net_vjp against fp64 torch.  conv: (3, 8, 8),
    hidden 64, kernels 3-1-3, B = 3; fc: d = 5 and d = 43, 64-64, B = 5."""
    monkeypatch.setenv('INFLOW_NO_FUSED', '1')
    torch.manual_seed(3)
    if kind == 'conv':
        shape, B = (3, 8, 8), 3
        seq = torch.nn.Sequential(Sin(), _conv(3, 64, 3), Sin(), _conv(64, 64, 1), Sin(), _conv(64, 3, 3)).to(DEV)
    else:
        d = int(kind[2:])
        shape, B = (d,), 5
        seq = torch.nn.Sequential(Sin(), _lin(d, 64), Sin(), _lin(64, 64), Sin(), _lin(64, d)).to(DEV)
    with torch.no_grad():
        seq(torch.zeros(1, *shape, device=DEV))              # lazy u/v (engine power iteration)
    x = _with_specials(torch.randn(B, *shape) * 0.7).to(DEV)
    v = torch.randn(B, *shape).to(DEV)
    y, g, _, tags = _engine(seq, shape, x, v)
    assert not any(500 <= t < 700 for t in tags), sorted(tags)        # no fused kernel
    y_ref, g_ref = _fp64(seq, x, v)
    _close(y, y_ref)
    _close(g, g_ref)


def _sin313(C, H, hid, lead, seed=2):
    """conv 3x3, Sin, conv 1x1, Sin, conv 3x3 on (C, H, H), with a leading Sin or without.  The weights are scaled by 3
    (every layer's Lipschitz normalisation is active, sigma = coeff) and the two hidden biases are uniform in
    (-2.5, 2.5), so that the hidden pre-activations span several periods of sin(2 pi a) whatever the layer's input:
    a Sin layer's output is at most 1 / (2 pi) in magnitude, so without the biases the second hidden pre-activation
    would stay within a fraction of one period."""
    torch.manual_seed(seed)
    mods = ([Sin()] if lead else []) + [_conv(C, hid, 3), Sin(), _conv(hid, hid, 1), Sin(), _conv(hid, C, 3)]
    seq = torch.nn.Sequential(*mods).to(DEV)
    with torch.no_grad():
        seq(torch.zeros(1, C, H, H, device=DEV))             # lazy u/v (engine power iteration)
        for m in seq:
            if hasattr(m, 'weight'):
                m.weight.mul_(3.0)
        for m in list(seq)[-5:-1:2]:
            m.bias.uniform_(-2.5, 2.5)
        for m in seq:
            if hasattr(m, 'weight'):
                m.compute_weight(update=True)
    return seq


def _check_preacts_span_periods(seq, x):
    """The two hidden pre-activations of seq at x (torch, the modules' own forward): each must reach below -1.5 and
    above 1.5 (more than three periods), and at least a fifth of its elements must lie past the +-0.25 fold of the short
    sine's reduction (|a - rint(a)| > 0.25; a uniform phase gives a half)."""
    h = x
    with torch.no_grad():
        for i, m in enumerate(seq):
            if isinstance(m, Sin) and i > 0:
                assert h.min().item() < -1.5 and h.max().item() > 1.5, (h.min().item(), h.max().item())
                folded = ((h - torch.round(h)).abs() > 0.25).float().mean().item()
                assert folded > 0.2, folded
            h = m(h)


# (C, H, hid, B): test_gpu_acts.FUSED_SHAPES (scale 0 at B = 2 and, to reach the 128-pixel kernel, B = 16; the
# one-row-block-per-wave hid-256 instantiation; the wide kernel) and one ragged shape (28 x 28 cuts into no whole tile)
FUSED_SHAPES = [(3, 32, 512, 2), (12, 16, 256, 2), (48, 8, 512, 3), (3, 32, 512, 16), (1, 28, 256, 2)]


@pytest.mark.parametrize('lead', [False, True])
@pytest.mark.parametrize('C,H,hid,B', FUSED_SHAPES)
def test_fused_313_sin_matches_generic(C, H, hid, B, lead, monkeypatch):
    """The fused 3-1-3 kernels' Sin case (forward-mode epilogues of the kind-switch instantiations, the halo staging's
    leading Sin and its derivative in series chaining) against the generic GEMM chain: inf_net_forward, inf_net_vjp
    and a 6-term inf_logdet_series within 1e-5 max(1, |ref|), in all three inf_net_set_mfma modes, at (3, 32, 512, B)
    under INF_OPT_FUSED_K128 0 and 2; a fused kernel must have run (launch profile)."""
    seq = _sin313(C, H, hid, lead)
    x = (torch.randn(B, C, H, H) * 1.5).to(DEV)              # a leading Sin sees several periods too
    v = torch.randn(B, C, H, H).to(DEV)
    _check_preacts_span_periods(seq, x)
    monkeypatch.setenv('INFLOW_NO_FUSED', '1')
    ref = _engine(seq, (C, H, H), x, v, series=6)
    assert not any(500 <= t < 550 for t in ref[3]), sorted(ref[3])
    monkeypatch.setenv('INFLOW_NO_FUSED', '0')
    for mfma in (0, 1, 2):
        for k128 in ((0, 2) if (C, H) == (3, 32) else (None,)):
            out = _engine(seq, (C, H, H), x, v, mfma=mfma, series=6, k128=k128)
            fused = sorted(t for t in out[3] if 500 <= t < 550)
            print((C, H, hid, B), 'lead', lead, 'mfma', mfma, 'k128', k128, 'fused tags', fused)
            # forward (EVAL), derivative-saving forward (SAVE) and VJP launches of a fused family
            assert {t % 10 for t in fused} >= {0, 1, 2}, sorted(out[3])
            if k128 == 2 and mfma == 2 and B == 16:
                assert {530, 531, 532} <= set(fused), fused               # the 128-pixel kernel: EVAL, SAVE, VJP
            if k128 == 0:
                assert not any(530 <= t < 540 for t in fused), fused
            for a, b in zip(out[:3], ref[:3]):
                _close(a, b, rel=1e-5)


def _block(act_x, act_z, C, hid, lead=True):
    from lib.implicit_flow import ACT_FNS

    def nnet(act):
        A = lambda: ACT_FNS[act](False)
        return torch.nn.Sequential(*(([A()] if lead else []) +
                                     [_conv(C, hid, 3), A(), _conv(hid, hid, 1), A(), _conv(hid, C, 3)]))
    return imBlock(nnet(act_x), nnet(act_z), n_dist='poisson', n_power_series=None, exact_trace=False,
                   brute_force=False, n_samples=1, n_exact_terms=10, neumann_grad=True, grad_in_forward=True,
                   eps_forward=1e-6)


@pytest.mark.parametrize('act_x,act_z', [('sin', 'sin'), ('sin', 'elu')])
def test_block_of_sin_nets_fused_matches_generic(act_x, act_z, monkeypatch):
    """One imBlock on (12, 16, 16) of two 256-wide nets with leading activations, fused and with INFLOW_NO_FUSED=1: the
    same Broyden nstep and series length, z and the block's log-det (the difference of the two nets' series) within
    1e-5.  sin / sin: both nets in the pair launches of the kind-switch instantiations.  sin / elu: Sin shares a pair
    launch with another kind of the switch family (the kind is per net)."""
    C, H, hid, B = 12, 16, 256, 2
    torch.manual_seed(4)
    blk = _block(act_x, act_z, C, hid).to(DEV)
    with torch.no_grad():
        for net in (blk.nnet_x, blk.nnet_z):
            net(torch.zeros(1, C, H, H, device=DEV))                      # lazy u / v (engine power iteration)
    blk.eval()
    x = (torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV)
    res = {}
    for mode in ('generic', 'fused'):
        monkeypatch.setenv('INFLOW_NO_FUSED', '1' if mode == 'generic' else '0')
        b = copy.deepcopy(blk)                                            # its own engine nets: reads INFLOW_NO_FUSED
        set_probe_mode('reference')
        np.random.seed(11)
        torch.manual_seed(11)
        _hip.profile_begin(20000)
        try:
            with torch.no_grad():
                z, lp = b(x, torch.zeros(B, 1, device=DEV))
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        assert any(500 <= t < 550 for t in tags) == (mode == 'fused'), sorted(tags)
        res[mode] = (z, lp, b.last_broyden['nstep'], b.last_n_power_series)
    print('nstep / series length: fused %s generic %s' % (res['fused'][2:], res['generic'][2:]))
    assert res['fused'][2:] == res['generic'][2:]
    _close(res['fused'][0], res['generic'][0], rel=1e-5)
    _close(res['fused'][1], res['generic'][1], rel=1e-5)


@pytest.mark.parametrize('C,hid,H,fused', [(12, 64, 8, False), (3, 256, 16, True)])
def test_engine_param_and_surrogate_grads_with_leading_sin(C, hid, H, fused):
    """inf_net_param_grad / inf_net_surrogate_grad of a conv net that leads with a Sin against fp64 torch autograd through
    the same modules (compute_weight(update=False) keeps the Lipschitz normalisation in the graph), at
    test_gpu_train.test_engine_param_and_surrogate_grads_match_autograd's bounds.  (12, 64, 8): a net of the generic
    path; (3, 256, 16): a net that takes the fused kernels in its forward and VJP."""
    torch.manual_seed(1)
    conv = lambda a, b, k: _conv(a, b, k)
    net = torch.nn.Sequential(Sin(), conv(C, hid, 3), Sin(), conv(hid, hid, 1), Sin(), conv(hid, C, 3)).to(DEV)
    with torch.no_grad():
        net(torch.zeros(1, C, H, H, device=DEV))
        for m in net:
            if hasattr(m, 'weight'):
                m.weight.mul_(3.0)               # sigma / coeff > 1: the normalisation is active
        for m in net:
            if hasattr(m, 'weight'):
                m.compute_weight(update=True)
    B = 2
    x = (torch.randn(B, C, H, H) * 0.5).to(DEV)
    gout = torch.randn(B, C, H, H).to(DEV)
    w = torch.randn(B, C, H, H).to(DEV)
    eps = torch.randn(B, C, H, H).sign().to(DEV)
    params = list(net.parameters())
    native = _hip.native_net(net, (C, H, H), x.device)
    native.refresh_if_needed(_hip.stream_of(x))
    # the fused net really is one: its forward launches a fused kernel
    _hip.profile_begin(2000)
    try:
        ws = _hip.workspace(x.device, native.ws_bytes(B))
        y = torch.empty_like(x)
        _hip.check(native.lib.inf_net_forward(native.handle, _hip.ptr(x), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(),
                                              _hip.stream_of(x)), 'fwd')
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    assert any(500 <= t < 550 for t in tags) == fused, sorted(tags)
    ref_net = copy.deepcopy(net).cpu().double()
    rparams = list(ref_net.parameters())
    d = lambda t: t.detach().cpu().double()
    # first order
    xg = d(x).requires_grad_(True)
    ref = torch.autograd.grad((ref_net(xg) * d(gout)).sum(), rparams + [xg])
    _close(y, ref_net(d(x)))
    got = netgrad.param_grads(native, net, x, gout, want_x=True)
    assert got is not None, 'inf_net_param_grad: INF_ERR_UNSUPPORTED'
    grads, gx = got
    torch.cuda.synchronize()
    for p, r in zip(params, ref[:-1]):
        _check_param(d(grads[p]), r, 'param %s' % (tuple(p.shape),))
    _check_param(d(gx), ref[-1], 'x')
    # surrogate (second order)
    xg = d(x).requires_grad_(True)
    vjp = torch.autograd.grad(ref_net(xg), xg, d(w), create_graph=True)[0]
    s = torch.sum(vjp.view(B, -1) * d(eps).view(B, -1), 1)
    ref2 = torch.autograd.grad(s.sum(), rparams + [xg], allow_unused=True)
    got = netgrad.surrogate_grads(native, net, x, w, eps)
    assert got is not None, 'inf_net_surrogate_grad: INF_ERR_UNSUPPORTED'
    value, grads2, gx2 = got
    torch.cuda.synchronize()
    _check_param(d(value), s.detach(), 'value', rel=1e-5)
    for p, r in zip(params, ref2[:-1]):
        r = torch.zeros_like(d(p)) if r is None else r
        _check_param(d(grads2[p]), r, 'surrogate param %s' % (tuple(p.shape),))
    _check_param(d(gx2), ref2[-1], 'surrogate x')


@pytest.mark.parametrize('name,arch_name', [('sin_small_b2', 'cifar10_small_sin'), ('sin_full_b2', 'cifar10_sin'),
                                            ('sin_fcend_small_b2', 'fcend_small_sin')])
def test_flow_matches_reference_fixture(golden_dir, name, arch_name):
    """The reference's own Sin image flows with preact (every net but the first block's leads with a Sin): per block
    Broyden nstep / lowest_step and series length exact, the loss within 1e-5 (and test_gpu_acts._check_flow's z /
    log-det / log p bounds).  The full-size flow's nets run on the fused kernels; the fc_end flow on 3 x 8 x 8 ends in
    two fc blocks over d = 192 whose FCNets lead with a Sin (the wide fc output stage's derivative multiply)."""
    g = _golden(golden_dir, name)
    arch = syn.CONFIGS[arch_name]
    x = torch.from_numpy(g['x']).to(DEV)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV).eval()
    _hip.profile_begin(100000)
    try:
        _check_flow(m, g, lambda: image_logpx(m, x, arch['nvals']))
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    assert any(500 <= t < 550 for t in tags) == (arch['idim'] == 512), sorted(tags)


def test_training_step_matches_reference_fixture(golden_dir):
    """sin_small_train_b2: the reference's loss.backward() of the preact Sin flow; the engine computes the parameter
    gradients of every block (_engine_grads true, no torch forward of a net layer), the loss within 1e-5, forward and
    backward Broyden step counts exact, every parameter gradient at _check_grads' bounds."""
    from lib.layers.base import lipschitz_ops as lo
    g = _golden(golden_dir, 'sin_small_train_b2')
    arch = syn.CONFIGS['cifar10_small_sin']
    x = torch.from_numpy(g['x']).to(DEV)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV).train()
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    calls = []
    real = lo.InducedNormConv2d.forward

    def spy(self, *a, **k):
        calls.append(type(self).__name__)
        return real(self, *a, **k)
    try:
        lo.InducedNormConv2d.forward = spy
        loss, logpx, z = image_bits_per_dim_graph(m, x, arch['nvals'])
        loss.backward()
    finally:
        lo.InducedNormConv2d.forward = real
    torch.cuda.synchronize()
    blocks = imblocks(m)
    for i, b in enumerate(blocks):
        assert b._engine_grads(torch.empty(1, 1, 1, 1)) is True
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'block %d forward nstep' % i
        assert b.last_broyden_backward['nstep'] == int(g['b%d_bwd_nstep' % i]), 'block %d bwd nstep' % i
    print('loss %.8f ref %.8f' % (loss.item(), float(g['loss'])))
    assert abs(loss.item() - float(g['loss'])) <= 1e-5, (loss.item(), float(g['loss']))
    assert not calls, 'a net module ran its torch forward in the training step: %s' % calls[:3]
    n = _check_grads(m, g)
    assert n == len([k for k in g.files if k.startswith('g:') or k.startswith('gs:')])


def test_still_refused():
    """Mixes of a leading activation and hidden activations of another family have no kernel: a leading Sin before
    Swish hidden layers, a leading ELU before Sin hidden layers.  HipError from inf_net_create, nothing launched."""
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    mixes = [torch.nn.Sequential(Sin(), _conv(3, 8, 3), Swish(), _conv(8, 3, 3)),
             torch.nn.Sequential(torch.nn.ELU(), _conv(3, 8, 3), Sin(), _conv(8, 3, 3))]
    for seq in mixes:
        seq = seq.to(DEV)
        with torch.no_grad():
            seq(x)                                                        # lazy u / v
        torch.cuda.synchronize()
        _hip.profile_begin(100)
        try:
            with pytest.raises(_hip.HipError):
                _hip.NativeNet(_hip.net_entries(seq), x.shape[1:], x.device)
            with pytest.raises(_hip.HipError):
                _hip.native_net(seq, x.shape[1:], x.device)
        finally:
            stats = _hip.profile_end()
        assert not stats, stats
