"""The residual builders of the output stage (out_stage.hip) and the solver's first step (broyden.hip), one case per
dispatch regime, against an independent computation in torch: the engine only supplies the net evaluations
(inf_net_forward), the residual arithmetic is restated here in fp32 and its norm in fp64.

  * first residual and first step of inf_root_find (global rule, eps 1e-12, two steps): with x_emb = e(x) + x and
    f0 = f(0), g0 = (x_emb - f0) - 0 in fp32 and trace[0] = ||g0|| in fp64; then x1 = -g0 (update = -g0, x1 = 0 + update,
    broyden.py:144,94), g1 = (x_emb - f(x1)) - x1 and trace[1] = ||g1||.  Conv nets at 1, 2, 4 chunks of OUT_CH = 1024
    elements per sample (the per-sample totals of broyden_start_sample_kernel and conv_out_resid_sample_kernel) and at 5
    chunks (resid_bcast_kernel / conv_out_kernel with chunk partials and reduce_partials_kernel); fc nets at d = 6
    (broyden_start_fc_kernel and the fused fc net's epilogue), d = 32 (last narrow width) and d = 33 (fc_out_wide_kernel,
    the first residual with the broadcast f(0)).
  * the implicit backward's first residual (inf_imblock_backward): the solve starts at y = 0, so g = (0 + 0) - grad and
    trace[0] = ||grad||: the three layouts of launch_vjp_resid (conv chunks, fc narrow, fc wide).
  * the per-sample rule on a batch of one returns z and nstep bit for bit as the global rule does (conv 2 chunks, fc
    d = 6).

Tolerance of the norms: relative 2 n 2^-53 with n = B d.  The engine and torch both sum the n exact fp64 squares of the
same fp32 values, in different fixed orders; n additions of positive terms are each off by at most 2^-53 relative, and
the two orders' errors add.  (The square root halves a relative error.)"""
import ctypes

import pytest
import torch

from lib import _hip
from lib.implicit_flow import ACT_FNS
from lib.layers.base import get_conv2d, get_linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 3
CH = 1024                        # out_stage.hip OUT_CH


def _conv_seq(hw, hid=16):
    """conv3 3 -> 16, Swish, conv3 16 -> 3 on (3, hw, hw): the generic GEMM chain and the 9-tap output stage."""
    conv = lambda a, b: get_conv2d(a, b, 3, 1, 1, coeff=0.9, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2,
                                   codomain=2)
    return torch.nn.Sequential(conv(3, hid), ACT_FNS['swish'](False), conv(hid, 3)), (3, hw, hw)


def _fc_seq(d):
    """d -> 128 -> 128 -> d with Sin (tests/test_gpu_options.py's fc nets)."""
    lin = lambda a, b: get_linear(a, b, coeff=0.99, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    A = lambda: ACT_FNS['sin'](False)
    return torch.nn.Sequential(lin(d, 128), A(), lin(128, 128), A(), lin(128, d)), (d,)


SHAPES = {'conv8': lambda: _conv_seq(8), 'conv20': lambda: _conv_seq(20), 'conv36': lambda: _conv_seq(36),
          'conv40': lambda: _conv_seq(40), 'fc6': lambda: _fc_seq(6), 'fc32': lambda: _fc_seq(32),
          'fc33': lambda: _fc_seq(33)}
_cache = {}


def _nets(name):
    """(engine net f, engine net e, per-sample shape, a batch of B inputs) of a shape, built once."""
    if name not in _cache:
        mods = []
        for seed in (3, 4):
            torch.manual_seed(seed)
            seq, shape = SHAPES[name]()
            seq = seq.to(DEV)
            with torch.no_grad():
                seq(torch.zeros(1, *shape, device=DEV))         # lazy u / v
            mods.append(seq)
        gen = torch.Generator().manual_seed(7)
        x = (torch.randn(B, *shape, generator=gen) * 0.5).to(DEV)
        nets = [_hip.NativeNet(_hip.net_entries(m), shape, torch.device(DEV)) for m in mods]
        _cache[name] = (nets[0], nets[1], shape, x, mods)
    return _cache[name][:4]


def _forward(net, x):
    n = x.shape[0]
    stream = _hip.stream_of(x)
    net.refresh_if_needed(stream)
    ws = torch.empty(net.ws_bytes(n), dtype=torch.uint8, device=DEV)
    y = torch.empty_like(x)
    _hip.check(net.lib.inf_net_forward(net.handle, _hip.ptr(x), _hip.ptr(y), n, _hip.ptr(ws), ws.numel(), stream), 'fwd')
    torch.cuda.synchronize()
    return y


def _root_find(nf, ne, x, T, eps, per_sample=False):
    n = x.shape[0]
    stream = _hip.stream_of(x)
    for net in (nf, ne):
        net.refresh_if_needed(stream)
    prev = nf.set_option(_hip.INF_OPT_CONVERGENCE, _hip.INF_CONV_PER_SAMPLE if per_sample else _hip.INF_CONV_GLOBAL)
    try:
        ws = torch.empty(max(nf.ws_bytes(n, T), ne.ws_bytes(n, T)), dtype=torch.uint8, device=DEV)
        ws.fill_(255)
        st = _hip.BroydenStats()
        if per_sample:
            st.want_samples(n)
        out = torch.empty_like(x)
        _hip.check(nf.lib.inf_root_find(nf.handle, ne.handle, _hip.ptr(x), _hip.ptr(out), n, T, eps, ctypes.byref(st),
                                        None, _hip.ptr(ws), ws.numel(), stream), 'inf_root_find')
        torch.cuda.synchronize()
    finally:
        nf.set_option(_hip.INF_OPT_CONVERGENCE, prev)
    return out, st.as_dict(T)


def _norm64(g):
    return float(g.double().cpu().pow(2).sum().sqrt())


def _check_norm(what, got, g):
    ref = _norm64(g)
    bound = 2.0 * g.numel() * 2.0 ** -53
    rel = abs(got - ref) / ref
    print('%s: engine %.17g torch %.17g rel %.3g (bound %.3g)' % (what, got, ref, rel, bound))
    assert ref > 0 and rel <= bound, (what, got, ref, rel, bound)


@pytest.mark.parametrize('name', ['conv8', 'conv20', 'conv36', 'conv40', 'fc6', 'fc32', 'fc33'])
def test_first_residual_and_first_step_of_root_find(name):
    nf, ne, shape, x = _nets(name)
    d = int(torch.tensor(shape).prod())
    assert {'conv8': 1, 'conv20': 2, 'conv36': 4, 'conv40': 5}.get(name, (d + CH - 1) // CH) == (d + CH - 1) // CH
    xemb = _forward(ne, x) + x
    f0 = _forward(nf, torch.zeros_like(x))[0]          # the engine caches sample 0 of a batch-sized evaluation at 0
    g0 = (xemb - f0) - torch.zeros_like(x)
    _, st = _root_find(nf, ne, x, 2, 1e-12)
    assert st['convergence'] == 'global' and len(st['trace']) >= 2, st
    _check_norm(name + ' trace[0]', st['trace'][0], g0)
    x1 = -g0
    g1 = (xemb - _forward(nf, x1)) - x1
    _check_norm(name + ' trace[1]', st['trace'][1], g1)


@pytest.mark.parametrize('name', ['conv20', 'fc6', 'fc33'])
def test_first_residual_of_implicit_backward(name):
    nz, nx, shape, x = _nets(name)
    gen = torch.Generator().manual_seed(11)
    z = (torch.randn(B, *shape, generator=gen) * 0.5).to(DEV)
    grad = torch.randn(B, *shape, generator=gen).to(DEV)
    stream = _hip.stream_of(x)
    for net in (nz, nx):
        net.refresh_if_needed(stream)
    T = 2
    ws = torch.empty(max(nz.ws_bytes(B, T), nx.ws_bytes(B, 1)), dtype=torch.uint8, device=DEV)
    ws.fill_(255)
    st = _hip.BroydenStats()
    dl_dh, dl_dx = torch.empty_like(grad), torch.empty_like(grad)
    _hip.check(nz.lib.inf_imblock_backward(nx.handle, nz.handle, _hip.ptr(z), _hip.ptr(x), _hip.ptr(grad),
                                           _hip.ptr(dl_dh), _hip.ptr(dl_dx), B, T, 1e-12, ctypes.byref(st),
                                           _hip.ptr(ws), ws.numel(), stream), 'inf_imblock_backward')
    torch.cuda.synchronize()
    st = st.as_dict(T)
    assert len(st['trace']) >= 1, st
    _check_norm(name + ' backward trace[0]', st['trace'][0], grad)
    assert torch.isfinite(dl_dh).all() and torch.isfinite(dl_dx).all()


@pytest.mark.parametrize('name', ['conv20', 'fc6'])
def test_per_sample_rule_on_a_batch_of_one_is_the_global_rule(name):
    nf, ne, shape, x = _nets(name)
    for b in range(B):
        zg, sg = _root_find(nf, ne, x[b:b + 1].contiguous(), 30, 1e-5)
        zp, sp = _root_find(nf, ne, x[b:b + 1].contiguous(), 30, 1e-5, per_sample=True)
        print('%s sample %d: nstep global %d per-sample %s' % (name, b, sg['nstep'], sp['sample_nstep']))
        assert sp['convergence'] == 'per_sample' and sg['convergence'] == 'global'
        assert sg['nstep'] >= 2 and not sg['prot_break']
        assert sp['sample_nstep'] == [sg['nstep']] and sp['nstep'] == sg['nstep']
        assert sp['sample_lowest_step'] == [sg['lowest_step']]
        assert torch.equal(zp, zg)
