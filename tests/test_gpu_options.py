"""How an engine net takes its options: the environment defaults read at inf_net_create (the six per-net option
variables and INFLOW_MFMA), inf_net_set_option and inf_net_get_option, on the smallest nets that reach each branch of
inf_net_create -- a fused 3-1-3 conv net, the TOY fc net (fused fc path) and one fc net just over FC_NARROW_MAX (the
per-layer chain).  Written against the library before its host code was split: every assertion here
held there unchanged.
"""
import ctypes

import pytest
import torch

from lib import _hip
from lib.implicit_flow import ACT_FNS
from lib.layers.base import get_conv2d, get_linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INVALID = 1                      # INF_ERR_INVALID (include/inflow.h)
F32, BF16X6, F16X3 = 0, 1, 2     # InfMfmaMode

# variable -> (option, accepted spellings in index order)
ENV_OPTIONS = {
    'INFLOW_FUSED_K128': (_hip.INF_OPT_FUSED_K128, ('0', '1', '2', '3')),
    'INFLOW_EVAL_OVERLAP': (_hip.INF_OPT_EVAL_OVERLAP, ('0', '1')),
    'INFLOW_CONVERGENCE': (_hip.INF_OPT_CONVERGENCE, ('global', 'per_sample')),
    'INFLOW_FC_BLOCK': (_hip.INF_OPT_FC_BLOCK, ('0', '1', '2')),
    'INFLOW_FC_SERIES': (_hip.INF_OPT_FC_SERIES, ('0', '1')),
    'INFLOW_FUSED_PRESPLIT': (_hip.INF_OPT_FUSED_PRESPLIT, ('0', '1')),
}
# option -> highest valid value
OPTION_MAX = {
    _hip.INF_OPT_FUSED_K128: 3, _hip.INF_OPT_EVAL_OVERLAP: 1, _hip.INF_OPT_CONVERGENCE: 1,
    _hip.INF_OPT_K128_EXACT_SCALE: 1, _hip.INF_OPT_FC_BLOCK: 2, _hip.INF_OPT_FC_SERIES: 1,
    _hip.INF_OPT_LINE_SEARCH: 1, _hip.INF_OPT_FUSED_PRESPLIT: 1, _hip.INF_OPT_FC_SKINNY: 1,
}


def _conv_seq():
    """Swish, conv3 3 -> 256, Swish, conv1, Swish, conv3 256 -> 3 on (3, 5, 12): the smallest fused 3-1-3 shape of
    tests/test_gpu_ragged_tiles.py."""
    C, H, W, hid = 3, 5, 12, 256
    conv = lambda a, b, k: get_conv2d(a, b, k, 1, k // 2, coeff=0.9, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2,
                                      codomain=2)
    A = lambda: ACT_FNS['swish'](False)
    return torch.nn.Sequential(A(), conv(C, hid, 3), A(), conv(hid, hid, 1), A(), conv(hid, C, 3)), (C, H, W)


def _fc_seq(d):
    """d -> 128 -> 128 -> d with Sin (synthetic.TOY's nets at d = 2)."""
    lin = lambda a, b: get_linear(a, b, coeff=0.99, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    A = lambda: ACT_FNS['sin'](False)
    return torch.nn.Sequential(lin(d, 128), A(), lin(128, 128), A(), lin(128, d)), (d,)


@pytest.fixture(scope='module')
def nets():
    """name -> (module with u / v initialised, per-sample shape, a batch of 3)."""
    out = {}
    for name, (seq, shape) in (('conv', _conv_seq()), ('toy', _fc_seq(2)), ('wide', _fc_seq(33))):
        torch.manual_seed(3)
        seq = seq.to(DEV)
        gen = torch.Generator().manual_seed(7)
        x = (torch.randn(3, *shape, generator=gen) * 0.5).to(DEV)
        with torch.no_grad():
            seq(torch.zeros(1, *shape, device=DEV))             # lazy u / v
        out[name] = (seq, shape, x)
    return out


def _create(seq, shape):
    return _hip.NativeNet(_hip.net_entries(seq), shape, torch.device(DEV))


def _forward(net, x):
    B = x.shape[0]
    stream = _hip.stream_of(x)
    net.refresh_if_needed(stream)
    ws = torch.empty(net.ws_bytes(B), dtype=torch.uint8, device=DEV)
    y = torch.empty_like(x)
    _hip.check(net.lib.inf_net_forward(net.handle, _hip.ptr(x), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream), 'fwd')
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('var', sorted(ENV_OPTIONS))
def test_option_variable_sets_the_default(var, nets, monkeypatch):
    """Every accepted spelling gives its index on a net created under it; a rejected one fails inf_net_create with
    INF_ERR_INVALID; the next creation without the variable succeeds, and its forward has the bits of a net created
    before the failed attempt."""
    option, spellings = ENV_OPTIONS[var]
    for name, (seq, shape, x) in nets.items():
        monkeypatch.delenv(var, raising=False)
        before = _forward(_create(seq, shape), x)
        for index, text in enumerate(spellings):
            monkeypatch.setenv(var, text)
            assert _create(seq, shape).get_option(option) == index, (name, var, text)
        for bad in ('7', ' 1'):
            monkeypatch.setenv(var, bad)
            with pytest.raises(_hip.HipError, match=r'inf_net_create failed: invalid argument \(status %d' % INVALID):
                _create(seq, shape)
        monkeypatch.delenv(var)
        after = _create(seq, shape)
        assert torch.equal(_forward(after, x), before), (name, var)


def test_mfma_variable(nets, monkeypatch):
    """INFLOW_MFMA on the fused conv net and on the fused fc net (which has no bf16x6 kernel: fp32); unset and empty:
    f16x3.  A rejected spelling fails inf_net_create on both."""
    modes = {'f32': (F32, F32), 'fp32': (F32, F32), 'bf16x6': (BF16X6, F32), 'f16x3': (F16X3, F16X3), '': (F16X3, F16X3),
             None: (F16X3, F16X3)}
    for text, want in modes.items():
        if text is None:
            monkeypatch.delenv('INFLOW_MFMA', raising=False)
        else:
            monkeypatch.setenv('INFLOW_MFMA', text)
        for name, mode in zip(('conv', 'toy'), want):
            net = _create(*nets[name][:2])
            assert net.lib.inf_net_get_mfma(net.handle) == mode, (text, name)
    monkeypatch.setenv('INFLOW_MFMA', 'f16')
    for name in ('conv', 'toy'):
        with pytest.raises(_hip.HipError, match=r'inf_net_create failed: invalid argument \(status %d' % INVALID):
            _create(*nets[name][:2])
    monkeypatch.delenv('INFLOW_MFMA')
    for name in ('conv', 'toy'):
        net = _create(*nets[name][:2])
        assert net.lib.inf_net_get_mfma(net.handle) == F16X3


def test_set_and_get_option(nets, monkeypatch):
    """All nine options: inf_net_set_option returns the previous value; -1 and one past the maximum return
    -INF_ERR_INVALID and leave the value; an unknown option id returns -INF_ERR_INVALID from both calls."""
    for var in ENV_OPTIONS:
        monkeypatch.delenv(var, raising=False)
    assert sorted(OPTION_MAX) == list(range(1, 10))
    for name, (seq, shape, _) in nets.items():
        net = _create(seq, shape)
        lib, h = net.lib, net.handle
        for option, hi in OPTION_MAX.items():
            prev = lib.inf_net_get_option(h, option)
            assert 0 <= prev <= hi
            for value in list(range(hi + 1)) + [0, hi]:
                assert lib.inf_net_set_option(h, option, value) == prev, (name, option, value)
                assert lib.inf_net_get_option(h, option) == value
                prev = value
            for bad in (-1, hi + 1):
                assert lib.inf_net_set_option(h, option, bad) == -INVALID, (name, option, bad)
                assert lib.inf_net_get_option(h, option) == prev
        for unknown in (0, 10, -3):
            assert lib.inf_net_get_option(h, unknown) == -INVALID
            assert lib.inf_net_set_option(h, unknown, 0) == -INVALID
        assert lib.inf_net_set_option(ctypes.c_void_p(0), _hip.INF_OPT_FC_SKINNY, 0) == -INVALID
