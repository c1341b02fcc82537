#!/usr/bin/env python3
"""The (tag, launches) table of inf_profile_begin / inf_profile_end around one call of each engine entry point, with
the sums of the outputs beside it: the "same launches" record of a refactor.  Run it once with the
parent's library and once with the new one (INFLOW_LIB=path selects the library); the two outputs must be
byte-identical.

Nets: the three of tests/test_gpu_options.py (a fused 3-1-3 conv net on (3, 5, 12), the TOY fc net at d = 2, an fc net
at d = 33) and a generic conv net on (3, 40, 40) (5 chunks of 1024 per sample); B = 3 and 5; fixed seeds.

    python tools/launch_tables.py > launch_tables.txt
"""
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, 'implicit-normalizing-flows_amd'), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

from lib import _hip                                            # noqa: E402
from lib.implicit_flow import ACT_FNS                           # noqa: E402
from lib.layers import netgrad                                  # noqa: E402
from lib.layers.base import get_conv2d, get_linear              # noqa: E402

DEV = 'cuda:0'
T = 8
COEFF = np.array([1.0, -0.5, 1.0 / 3, -0.25, 0.2], dtype=np.float32)


def conv_seq(shape, hid, ks_mid):
    C = shape[0]
    conv = lambda a, b, k: get_conv2d(a, b, k, 1, k // 2, coeff=0.9, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2,
                                      codomain=2)
    A = lambda: ACT_FNS['swish'](False)
    if ks_mid:
        return torch.nn.Sequential(A(), conv(C, hid, 3), A(), conv(hid, hid, 1), A(), conv(hid, C, 3))
    return torch.nn.Sequential(conv(C, hid, 3), A(), conv(hid, C, 3))


def fc_seq(d):
    lin = lambda a, b: get_linear(a, b, coeff=0.99, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    A = lambda: ACT_FNS['sin'](False)
    return torch.nn.Sequential(lin(d, 128), A(), lin(128, 128), A(), lin(128, d))


NETS = [('conv', (3, 5, 12), lambda s: conv_seq(s, 256, True)), ('toy', (2,), lambda s: fc_seq(2)),
        ('wide', (33,), lambda s: fc_seq(33)), ('conv5', (3, 40, 40), lambda s: conv_seq(s, 16, False))]


def build(shape, make, seed):
    torch.manual_seed(seed)
    seq = make(shape).to(DEV)
    with torch.no_grad():
        seq(torch.zeros(1, *shape, device=DEV))                 # lazy u / v
    return seq, _hip.NativeNet(_hip.net_entries(seq), shape, torch.device(DEV))


def lib_hip_error():
    return _hip.load().inf_last_hip_error() != 0


def report(name, fn):
    """One profiled call: its status, its launch table and the fp64 sums of what it returned."""
    _hip.profile_begin(100000)
    outs, rc = (), 0
    try:
        r = fn()
        rc, outs = (r, ()) if isinstance(r, int) else (0, r)
        torch.cuda.synchronize()
    except _hip.HipError as e:                                  # a declined call is part of the record; a HIP error ends it
        if lib_hip_error():
            raise
        outs = (str(e),)
    finally:
        table = sorted((s['tag'], s['launches']) for s in _hip.profile_end())
    sums = ' '.join(repr(float(o.double().sum())) if torch.is_tensor(o) else repr(o) for o in outs)
    print('%s: rc %d launches %s | %s' % (name, rc, ' '.join('%d:%d' % t for t in table), sums))


def main():
    lib = _hip.load()
    P = _hip.ptr
    for name, shape, make in NETS:
        (sx, nx), (sz, nz) = build(shape, make, 3), build(shape, make, 4)
        fc = len(shape) == 1
        for B in (3, 5):
            gen = torch.Generator().manual_seed(7 + B)
            rnd = lambda: (torch.randn(B, *shape, generator=gen) * 0.5).to(DEV)
            x, v, z0 = rnd(), rnd(), rnd()
            eps = torch.where(rnd() >= 0, 1.0, -1.0).contiguous()
            stream = _hip.stream_of(x)
            for n in (nx, nz):
                n.refresh_if_needed(stream)
            ws = torch.empty(max(nx.ws_bytes(B, T), nz.ws_bytes(B, T), 1 << 24), dtype=torch.uint8, device=DEV)
            W = (P(ws), ws.numel(), stream)
            new = lambda: torch.empty_like(x)
            vec = lambda: torch.empty(B, device=DEV)
            tagp = '%s B%d ' % (name, B)

            def forward():
                y = new()
                _hip.check(lib.inf_net_forward(nx.handle, P(x), P(y), B, *W), 'forward')
                return (y,)

            def vjp():
                g = new()
                _hip.check(lib.inf_net_vjp(nx.handle, P(x), P(v), P(g), B, *W), 'vjp')
                return (g,)

            def root(per_sample=False, ls=False):
                def run():
                    nz.set_option(_hip.INF_OPT_CONVERGENCE, int(per_sample))
                    nz.set_option(_hip.INF_OPT_LINE_SEARCH, int(ls))
                    st = _hip.BroydenStats()
                    if per_sample:
                        st.want_samples(B)
                    out = new()
                    try:
                        _hip.check(lib.inf_root_find(nz.handle, nx.handle, P(x), P(out), B, T, 1e-6, ctypes.byref(st),
                                                     None, *W), 'root_find')
                    finally:
                        nz.set_option(_hip.INF_OPT_CONVERGENCE, 0)
                        nz.set_option(_hip.INF_OPT_LINE_SEARCH, 0)
                    return (out, st.nstep, st.lowest_step, st.diff)
                return run

            def banach():
                out, it = new(), ctypes.c_int()
                _hip.check(lib.inf_banach_find_root(nz.handle, nx.handle, P(x), P(out), B, 20, 1e-9, ctypes.byref(it),
                                                    *W), 'banach')
                return (out, it.value)

            def block_forward():
                out, st = new(), _hip.BroydenStats()
                _hip.check(lib.inf_imblock_forward(nx.handle, nz.handle, P(x), P(out), B, T, 1e-6, ctypes.byref(st),
                                                   *W), 'imblock_forward')
                return (out, st.nstep)

            def block_backward():
                dh, dx, st = new(), new(), _hip.BroydenStats()
                _hip.check(lib.inf_imblock_backward(nx.handle, nz.handle, P(z0), P(x), P(v), P(dh), P(dx), B, T, 1e-6,
                                                    ctypes.byref(st), *W), 'imblock_backward')
                return (dh, dx, st.nstep)

            def eval_exact():
                out, lx, lz, st = new(), vec(), vec(), _hip.BroydenStats()
                rc = lib.inf_imblock_eval_exact(nx.handle, nz.handle, P(x), P(out), P(lx), P(lz), B, T, 1e-6,
                                                ctypes.byref(st), *W)
                return rc if rc else (out, lx, lz, st.nstep)

            def series():
                out = vec()
                carr = COEFF.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
                _hip.check(lib.inf_logdet_series(nx.handle, P(x), P(eps), carr, len(COEFF), P(out), B, *W), 'series')
                return (out,)

            def exact():
                out = vec()
                rc = lib.inf_logdet_exact(nx.handle, P(x), P(out), B, *W)
                return rc if rc else (out,)

            def trace():
                out = vec()
                carr = COEFF.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
                rc = lib.inf_logdet_exact_trace(nx.handle, P(x), carr, len(COEFF), P(out), B, *W)
                return rc if rc else (out,)

            def logdet_grad(mode):
                def run():
                    r = netgrad.logdet_grads(nx, sx, x, mode, eps if mode == 0 else None,
                                             COEFF if mode != 1 else None, torch.ones(B, device=DEV))
                    return _hip.INF_ERR_UNSUPPORTED if r is None else (r[0], r[2]) + tuple(r[1].values())
                return run

            def param_grad():
                r = netgrad.param_grads(nx, sx, x, v, want_x=True)
                return _hip.INF_ERR_UNSUPPORTED if r is None else (r[1],) + tuple(r[0].values())

            calls = [('net_forward', forward), ('net_vjp', vjp), ('root_find', root()),
                     ('root_find per_sample', root(per_sample=True)), ('root_find line_search', root(ls=True)),
                     ('banach_find_root', banach), ('imblock_forward', block_forward),
                     ('imblock_backward', block_backward), ('logdet_series', series), ('net_param_grad', param_grad)]
            if fc:
                calls += [('imblock_eval_exact', eval_exact), ('logdet_exact', exact), ('logdet_exact_trace', trace)]
                calls += [('logdet_grad mode %d' % m, logdet_grad(m)) for m in (0, 1, 2)]
            for cname, fn in calls:
                report(tagp + cname, fn)


if __name__ == '__main__':
    main()
