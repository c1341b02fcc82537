#!/usr/bin/env python3
"""The (tag, launches) table of inf_profile_begin / inf_profile_end around one call of each engine entry point, with
the sums of the outputs beside it: the "same launches" record of a refactor.  Run it once with the
parent's library and once with the new one (INFLOW_LIB=path selects the library); the two outputs must be
byte-identical.

Nets: the three of tests/test_gpu_options.py (a fused 3-1-3 conv net on (3, 5, 12), the TOY fc net at d = 2, an fc net
at d = 33) and a generic conv net on (3, 40, 40) (5 chunks of 1024 per sample); B = 3 and 5; fixed seeds.

Then the fused fc family, every row with a hash of each returned tensor's bytes beside its sum: the
POWER shape (d = 6, three 128-wide hidden layers) and TOY (d = 2, one) with Sin and Swish, d = 6 with ELU and Softplus,
d = 8 and d = 5 with Sin; B = 3 and 50 (two FWD / block workgroups of 48, the second ragged; four JAC workgroups of
16); the same fc call list in exact fp32 and f16x3, and in f16x3 inf_imblock_eval_exact and a two-block
inf_flow_eval_exact_chain under INF_OPT_FC_BLOCK 0 / 2 and both convergence rules, inf_logdet_series and
inf_logdet_series_pair with INF_OPT_FC_SERIES off and on.

    python tools/launch_tables.py > launch_tables.txt
"""
import ctypes
import hashlib
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


def fc_seq(d, nh=1, act='sin'):
    lin = lambda a, b: get_linear(a, b, coeff=0.99, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    A = lambda: ACT_FNS[act](False)
    mods = [lin(d, 128)]
    for _ in range(nh):
        mods += [A(), lin(128, 128)]
    return torch.nn.Sequential(*mods, A(), lin(128, d))


NETS = [('conv', (3, 5, 12), lambda s: conv_seq(s, 256, True)), ('toy', (2,), lambda s: fc_seq(2)),
        ('wide', (33,), lambda s: fc_seq(33)), ('conv5', (3, 40, 40), lambda s: conv_seq(s, 16, False))]
FUSED_FC = [('power_sin', 6, 3, 'sin'), ('power_swish', 6, 3, 'swish'), ('toy_sin', 2, 1, 'sin'),
            ('toy_swish', 2, 1, 'swish'), ('d6_elu', 6, 3, 'elu'), ('d6_softplus', 6, 3, 'softplus'),
            ('d8_sin', 8, 3, 'sin'), ('d5_sin', 5, 3, 'sin')]
MFMA_F32, MFMA_F16X3 = 0, 2


def build(shape, make, seed):
    torch.manual_seed(seed)
    seq = make(shape).to(DEV)
    with torch.no_grad():
        seq(torch.zeros(1, *shape, device=DEV))                 # lazy u / v
    return seq, _hip.NativeNet(_hip.net_entries(seq), shape, torch.device(DEV))


def lib_hip_error():
    return _hip.load().inf_last_hip_error() != 0


def digest(t):
    return hashlib.sha1(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:12]


def report(name, fn, hashes=False):
    """One profiled call: its status, its launch table and the fp64 sums of what it returned (hashes: and a hash of
    each returned tensor's bytes)."""
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
    one = lambda o: repr(float(o.double().sum())) + ('#' + digest(o) if hashes else '')
    sums = ' '.join(one(o) if torch.is_tensor(o) else repr(o) for o in outs)
    print('%s: rc %d launches %s | %s' % (name, rc, ' '.join('%d:%d' % t for t in table), sums))


def main():
    lib = _hip.load()
    P = _hip.ptr
    fused_nets = [(n, (d,), lambda s, d=d, nh=nh, act=act: fc_seq(d, nh, act)) for n, d, nh, act in FUSED_FC]
    for name, shape, make in NETS + fused_nets:
        (sx, nx), (sz, nz) = build(shape, make, 3), build(shape, make, 4)
        fc = len(shape) == 1
        fused = (name, shape, make) in fused_nets
        for B in ((3, 50) if fused else (3, 5)):
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
            if not fused:
                for cname, fn in calls:
                    report(tagp + cname, fn)
                continue

            def with_options(opts, fn):
                """fn under (option, value) pairs set on both nets, the options restored afterwards"""
                def run():
                    prev = [(n, o, n.set_option(o, v)) for n in (nx, nz) for o, v in opts]
                    try:
                        return fn()
                    finally:
                        for n, o, v in prev:
                            n.set_option(o, v)
                return run

            def eval_exact_rule(per_sample):
                def run():
                    out, lx, lz, st = new(), vec(), vec(), _hip.BroydenStats()
                    if per_sample:
                        st.want_samples(B)
                    rc = lib.inf_imblock_eval_exact(nx.handle, nz.handle, P(x), P(out), P(lx), P(lz), B, T, 1e-6,
                                                    ctypes.byref(st), *W)
                    steps = tuple(st._samples[0]) if per_sample else st.nstep
                    return rc if rc else (out, lx, lz, steps, st.lowest_step)
                return run

            def chain(per_sample):
                """two blocks, (nx, nz) then (nz, nx), in one engine call"""
                def run():
                    bx = (ctypes.c_void_p * 2)(nx.handle.value, nz.handle.value)
                    bz = (ctypes.c_void_p * 2)(nz.handle.value, nx.handle.value)
                    Ts, es = (ctypes.c_int * 2)(T, T), (ctypes.c_double * 2)(1e-6, 1e-6)
                    st = (_hip.BroydenStats * 2)()
                    if per_sample:
                        for s_ in st:
                            s_.want_samples(B)
                    need = lib.inf_flow_chain_workspace_bytes(bz, 2, B, Ts)
                    cws = torch.empty(max(need, 1 << 24), dtype=torch.uint8, device=DEV)
                    out, lp_in, lp_out = new(), torch.zeros(B, device=DEV), vec()
                    rc = lib.inf_flow_eval_exact_chain(bx, bz, 2, P(x), P(out), P(lp_in), P(lp_out), B, Ts, es, st,
                                                       P(cws), cws.numel(), stream)
                    return rc if rc else (out, lp_out, st[0].nstep, st[1].nstep)
                return run

            def series_pair():
                oa, ob = vec(), vec()
                carr = COEFF.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
                rc = lib.inf_logdet_series_pair(nx.handle, P(x), P(eps), nz.handle, P(z0), P(eps), carr, len(COEFF),
                                                P(oa), P(ob), B, *W)
                return rc if rc else (oa, ob)

            if name == 'd6_softplus':                           # (netgrad takes nn.Softplus's float beta for Swish's)
                calls = [c for c in calls if c[0] != 'net_param_grad' and not c[0].startswith('logdet_grad')]
            for mode, mname in ((MFMA_F32, 'f32'), (MFMA_F16X3, 'f16x3')):
                for n in (nx, nz):
                    _hip.check(lib.inf_net_set_mfma(n.handle, mode), 'set_mfma')
                for cname, fn in calls:
                    report(tagp + mname + ' ' + cname, fn, hashes=True)
            for fcb in (0, 2):                                  # (the nets stay f16x3)
                for ps in (0, 1):
                    opts = [(_hip.INF_OPT_FC_BLOCK, fcb), (_hip.INF_OPT_CONVERGENCE, ps)]
                    label = '%sfc_block %d %s ' % (tagp, fcb, 'per_sample' if ps else 'global')
                    report(label + 'imblock_eval_exact', with_options(opts, eval_exact_rule(ps)), hashes=True)
                    report(label + 'flow_eval_exact_chain', with_options(opts, chain(ps)), hashes=True)
            for ser in (0, 1):
                opts = [(_hip.INF_OPT_FC_SERIES, ser)]
                label = '%sfc_series %d ' % (tagp, ser)
                report(label + 'logdet_series', with_options(opts, series), hashes=True)
                report(label + 'logdet_series_pair', with_options(opts, series_pair), hashes=True)


if __name__ == '__main__':
    main()
