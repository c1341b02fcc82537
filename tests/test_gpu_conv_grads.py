"""Conv-net parameter gradients on the engine (inf_net_param_grad / inf_net_surrogate_grad, conv layout) in every regime
`launch_wgrad` (csrc/grad.hip) dispatches on, against torch autograd in fp64 on the CPU of the same nets.

The nets are the project's own modules: [Swish], conv3(C -> hid), act, conv1(hid -> hid), act, conv3(hid -> C).  The
fp64 reference evaluates them on fp64 leaf copies of the parameters with W / max(1, sigma / coeff) inside the graph
(sigma = sum u . conv2d(v, W) on the layer's (H, W) for a k x k layer, u . (W v) for a 1x1 layer), like
`_eval64` / `_params64` of test_gpu_fcgrad.py.  Compared: every dW, db, dbeta, dpre_beta and gx of
`netgrad.param_grads(..., want_x=True)`, and the value, gx and parameter gradients of `netgrad.surrogate_grads`
(reference: autograd.grad(net(x), x, w, create_graph=True) dotted with eps, then differentiated).

Tolerance, per tensor and computed at run time: e32 = the error of fp32 torch autograd through the same modules on the
CPU against the fp64 reference (largest absolute difference over the largest reference element, the measure of
test_gpu_train.py::_check_param).  The engine must be within max(8 e32, 1e-6) of the scale, never more than the 2e-4 of
the existing test.  The factor 8 is a margin for summation order (the wgrad kernels add the K = B H W / nsplit products
of a split one after another in fp32, torch's CPU kernels add in blocks; K is a few hundred per split here).  Each
case prints the engine's error, e32 and their ratio per tensor.  Measured on an MI355X: at most 2.7 on a weight
gradient, at most 4.9 where the engine's error is above the 1e-6 floor (a scalar dbeta), 20 under the floor (DESIGN.md
section 8).

Each case also asserts which weight-gradient kernels ran (launch-profile tags, lib/_hip WGRAD_TAGS and 8<TMW><TNW>),
that every output buffer is overwritten (NaN-filled before the call), that a 0xFF-filled workspace and NaN-poisoned LDS
do not reach the results, and that nothing is written past `inf_grad_workspace_bytes` (a 4 KiB guard behind it stays
0xFF).  Case (a) has B = 9: its dW is compared with the fp64 gradient of the sum over the samples, so the result does
not depend on the batch size through the row / chunk split (36 rows over 32 splits, 9 chunks over 2).

The table of the cases is CASES; `tags` is what `launch_wgrad` chooses for the layers' data and dsigma/dW calls (a 1x1
layer's dsigma/dW has P = 1 and always takes the plain kernel, 890).

The GPU tests carry the `gpu` mark one by one; `test_reference_tells_faulty_contractions_apart` needs no GPU.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lib import _hip
from lib.layers import netgrad
from lib.layers.base import InducedNormConv2d, Sin, Swish

DEV = 'cuda:0'
REL_CAP = 2e-4          # test_gpu_train.py::_check_param's bound: never exceeded here
REL_FLOOR = 1e-6
FACTOR = 8.0
GUARD_BYTES = 4096

PLAIN, VALU, VALU3, V3R8, V3R16, V3R32 = 890, 895, 896, 897, 898, 899      # lib/_hip WGRAD_TAGS
T11, T12, T21, T22 = 811, 812, 821, 822

# name: C, hid, H, W, B, leading Swish, activation, weight scales, inputs one float off 16-byte alignment, wgrad tags.
# M = cout, N = cin k^2, P = H W; VALU family: M <= 16 and W % 8 == 0 (3x3 form: X 16-byte aligned; row-resident at
# W in {8, 16, 32}); tiled: P % 32 == 0, 128-wide along M / N >= 128; plain otherwise.
CASES = {
    # tiled<1,1> with ragged M = 40, N = 27 / 40, 9 chunks over 2 splits (4 + 5); valu3r<8>, H != W, 36 rows over 32
    # splits (uneven).  (B = 9, not 3: at 12 rows the VALU split is one row each and the tiled kernel has one split.)
    'a': dict(C=3, hid=40, H=4, W=8, B=9, pre=False, tags={T11, PLAIN, V3R8}),
    # tiled<1,2> (M = 72, N = 144, both ragged); valu3r<8> at M = 16; B = 1; dpre_beta
    'b': dict(C=16, hid=72, H=8, W=8, B=1, pre=True, tags={T12, T11, PLAIN, V3R8}),
    # tiled<2,1> (M = 136, N = 27), tiled<2,2> with ragged M = N = 136; nchunks = 2: one split
    'c': dict(C=3, hid=136, H=4, W=8, B=2, pre=False, tags={T21, T22, PLAIN, V3R8}),
    # the VALU family throughout: valu3r<16> at M = 16 and M = 1, valu (1x1, M = 16)
    'd': dict(C=1, hid=16, H=16, W=16, B=2, pre=True, tags={V3R16, VALU, PLAIN}),
    # x, gout, w, eps 4 bytes past 16-byte alignment: layer 0's X -> valu with k = 3; the last layer's G -> off the VALU
    # family (tiled<1,2>, N = 144); the GEMM loaders' non-vector path.  u, v stay aligned: dsigma/dW on valu3r<8>
    'e': dict(C=3, hid=16, H=8, W=8, B=2, pre=False, misaligned=True, tags={VALU, T12, PLAIN, V3R8}),
    # valu3 at W = 24: three 8-pixel chunks, both halo loads, both image edges
    'f': dict(C=3, hid=24, H=4, W=24, B=2, pre=True, tags={T11, PLAIN, VALU3}),
    # valu3 at CelebA-HQ 256's width; B = 1, two rows
    'g': dict(C=2, hid=20, H=2, W=64, B=1, pre=False, tags={T11, PLAIN, VALU3}),
    # plain kernel, P = 16, K = 640: two splits, every 32-pixel chunk holds two images
    'h': dict(C=3, hid=48, H=4, W=4, B=40, pre=False, tags={PLAIN}),
    # plain kernel, W % 8 != 0, K = 576: two splits, chunks straddle images (P = 144 = 4.5 chunks)
    'i': dict(C=5, hid=24, H=12, W=12, B=4, pre=True, tags={PLAIN}),
    # the last layer tiled (M = 20 > 16, N = 360), its dsigma/dW call with B = 1
    'j': dict(C=20, hid=40, H=4, W=8, B=2, pre=False, tags={T12, T11, PLAIN}),
    # plain kernel, P = 30 (P % 4 != 0: the GEMMs' non-vector path, their 32-row and 128-row configs with ragged N)
    'k': dict(C=3, hid=40, H=5, W=6, B=3, pre=False, tags={PLAIN}),
    # Sin in place of Swish in the conv layout, first and second order
    'l_a': dict(C=3, hid=40, H=4, W=8, B=9, pre=False, act='sin', tags={T11, PLAIN, V3R8}),
    'l_f': dict(C=3, hid=24, H=4, W=24, B=2, pre=False, act='sin', tags={T11, PLAIN, VALU3}),
    # both branches of sigma_chain_kernel in one net: sigma / coeff < 1 in the middle layer, > 1 in the other two
    'm': dict(C=3, hid=40, H=4, W=8, B=9, pre=False, scales=(3.0, 0.3, 3.0), tags={T11, PLAIN, V3R8}),
    # valu3r<32> (not in the issue's table; no other case has W = 32) with H != W and 6 rows; valu at M = 12
    'n': dict(C=2, hid=12, H=3, W=32, B=2, pre=True, tags={V3R32, VALU, PLAIN}),
}
COEFF = 0.9


def _case(name):
    c = dict(act='swish', scales=(3.0, 3.0, 3.0), misaligned=False)
    c.update(CASES[name])
    return c


def _seed(name):
    return 100 + sorted(CASES).index(name)


def _layers(net):
    return [m for m in net if isinstance(m, InducedNormConv2d)]


@functools.lru_cache(maxsize=None)
def _build(name):
    """The case's net (CPU, u / v / sigma consistent after the scaling) and its inputs x, gout, w, eps."""
    c = _case(name)
    torch.manual_seed(_seed(name))
    conv = lambda a, b, k: InducedNormConv2d(a, b, k, 1, k // 2, coeff=COEFF, atol=1e-3, rtol=1e-3)
    act = Swish if c['act'] == 'swish' else Sin
    C, hid = c['C'], c['hid']
    net = torch.nn.Sequential(*(([Swish()] if c['pre'] else []) +
                                [conv(C, hid, 3), act(), conv(hid, hid, 1), act(), conv(hid, C, 3)]))
    g = torch.Generator().manual_seed(_seed(name))
    with torch.no_grad():
        net(torch.zeros(1, C, c['H'], c['W']))                 # spatial dims, u / v
        nb = 0
        for m in net:
            if hasattr(m, 'beta'):
                m.beta.fill_(0.4 + 0.15 * nb)                  # not the initial value, and one per activation
                nb += 1
        for m, s in zip(_layers(net), c['scales']):
            m.weight.mul_(s)
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
        for m in _layers(net):
            m.compute_weight(update=True)                      # power iteration on the scaled weights
    shape = (c['B'], C, c['H'], c['W'])
    x = torch.randn(shape, generator=g) * 0.7
    gout = torch.randn(shape, generator=g)
    w = torch.randn(shape, generator=g)
    eps = torch.randn(shape, generator=g).sign()
    return net, (x, gout, w, eps)


def _params(net):
    return [getattr(m, n) for m in net for n in ('weight', 'bias', 'beta') if hasattr(m, n)]


def _param_names(net):
    """The InfNetGrads slot of every entry of _params(net): dW[l], db[l], dbeta[l] (the activation after layer l),
    dpre_beta."""
    names, l = [], -1
    for m in net:
        if isinstance(m, InducedNormConv2d):
            l += 1
            names += ['dW[%d]' % l, 'db[%d]' % l]
        elif hasattr(m, 'beta'):
            names.append('dbeta[%d]' % l if l >= 0 else 'dpre_beta')
    return names


def _eval64(net, x, leaf, rec=None):
    """The net in fp64 on the leaf copies, compute_weight(update=False) semantics with the normalisation in the graph.
    rec (a dict) receives every layer's effective weight, input, pre-activation, sigma / coeff."""
    h = x
    for m in net:
        if isinstance(m, InducedNormConv2d):
            W = leaf[id(m.weight)]
            k = m.kernel_size[0]
            if k > 1:
                H, Wd = x.shape[2:]
                v = m.v.double().view(1, m.in_channels, H, Wd)
                sigma = (m.u.double().view(1, m.out_channels, H, Wd) * F.conv2d(v, W, padding=k // 2)).sum()
            else:
                sigma = torch.dot(m.u.double(), torch.mv(W.view(m.out_channels, m.in_channels), m.v.double()))
            We = W / torch.max(torch.ones(1, dtype=torch.float64), sigma / m.coeff)
            if rec is not None:
                rec.setdefault('Weff', []).append(We)
                rec.setdefault('in', []).append(h)
                rec.setdefault('ratio', []).append(float(sigma.detach()) / m.coeff)
            h = F.conv2d(h, We, leaf[id(m.bias)], padding=k // 2)
            if rec is not None:
                rec.setdefault('h', []).append(h)
        elif isinstance(m, Sin):
            h = torch.sin(2 * np.pi * h) / (2 * np.pi)
        else:
            h = h * torch.sigmoid(h * F.softplus(leaf[id(m.beta)])) / 1.1
    return h


def _grads(outs, wrt):
    gs = torch.autograd.grad(outs, wrt, allow_unused=True)
    return [torch.zeros_like(t) if g is None else g.detach() for g, t in zip(gs, wrt)]


@functools.lru_cache(maxsize=None)
def _reference(name):
    """fp64 autograd (the reference) and fp32 autograd through the modules on the CPU (the tolerance's yardstick), once
    per case: {'first' / 'second': {key: (ref64, cpu32)}}, keys the parameters' indices, 'x', 'value'; plus the fp64
    pieces the sigma-chain check and the CPU guard use."""
    net, (x, gout, w, eps) = _build(name)
    params = _params(net)
    B = x.shape[0]
    out = {}
    # fp64
    leaves = [p.detach().double().requires_grad_(True) for p in params]
    leaf = {id(p): t for p, t in zip(params, leaves)}
    x64 = x.double().requires_grad_(True)
    rec = {}
    y = _eval64(net, x64, leaf, rec)
    first64 = _grads((y * gout.double()).sum(), leaves + [x64] + rec['Weff'] + rec['h'])
    n = len(leaves)
    out['dWeff'] = first64[n + 1:n + 1 + len(rec['Weff'])]
    out['G'] = first64[n + 1 + len(rec['Weff']):]
    out['in'] = [t.detach() for t in rec['in']]
    out['ratio'] = rec['ratio']
    out['h'] = [t.detach() for t in rec['h']]
    x64 = x.double().requires_grad_(True)
    y = _eval64(net, x64, leaf)
    vjp = torch.autograd.grad(y, x64, w.double(), create_graph=True)[0]
    s64 = (vjp.view(B, -1) * eps.double().view(B, -1)).sum(1)
    second64 = _grads(s64.sum(), leaves + [x64])
    # fp32 through the modules, on one thread: torch's blocked sums then do not depend on the machine's core count
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        x32 = x.clone().requires_grad_(True)
        first32 = _grads((net(x32) * gout).sum(), params + [x32])
        x32 = x.clone().requires_grad_(True)
        vjp = torch.autograd.grad(net(x32), x32, w, create_graph=True)[0]
        s32 = (vjp.view(B, -1) * eps.view(B, -1)).sum(1)
        second32 = _grads(s32.sum(), params + [x32])
    finally:
        torch.set_num_threads(threads)
    keys = list(range(n)) + ['x']
    out['first'] = {k: (a, b) for k, a, b in zip(keys, first64[:n + 1], first32)}
    out['second'] = {k: (a, b) for k, a, b in zip(keys, second64, second32)}
    out['second']['value'] = (s64.detach(), s32.detach())
    return out


def _bound(ref64, cpu32):
    """(relative bound, e32, scale) of one tensor: max(8 e32, 1e-6), capped at 2e-4."""
    scale = max(ref64.abs().max().item(), 1e-12)
    e32 = (cpu32.double() - ref64).abs().max().item() / scale
    return min(REL_CAP, max(FACTOR * e32, REL_FLOOR)), e32, scale


class _Report:
    def __init__(self, name):
        self.name, self.bad, self.worst = name, [], 0.0

    def check(self, what, got, ref64, cpu32):
        got = got.detach().double().cpu()
        assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
        assert torch.isfinite(got).all(), '%s: not overwritten / not finite' % what
        rel, e32, scale = _bound(ref64, cpu32)
        err = (got - ref64).abs().max().item() / scale
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float('inf'))
        if err > REL_FLOOR:                        # below the floor the factor does not decide
            self.worst = max(self.worst, ratio)
        print('case %s %-28s engine %.3e  fp32-cpu %.3e  ratio %6.2f  bound %.3e  scale %.3e'
              % (self.name, what, err, e32, ratio, rel, scale))
        if not err <= rel:
            self.bad.append('%s: engine %.3e > bound %.3e (fp32-cpu %.3e)' % (what, err, rel, e32))

    def finish(self):
        print('case %s largest engine / fp32-cpu ratio among engine errors above the 1e-6 floor: %.2f'
              % (self.name, self.worst))
        assert not self.bad, '\n'.join(self.bad)


def _misalign(t):
    """A contiguous copy of t that starts 4 bytes past 16-byte alignment."""
    buf = torch.empty(t.numel() + 8, device=t.device)
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


class _NanTorch:
    """Stands in for `torch` inside netgrad: every output buffer it allocates starts as NaN."""

    @staticmethod
    def empty_like(t):
        return torch.full_like(t, float('nan'))

    @staticmethod
    def empty(*size, **kw):
        return torch.full(size, float('nan'), **kw)


class _GuardedWorkspace:
    """Stands in for `_hip.workspace`: exactly the requested bytes, 0xFF-filled, with a 0xFF guard behind them, and the
    LDS NaN-poisoned ahead of the call that asked for it."""

    def __init__(self):
        self.bufs = []

    def __call__(self, device, nbytes):
        buf = torch.empty(int(nbytes) + GUARD_BYTES, dtype=torch.uint8, device=device)
        buf.fill_(255)
        _hip.check(_hip.load().inf_debug_poison_lds(_hip.stream_of(buf)), 'poison_lds')
        self.bufs.append((buf, int(nbytes)))
        return buf[:int(nbytes)]

    def check_guards(self):
        assert self.bufs
        for buf, n in self.bufs:
            assert n > 0 and bool((buf[n:] == 255).all()), 'a write past inf_grad_workspace_bytes'


def _device_net(name):
    net, inputs = _build(name)
    c = _case(name)
    netd = copy.deepcopy(net).to(DEV)
    ins = [t.to(DEV) for t in inputs]
    if c['misaligned']:
        ins = [_misalign(t) for t in ins]
    native = _hip.native_net(netd, (c['C'], c['H'], c['W']), torch.device(DEV))
    native.refresh_if_needed(_hip.stream_of(ins[0]))
    return netd, native, ins


def _wgrad_tags(stats):
    return {s['tag'] for s in stats if 800 <= s['tag'] < 900 and s['launches'] > 0}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_conv_grads_match_fp64_autograd(name, monkeypatch):
    c = _case(name)
    net, _ = _build(name)
    ref = _reference(name)
    # the inputs reach what the case is for: pre-activations on both sides of zero, the normalisation on the side meant
    for h in ref['h'][:-1]:
        assert (h > 0.05).any() and (h < -0.05).any()
    for r, s in zip(ref['ratio'], c['scales']):
        assert (r > 1.1) if s > 1 else (r < 0.9), 'sigma / coeff = %g' % r
    netd, native, (x, gout, w, eps) = _device_net(name)
    params, paramsd = _params(net), _params(netd)
    ws = _GuardedWorkspace()
    monkeypatch.setattr(netgrad, 'torch', _NanTorch)
    monkeypatch.setattr(_hip, 'workspace', ws)
    _hip.profile_begin(20000)
    try:
        grads, gx = netgrad.param_grads(native, netd, x, gout, want_x=True)
        value, grads2, gx2 = netgrad.surrogate_grads(native, netd, x, w, eps)
        torch.cuda.synchronize()
    finally:
        stats = _hip.profile_end()
    monkeypatch.undo()
    ws.check_guards()
    tags = _wgrad_tags(stats)
    print('case %s wgrad kernels: %s' % (name, ', '.join('%d %s' % (t, _hip.tag_name(t)) for t in sorted(tags))))
    assert tags == c['tags'], 'wgrad tags %s, the case is written for %s' % (sorted(tags), sorted(c['tags']))
    assert len(grads) == len(grads2) == len(params)
    rep = _Report(name)
    names = _param_names(net)
    for i, (p, pd) in enumerate(zip(params, paramsd)):
        what = names[i]
        rep.check(what, grads[pd], *ref['first'][i])
        rep.check('surrogate ' + what, grads2[pd], *ref['second'][i])
    rep.check('gx', gx, *ref['first']['x'])
    rep.check('surrogate gx', gx2, *ref['second']['x'])
    rep.check('surrogate value', value, *ref['second']['value'])
    # the Lipschitz chain's branches: an inactive layer's dW is its dW_eff (factor 1), an active layer's is not
    for l, m in enumerate(_layers(net)):
        i = [id(p) for p in params].index(id(m.weight))
        dW64, dWe64 = ref['first'][i][0], ref['dWeff'][l]
        if ref['ratio'][l] < 1:
            assert torch.equal(dW64, dWe64)
            rep.check('dW[%d] against dW_eff (inactive)' % l, grads[paramsd[i]], dWe64, ref['first'][i][1])
        else:
            assert (dW64 - dWe64).abs().max() > 0.1 * dWe64.abs().max()
    rep.finish()


# ---- the InfNetGrads contract through the C ABI (netgrad._alloc always allocates everything) ---------------------------

def _abi_call(native, netd, ins, surrogate, skip_dW=(), with_db=True, with_dpre=True, with_gx=True):
    """inf_net_param_grad / inf_net_surrogate_grad with chosen outputs left NULL; NaN-filled buffers, 0xFF workspace,
    poisoned LDS.  Returns {name: tensor} of the outputs asked for."""
    lib = _hip.load()
    x, gout, w, eps = ins
    B = x.shape[0]
    layers, acts, pre = netgrad._slots(netd)
    nan = lambda t: torch.full_like(t, float('nan'))
    dW = [None if l in skip_dW else nan(m.weight) for l, m in enumerate(layers)]
    db = [nan(m.bias) for m in layers] if with_db else None
    dbeta = [nan(acts[l].beta) if (l in acts and hasattr(acts[l], 'beta')) else None for l in range(len(layers))]
    dpre = nan(pre.beta) if (with_dpre and pre is not None) else None
    gx = nan(x) if with_gx else None
    value = torch.full((B,), float('nan'), device=x.device)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts])
    keep = (arr(dW), arr(db) if db is not None else None, arr(dbeta))
    cast = lambda a: ctypes.cast(a, ctypes.POINTER(ctypes.c_void_p)) if a is not None else \
        ctypes.POINTER(ctypes.c_void_p)()
    ng = _hip.NetGrads(cast(keep[0]), cast(keep[1]), cast(keep[2]), dpre.data_ptr() if dpre is not None else None)
    ws = _GuardedWorkspace()
    buf = ws(x.device, lib.inf_grad_workspace_bytes(native.handle, B))
    if surrogate:
        rc = lib.inf_net_surrogate_grad(native.handle, _hip.ptr(x), _hip.ptr(w), _hip.ptr(eps), _hip.ptr(value),
                                        _hip.ptr(gx), ctypes.byref(ng), B, _hip.ptr(buf), buf.numel(),
                                        _hip.stream_of(x))
    else:
        rc = lib.inf_net_param_grad(native.handle, _hip.ptr(x), _hip.ptr(gout), _hip.ptr(gx), ctypes.byref(ng), B,
                                    _hip.ptr(buf), buf.numel(), _hip.stream_of(x))
    _hip.check(rc, 'grad call')
    torch.cuda.synchronize()
    ws.check_guards()
    out = {}
    for nm, ts in (('dW', dW), ('db', db or []), ('dbeta', dbeta)):
        for l, t in enumerate(ts):
            if t is not None:
                out['%s%d' % (nm, l)] = t
    for nm, t in (('dpre', dpre), ('gx', gx)) + ((('value', value),) if surrogate else ()):
        if t is not None:
            out[nm] = t
    for nm, t in out.items():
        assert torch.isfinite(t).all(), nm
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('surrogate', [False, True], ids=['param_grad', 'surrogate'])
def test_null_outputs_are_skipped_and_the_rest_is_bit_identical(surrogate):
    """InfNetGrads: "NULL entries / arrays are skipped".  Case (b) (leading Swish, so dpre_beta exists): with dW[1], the
    db array and dpre_beta NULL, and with gx NULL, what is still written equals the full call bit for bit."""
    netd, native, ins = _device_net('b')
    full = _abi_call(native, netd, ins, surrogate)
    assert {'dW0', 'dW1', 'dW2', 'db0', 'db2', 'dbeta0', 'dbeta1', 'dpre', 'gx'} <= set(full)
    part = _abi_call(native, netd, ins, surrogate, skip_dW=(1,), with_db=False, with_dpre=False)
    assert set(part) == set(full) - {'dW1', 'db0', 'db1', 'db2', 'dpre'}
    for k, t in part.items():
        assert torch.equal(t, full[k]), k
    nogx = _abi_call(native, netd, ins, surrogate, with_gx=False)
    assert set(nogx) == set(full) - {'gx'}
    for k, t in nogx.items():
        assert torch.equal(t, full[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['bias_free', 'elu'])
def test_uncovered_conv_nets_are_refused(kind):
    """A conv net with a bias-free layer, or with ELU, is not the gradient kernels': INF_ERR_UNSUPPORTED from the
    engine, None from netgrad (the caller keeps autograd)."""
    torch.manual_seed(0)
    conv = lambda a, b, k, bias=True: InducedNormConv2d(a, b, k, 1, k // 2, bias=bias, coeff=COEFF, atol=1e-3,
                                                         rtol=1e-3)
    act = torch.nn.ELU if kind == 'elu' else Swish
    net = torch.nn.Sequential(conv(3, 16, 3), act(), conv(16, 16, 1, bias=kind != 'bias_free'), act(), conv(16, 3, 3))
    with torch.no_grad():
        net(torch.zeros(1, 3, 8, 8))
    net = net.to(DEV)
    x = torch.randn(2, 3, 8, 8, device=DEV)
    native = _hip.native_net(net, (3, 8, 8), x.device)
    native.refresh_if_needed(_hip.stream_of(x))
    assert netgrad.param_grads(native, net, x, x, want_x=True) is None
    assert netgrad.surrogate_grads(native, net, x, x, x.sign()) is None
    lib = _hip.load()
    ng, keep, _ = netgrad._alloc(net)
    ws = _hip.workspace(x.device, max(int(lib.inf_grad_workspace_bytes(native.handle, 2)), 1 << 20))
    assert lib.inf_net_param_grad(native.handle, _hip.ptr(x), _hip.ptr(x), None, ctypes.byref(ng), 2, _hip.ptr(ws),
                                  ws.numel(), _hip.stream_of(x)) == _hip.INF_ERR_UNSUPPORTED


# ---- CPU guard: the inputs tell a right contraction from a subtly wrong one ---------------------------------------------

def _wgrad64(G, X, tap_G=None, tap_shift=None):
    """dW_eff[m, i, ty, tx] = sum_{b, y, x} G[b, m, y, x] X[b, i, y + ty - 1, x + tx - 1] (zero outside the image), fp64.
    tap_G: {(ty, tx): G for that tap}; tap_shift: {(ty, tx): extra (dy, dx)} -- the faults."""
    B, M, H, W = G.shape
    Xp = F.pad(X, (2, 2, 2, 2))
    out = torch.zeros(M, X.shape[1], 3, 3, dtype=torch.float64)
    for ty in range(3):
        for tx in range(3):
            dy, dx = (tap_shift or {}).get((ty, tx), (0, 0))
            Gt = (tap_G or {}).get((ty, tx), G)
            win = Xp[:, :, 1 + ty + dy:1 + ty + dy + H, 1 + tx + dx:1 + tx + dx + W]
            out[:, :, ty, tx] = torch.einsum('bmyx,biyx->mi', Gt, win)
    return out


def _faults(name, G, X):
    """name -> faulty dW_eff of the first layer."""
    B, M, H, W = G.shape
    def z(t, idx):
        t = t.clone()
        t[idx] = 0.0
        return t
    sl = slice(None)
    out = {
        'last row of X dropped': _wgrad64(G, z(X, (sl, sl, H - 1))),
        'last column of X dropped': _wgrad64(G, z(X, (sl, sl, sl, W - 1))),
        'last sample dropped': _wgrad64(z(G, (B - 1,)), X),
        'corner tap shifted by one pixel': _wgrad64(G, X, tap_shift={(0, 0): (0, -1)}),
    }
    if name == 'f':
        # wgrad_valu3_kernel's halo elements: tap tx = 0 reads X[x0 - 1] at pixel x0, tap tx = 2 reads X[x0 + 8] at
        # pixel x0 + 7, for the chunk starts x0 = 0, 8, 16 (the image edges give zero anyway)
        for x0 in (8, 16):
            out['left halo of the chunk at %d dropped' % x0] = _wgrad64(
                G, X, tap_G={(ty, 0): z(G, (sl, sl, sl, x0)) for ty in range(3)})
        for x0 in (0, 8):
            out['right halo of the chunk at %d dropped' % x0] = _wgrad64(
                G, X, tap_G={(ty, 2): z(G, (sl, sl, sl, x0 + 7)) for ty in range(3)})
    if name == 'h':
        # wgrad_kernel's split boundary: K = B P = 640 over 2 splits, k = 319 | 320
        P = H * W
        for k in (B * P // 2 - 1, B * P // 2):
            b, p = divmod(k, P)
            idx = (b, sl, p // W, p % W)
            out['pixel k = %d at the split boundary dropped' % k] = _wgrad64(z(G, idx), X)
    return out


@pytest.mark.parametrize('name', ['a', 'f', 'h'])
def test_reference_tells_faulty_contractions_apart(name):
    """No GPU: on cases (a), (f), (h) the first layer's fp64 dW_eff is recomputed with a fault a wgrad kernel could have
    -- the last image row, the last column or the last sample of the sum dropped, one corner tap shifted by a pixel,
    (f) each halo element at an 8-pixel chunk boundary dropped, (h) the pixel on either side of the split boundary
    dropped -- and carried through the Lipschitz chain to dW.  Every fault moves dW's largest difference by at least
    10x the largest tolerance test_conv_grads_match_fp64_autograd can apply to that tensor (2e-4 of its largest
    element; the run-time bound max(8 e32, 1e-6) is smaller still).  The inputs are plain random draws; no boundary
    element had to be enlarged.  Smallest ratio found (move / 2e-4 of the scale): 130 (case h, the pixel k = 319 on the
    split boundary, 10x the bound being 10); 265 for k = 320, 527 for (f)'s halo elements and up."""
    net, _ = _build(name)
    ref = _reference(name)
    m = _layers(net)[0]
    G, X = ref['G'][0], ref['in'][0]
    dWe = _wgrad64(G, X)
    assert (dWe - ref['dWeff'][0]).abs().max() <= 1e-12 * ref['dWeff'][0].abs().max()   # the contraction is layer 0's
    # the chain to the raw weight, linear in dW_eff: dW = dW_eff / f - [sigma / coeff > 1] <dW_eff, W> / (f^2 coeff) dsig
    W = m.weight.detach().double().requires_grad_(True)
    H, Wd = X.shape[2:]
    sigma = (m.u.double().view(1, m.out_channels, H, Wd) *
             F.conv2d(m.v.double().view(1, m.in_channels, H, Wd), W, padding=1)).sum()
    dsig = torch.autograd.grad(sigma, W)[0]
    f = max(1.0, float(sigma.detach()) / m.coeff)
    assert f > 1
    chain = lambda d: d / f - (d * W.detach()).sum() / (f * f * m.coeff) * dsig
    i = [id(p) for p in _params(net)].index(id(m.weight))
    dW = ref['first'][i][0]
    scale = dW.abs().max().item()
    assert (chain(dWe) - dW).abs().max().item() <= 1e-12 * scale
    rel, e32, _ = _bound(*ref['first'][i])
    assert rel <= REL_CAP
    worst = None
    for what, bad in _faults(name, G, X).items():
        move = (chain(bad) - dW).abs().max().item() / scale
        print('case %s %-46s moves dW[0] by %.3e of its scale = %6.1f x 2e-4 (run-time bound here %.2e)'
              % (name, what, move, move / REL_CAP, rel))
        assert move >= 10 * REL_CAP, '%s would pass unnoticed: %.3e' % (what, move)
        worst = move if worst is None else min(worst, move)
    print('case %s smallest move / 2e-4: %.1f' % (name, worst / REL_CAP))
