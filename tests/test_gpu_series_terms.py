"""Every term of the power-series log-det, the Neumann vector, the exact-trace series and their gradients against fp64.

The other tests' nets (lib/synthetic.py, random weights capped per layer) have Jacobians so far below 1 that a term
beyond the second is smaller than the tolerance of the sum it belongs to: it could be zero, carry the wrong coefficient
or be read from the wrong buffer unnoticed.  Two instruments close that:

1. One-hot coefficients.  Every entry point takes its coefficients from the caller; with 1 at term k and 0 elsewhere the
   output is term k alone (eps^T J^k eps; w - eps = eps^T J^k; tr(J^k); the gradients of sum_b g_b term_k(x_b)), which is
   compared with the fp64 term at the term's OWN scale, without a max(1, .) floor:
     scalars    |got - ref| <= tol_k * sum_i |eps_i (v_k)_i|   per sample, v_k = eps^T J^k in fp64
                (the exact trace: tol_k * sum_ij |J_ij (J^(k-1))_ji|, the products its trace sums, plus one fp32
                rounding of the bare trace tr(J) that inf_logdet_exact_trace always adds: 2^-23 |tr J|);
     vectors    |got - ref|_inf <= tol_k * |v_k|_inf           per sample;
     gradients  |got - ref|_inf <= tol_k * |ref|_inf           per tensor;
   tol_k = k x the project's single-call bound against fp64 (2e-5 net forward / VJP, 2e-4 gradient tensors): a chain of
   k VJPs accumulates k roundings of that size.  inf_logdet_neumann's value (w^T J) . eps with a one-hot ncoeff is
   eps^T J eps + eps^T J^(k+1) eps: its bound is the two terms' bounds added (tol_1 scale_1 + tol_(k+1) scale_(k+1)).
   Every case prints its largest error / bound ratio per term ("Series terms against fp64").

2. Strong nets (strong_fc / strong_conv): "trained-like" nets whose layers' singular vectors line up, so the Jacobian's
   powers decay like 0.7^k, not 0.01^k, and every term of an n-term sum weighs at least 100 x the sum's tolerance
   (tests/test_series_terms_host.py asserts that on the CPU for every such net and input used here).  On them the whole
   sums with the ordinary coefficients (-1)^(k+1) / k and the Neumann coefficients of
   test_gpu_parity._k128_policies_match_64px are checked at the project's bounds: 2e-5 max(1, |ref|_inf) for values and
   vectors, 2e-4 of the tensor's max for gradients.

References: fp64 torch evaluations of the same modules on the CPU (compute_weight(update=False) semantics), computed
once per (net, input) and shared.  Workspace and LDS are NaN-filled before every engine call; the launch profile of every
call is read and the intended kernel's tag asserted.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from lib import _hip
from lib.layers import netgrad
from lib.layers.base import Sin, Swish, get_conv2d, get_linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FWD_TOL, GRAD_TOL = 2e-5, 2e-4          # the project's single-call bounds against fp64
N_CONV, N_FC, N_MAX = 6, 8, 128         # series lengths of the one-hot runs; N_MAX: CoeffTable / FcSeriesArgs / SERIES_MAX
TAG_FCSERIES = 620                      # fcblock.hip fcseries_kernel


# ---------------------------------------------------------------------------------------------------------------------
# strong nets (CPU modules; the host test imports these)
# ---------------------------------------------------------------------------------------------------------------------
def _orth(rows, cols, gen):
    q, _ = torch.linalg.qr(torch.randn(rows, cols, generator=gen, dtype=torch.float64))
    return q.float()


def _set_acts(seq, beta):
    for m in seq:
        if isinstance(m, Swish):
            m.beta.fill_(beta)


def strong_fc(d, hidden, act, depth=3, seed=0, bias=None, coeff=0.97, noise=0.1):
    """d -> hidden (x depth - 1) -> d with `act` between the linears, the layers' singular vectors lined up:
    W_first = 2 Q + noise, W_mid = 2 Q Q^T + noise, W_last = 2 R Q^T + noise (Q hidden x d with orthonormal columns, R a
    random d x d rotation, noise 0.1 / sqrt(fan_in)), then compute_weight(update=True, n_iterations=200) so that u / v
    lie in the top singular cluster and every layer sits at sigma = coeff.  Swish nets take a positive hidden bias
    (swish' near its plateau); Sin nets a zero one (cos(2 pi a) near 1 for the small inputs they are used at)."""
    with torch.random.fork_rng(devices=[]):                          # the layers' own initialisation draws globally
        torch.manual_seed(1000 + 17 * d + seed)
        return _strong_fc(d, hidden, act, depth, seed, bias, coeff, noise)


def _strong_fc(d, hidden, act, depth, seed, bias, coeff, noise):
    gen = torch.Generator().manual_seed(1000 + 17 * d + seed)
    lin = lambda a, b: get_linear(a, b, coeff=coeff, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    dims = [d] + [hidden] * (depth - 1) + [d]
    mods = []
    for i in range(depth):
        mods.append(lin(dims[i], dims[i + 1]))
        if i < depth - 1:
            mods.append(act())
    seq = torch.nn.Sequential(*mods)
    Q, R = _orth(hidden, d, gen), _orth(d, d, gen)
    bias = (3.0 if act is Swish else 0.0) if bias is None else bias
    jitter = 0.1 if act is Swish else 0.02
    with torch.no_grad():
        lins = [m for m in seq if hasattr(m, 'compute_weight')]
        for i, m in enumerate(lins):
            core = 2 * Q if i == 0 else (2 * R @ Q.t() if i == depth - 1 else 2 * Q @ Q.t())
            m.weight.copy_(core + torch.randn(m.weight.shape, generator=gen) * (noise / m.weight.shape[1] ** 0.5))
            m.bias.copy_(torch.rand(m.bias.shape, generator=gen) * jitter + (bias if i < depth - 1 else 0.0))
            m.compute_weight(update=True, n_iterations=200)
        _set_acts(seq, 0.7)
    return seq


def strong_conv(C, hid, H, W, act=Swish, lead=False, seed=0, bias=3.0, coeff=0.97, noise=0.1):
    """conv 3x3, act, conv 1x1, act, conv 3x3 on (C, H, W), with or without a leading `act`: strong_fc's structure on the
    centre tap (hid x C, hid x hid, C x hid), noise 0.1 / sqrt(fan_in) on all nine taps, positive hidden biases for
    Swish."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(2000 + 31 * C + H + seed)
        return _strong_conv(C, hid, H, W, act, lead, seed, bias, coeff, noise)


def _strong_conv(C, hid, H, W, act, lead, seed, bias, coeff, noise):
    gen = torch.Generator().manual_seed(2000 + 31 * C + H + seed)
    conv = lambda a, b, k: get_conv2d(a, b, k, 1, k // 2, coeff=coeff, n_iterations=None, atol=1e-3, rtol=1e-3,
                                      domain=2, codomain=2)
    mods = ([act()] if lead else []) + [conv(C, hid, 3), act(), conv(hid, hid, 1), act(), conv(hid, C, 3)]
    seq = torch.nn.Sequential(*mods)
    Q, R = _orth(hid, C, gen), _orth(C, C, gen)
    bias, jitter = (bias, 0.1) if act is Swish else (0.0, 0.02)
    with torch.no_grad():
        seq(torch.zeros(1, C, H, W))                                  # spatial_dims, lazy u / v
        convs = [m for m in seq if hasattr(m, 'compute_weight')]
        for i, (m, core) in enumerate(zip(convs, (2 * Q, 2 * Q @ Q.t(), 2 * R @ Q.t()))):
            k = m.weight.shape[-1]
            w = torch.randn(m.weight.shape, generator=gen) * (noise / (m.weight.shape[1] * k * k) ** 0.5)
            w[:, :, k // 2, k // 2] += core
            m.weight.copy_(w)
            m.bias.copy_(torch.rand(m.bias.shape, generator=gen) * jitter + (bias if i < 2 else 0.0))
            m.compute_weight(update=True, n_iterations=200)
        _set_acts(seq, 0.7)
    return seq


def probes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2, shape, generator=g).float() * 2 - 1


def inputs(shape, seed, scale, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale + offset


def series_coeff(n):
    return np.array([(-1) ** (k + 1) / k for k in range(1, n + 1)], dtype=np.float32)


def neumann_coeff(n):
    """test_gpu_parity._k128_policies_match_64px's: (-1)^k, halved from k = 8 on."""
    return np.array([(-1) ** k * (1.0 if k < 8 else 0.5) for k in range(n + 1)], dtype=np.float32)


def one_hot(n, k, first=1):
    """n coefficients for terms first .. first + n - 1, 1 at term k."""
    a = np.zeros(n, dtype=np.float32)
    a[k - first] = 1.0
    return a


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def ref_chain(seq, x, eps, n):
    """v_k = eps^T J(x)^k for k = 1 .. n of the module in fp64, (n, B, ...)."""
    ref = copy.deepcopy(seq).cpu().double()
    x64 = x.detach().cpu().double().requires_grad_(True)
    y = ref(x64)
    v, out = eps.detach().cpu().double(), []
    for _ in range(n):
        v = torch.autograd.grad(y, x64, v, retain_graph=True)[0]
        out.append(v)
    return torch.stack(out)


def ref_jacobian(seq, x):
    """J[b, i, j] = d f_i / d x_j of an fc module in fp64."""
    ref = copy.deepcopy(seq).cpu().double()
    x64 = x.detach().cpu().double().requires_grad_(True)
    y = ref(x64)
    return torch.stack([torch.autograd.grad(y[:, i].sum(), x64, retain_graph=True)[0] for i in range(y.shape[1])], 1)


def term_dots(chain, eps):
    """(eps . v_k per sample, sum_i |eps_i (v_k)_i| per sample), each (n, B)."""
    e = eps.detach().cpu().double().unsqueeze(0)
    p = (chain * e).flatten(2)
    return p.sum(2), p.abs().sum(2)


def fixture_margin(chain, eps, coeff, rel=FWD_TOL):
    """|c_n term_n| (max over samples) over the absolute tolerance rel * max(1, |S|_inf) of the n-term sum S."""
    dots, _ = term_dots(chain, eps)
    c = torch.tensor(np.asarray(coeff, dtype=np.float64)).unsqueeze(1)
    S = (c * dots).sum(0)
    return (c[-1] * dots[-1]).abs().max().item() / (rel * max(1.0, S.abs().max().item()))


# ---------------------------------------------------------------------------------------------------------------------
# the cases (the host test walks STRONG_CASES; the GPU tests build the same nets and inputs)
# ---------------------------------------------------------------------------------------------------------------------
# name -> (builder kwargs, (C, H, W), B of the widest use, input scale, input offset, n of the whole-sum check)
CONV_NETS = {
    's0': (dict(C=3, hid=512, H=32, W=32), 17, 0.5, 0.0, 8),
    's0_z': (dict(C=3, hid=512, H=32, W=32, seed=1), 9, 0.5, 0.0, 8),
    'rt_lead': (dict(C=5, hid=512, H=16, W=16, lead=True), 65, 0.5, 2.5, 8),
    'rt_first': (dict(C=5, hid=512, H=16, W=16), 65, 0.5, 0.0, 8),
    'wide': (dict(C=48, hid=512, H=8, W=8, lead=True), 3, 0.5, 2.5, 8),
    'ragged': (dict(C=3, hid=512, H=28, W=28, lead=True), 3, 0.5, 2.5, 8),
    'hid64': (dict(C=3, hid=64, H=16, W=16, lead=True), 3, 0.5, 2.5, 8),
    'sin': (dict(C=3, hid=512, H=32, W=32, act=Sin, lead=True), 3, 0.03, 0.0, 8),
}
# name -> (d, hidden, act, depth, B, input scale, n of the whole-sum check)
FC_NETS = {
    'sin2': (2, 128, Sin, 3, 49, 0.03, 10), 'swish2': (2, 128, Swish, 3, 48, 0.3, 8),
    'sin6': (6, 128, Sin, 5, 65, 0.03, 10), 'swish6': (6, 128, Swish, 5, 49, 0.3, 8),
    'sin8': (8, 128, Sin, 3, 48, 0.03, 10), 'swish8': (8, 128, Swish, 3, 1, 0.3, 8),
    'sin16': (16, 128, Sin, 3, 65, 0.03, 10), 'swish16': (16, 128, Swish, 3, 49, 0.3, 8),
    'sin6_h64': (6, 64, Sin, 3, 65, 0.03, 10),
    'sin17': (17, 64, Sin, 3, 49, 0.03, 10), 'swish43': (43, 64, Swish, 3, 65, 0.3, 8),
    'sin43': (43, 64, Sin, 3, 48, 0.03, 10),
}


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """(module on the CPU, x, eps) of a CONV_NETS entry at its widest batch; narrower uses take the first samples."""
    kw, B, scale, offset, _ = CONV_NETS[name]
    seq = strong_conv(**kw)
    shape = (B, kw['C'], kw['H'], kw['W'])
    seed = sum(map(ord, name))
    return seq, inputs(shape, seed, scale, offset), probes(shape, seed + 1)


@functools.lru_cache(maxsize=None)
def fc_case(name):
    d, hidden, act, depth, B, scale, _ = FC_NETS[name]
    seq = strong_fc(d, hidden, act, depth)
    seed = sum(map(ord, name))
    return seq, inputs((B, d), seed, scale), probes((B, d), seed + 1)


@functools.lru_cache(maxsize=None)
def conv_chain(name, n=8):
    seq, x, eps = conv_case(name)
    return ref_chain(seq, x, eps, n)


@functools.lru_cache(maxsize=None)
def fc_chain(name, n=10):
    seq, x, eps = fc_case(name)
    return ref_chain(seq, x, eps, n)


# ---------------------------------------------------------------------------------------------------------------------
# engine calls: NaN-filled workspace and LDS before each, the launch profile {tag: launches} returned with the result
# ---------------------------------------------------------------------------------------------------------------------
def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _native(seq_dev, shape, mfma=None, options=()):
    net = _hip.NativeNet(_hip.net_entries(seq_dev), shape, torch.device(DEV))   # fresh: reads INFLOW_NO_FUSED
    if mfma is not None:
        _hip.check(net.lib.inf_net_set_mfma(net.handle, mfma), 'set_mfma')
    for o, v in options:
        net.set_option(o, v)
    net.refresh_if_needed(_hip.stream_of(torch.empty(1, device=DEV)))
    return net


def _call(nets, nbytes, fn):
    stream = _hip.stream_of(torch.empty(1, device=DEV))
    ws = _hip.workspace(torch.device(DEV), nbytes)
    ws.fill_(255)
    _hip.check(nets[0].lib.inf_debug_poison_lds(stream), 'poison_lds')
    _hip.profile_begin(4000)
    try:
        _hip.check(fn(ws, stream), fn.__name__)
        torch.cuda.synchronize()
    finally:
        tags = {s['tag']: s['launches'] for s in _hip.profile_end()}
    return tags


def e_series(net, x, eps, co):
    B, out = x.shape[0], torch.empty(x.shape[0], device=DEV)
    tags = _call((net,), net.ws_bytes(B), lambda ws, s: net.lib.inf_logdet_series(
        net.handle, _hip.ptr(x), _hip.ptr(eps), _fptr(co), len(co), _hip.ptr(out), B, _hip.ptr(ws), ws.numel(), s))
    return out.double().cpu(), tags


def e_series_pair(nx, nz, x, z, ex, ez, co):
    B, out = x.shape[0], torch.empty(2, x.shape[0], device=DEV)
    tags = _call((nx, nz), 2 * max(nx.ws_bytes(B), nz.ws_bytes(B)), lambda ws, s: nx.lib.inf_logdet_series_pair(
        nx.handle, _hip.ptr(x), _hip.ptr(ex), nz.handle, _hip.ptr(z), _hip.ptr(ez), _fptr(co), len(co),
        _hip.ptr(out[0]), _hip.ptr(out[1]), B, _hip.ptr(ws), ws.numel(), s))
    return out.double().cpu(), tags


def e_neumann(net, x, eps, nco):
    B, w = x.shape[0], torch.empty_like(x)
    tags = _call((net,), net.ws_bytes(B), lambda ws, s: net.lib.inf_neumann_vector(
        net.handle, _hip.ptr(x), _hip.ptr(eps), _fptr(nco), len(nco) - 1, _hip.ptr(w), B, _hip.ptr(ws), ws.numel(), s))
    return w.double().cpu(), tags


def e_neumann_pair(nx, nz, x, z, ex, ez, nco):
    B, wa, wb = x.shape[0], torch.empty_like(x), torch.empty_like(z)
    tags = _call((nx, nz), 2 * max(nx.ws_bytes(B), nz.ws_bytes(B)), lambda ws, s: nx.lib.inf_neumann_vector_pair(
        nx.handle, _hip.ptr(x), _hip.ptr(ex), nz.handle, _hip.ptr(z), _hip.ptr(ez), _fptr(nco), len(nco) - 1,
        _hip.ptr(wa), _hip.ptr(wb), B, _hip.ptr(ws), ws.numel() // 2 * 2, s))
    return torch.stack([wa, wb]).double().cpu(), tags


def e_logdet_neumann(net, x, eps, nco):
    B, out = x.shape[0], torch.empty(x.shape[0], device=DEV)
    tags = _call((net,), net.ws_bytes(B), lambda ws, s: net.lib.inf_logdet_neumann(
        net.handle, _hip.ptr(x), _hip.ptr(eps), _fptr(nco), len(nco) - 1, _hip.ptr(out), B, _hip.ptr(ws), ws.numel(), s))
    return out.double().cpu(), tags


def e_exact_trace(net, x, co):
    B, out = x.shape[0], torch.empty(x.shape[0], device=DEV)
    tags = _call((net,), net.ws_bytes(B), lambda ws, s: net.lib.inf_logdet_exact_trace(
        net.handle, _hip.ptr(x), _fptr(co), len(co), _hip.ptr(out), B, _hip.ptr(ws), ws.numel(), s))
    return out.double().cpu(), tags


# ---------------------------------------------------------------------------------------------------------------------
# comparisons at the term's own scale
# ---------------------------------------------------------------------------------------------------------------------
class Ratios:
    """Largest error / bound per term of one case; printed, then asserted <= 1."""

    def __init__(self, what):
        self.what, self.r = what, {}

    def add(self, k, got, ref, bound):
        assert torch.isfinite(got).all(), (self.what, k, 'not finite')
        err = (got - ref).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        self.r[k] = max(self.r.get(k, 0.0), ratio)

    def check(self):
        print('%s: max err / bound per term: %s' % (self.what, ' '.join('k%d %.3f' % kv for kv in sorted(self.r.items()))))
        bad = {k: v for k, v in self.r.items() if not v <= 1.0}
        assert not bad, (self.what, bad)


def _vec_bound(ref_k, k):
    """tol_k |v_k|_inf per sample, broadcast over the sample's elements."""
    m = ref_k.flatten(1).abs().max(1)[0]
    return (k * FWD_TOL * m).view(-1, *([1] * (ref_k.dim() - 1))).expand_as(ref_k)


def _close_sum(got, ref, what, rel=FWD_TOL):
    """The project's bound for a whole sum against fp64: rel * max(1, |ref|_inf)."""
    assert torch.isfinite(got).all(), what
    err, bound = (got - ref).abs().max().item(), rel * max(1.0, ref.abs().max().item())
    print('%s: max err %.3e  bound %.3e' % (what, err, bound))
    assert err <= bound, (what, err, bound)


def _vjp_tags(tags):
    """The fused conv VJP launches of a profile: {tag: launches} for tags 5x2."""
    return {t: c for t, c in tags.items() if 500 <= t < 600 and t % 10 == 2}


# ---------------------------------------------------------------------------------------------------------------------
# conv nets
# ---------------------------------------------------------------------------------------------------------------------
K128, GROUP = _hip.INF_OPT_FUSED_K128, _hip.INF_OPT_SERIES_GROUP
# The launcher's rule at (3, 32, 32) (fused313.hip net313_family; nets x B images of 16 64-pixel / 32 32-pixel tiles): the
# 64-pixel layout (and with it the 128-pixel and two-per-CU 64-pixel kernels) from 256 64-pixel tiles on -- B >= 16 for one
# net, B >= 8 for a pair; below that the 32-pixel two-per-CU variant, and the wide 32-pixel one up to 256 32-pixel tiles --
# B <= 8 for one net, B <= 4 for a pair.  So B = 3 runs on the wide variant (522) whatever the shape, a single net at B = 9
# (the pair runs' own single-net calls) and a pair at B = 6 on the two-per-CU variant (512).
# id -> (x net, z net or None, B, mfma, options, env INFLOW_NO_FUSED, the VJP tag every term of a single-net call must
# launch on, that of a pair call; None: the GEMM chain)
CONV_RUNS = {
    '32px_wide_b3': ('s0', 's0_z', 3, 2, (), 0, 522, 522),
    '32px_2cu_pair_b6': ('s0', 's0_z', 6, 2, (), 0, 522, 512),
    '64px_single': ('s0', None, 17, 2, ((K128, 0),), 0, 502, None),
    '64px_pair': ('s0', 's0_z', 9, 2, ((K128, 0),), 0, 512, 502),
    '128px_single': ('s0', None, 17, 2, ((K128, 2),), 0, 532, None),
    '128px_pair': ('s0', 's0_z', 9, 2, ((K128, 2),), 0, 512, 532),
    '64px_2cu_single': ('s0', None, 17, 2, ((K128, 3),), 0, 542, None),
    '64px_2cu_pair': ('s0', 's0_z', 9, 2, ((K128, 3),), 0, 512, 542),
    'group6_of_17': ('s0', None, 17, 2, ((K128, 2), (GROUP, 6)), 0, 532, None),
    'group4_of_9_pair': ('s0', 's0_z', 9, 2, ((K128, 2), (GROUP, 4)), 0, 512, 532),
    'runtime_lead': ('rt_lead', None, 65, 2, ((K128, 2),), 0, 532, None),
    'runtime_first': ('rt_first', None, 65, 2, ((K128, 2),), 0, 532, None),
    'wide_32px': ('wide', None, 3, 2, (), 0, 522, None),
    'ragged_28': ('ragged', None, 3, 2, (), 0, 522, None),
    'gemm_chain_512': ('s0', None, 3, 2, (), 1, None, None),
    'gemm_chain_hid64': ('hid64', None, 3, 2, (), 0, None, None),
    'sin_lead': ('sin', None, 3, 2, (), 0, 522, None),
    'mfma_f32': ('s0', 's0_z', 3, 0, (), 0, 522, 522),
    'mfma_bf16x6': ('s0', 's0_z', 3, 1, (), 0, 522, 522),
}


def _conv_setup(run, monkeypatch):
    xname, zname, B, mfma, options, no_fused, tag, pair_tag = CONV_RUNS[run]
    monkeypatch.setenv('INFLOW_NO_FUSED', str(no_fused))
    side = []
    for name in (xname, zname):
        if name is None:
            continue
        seq, x, eps = conv_case(name)
        assert B <= x.shape[0]
        seqd = copy.deepcopy(seq).to(DEV)
        net = _native(seqd, tuple(x.shape[1:]), mfma, options)
        side.append((name, seqd, net, x[:B].to(DEV).contiguous(), eps[:B].to(DEV).contiguous()))
    return side, B, tag, pair_tag


def _groups(run, B):
    g = dict(CONV_RUNS[run][4]).get(GROUP)
    return -(-B // g) if g else 1


@pytest.mark.parametrize('run', sorted(CONV_RUNS))
def test_conv_terms_one_hot(run, monkeypatch):
    """Term k = 1 .. 6 alone from every conv series entry, on each kernel family the series launches on: the wide
    32-pixel variant (B = 3) and the two-per-CU one (a pair at B = 6, one net at B = 9) at (3, 32, 32), the 64-pixel,
    128-pixel and two-per-CU 64-pixel kernels under INF_OPT_FUSED_K128 0 / 2 / 3 (B = 17 single, B = 9 pair), the runtime-geometry instantiation with and without the leading Swish ((5, 16, 16),
    B = 65; without: no vmul_x), the wide 32-pixel kernel ((48, 8, 8)), ragged tiles ((3, 28, 28)), the GEMM chain
    (INFLOW_NO_FUSED = 1, and a 64-wide net), a leading-Sin net, MFMA modes 0 and 1, and forced sample groups with a
    short last group (6 + 6 + 5 of 17; 4 + 4 + 1 of 9) -- against fp64, not against the ungrouped run.
    Bounds: k x 2e-5 at the term's own scale (module docstring); no path needed more."""
    side, B, tag, pair_tag = _conv_setup(run, monkeypatch)
    n = N_CONV
    chains = [conv_chain(name)[:, :B] for name, *_ in side]
    dots = [term_dots(c, e.cpu()) for c, (_, _, _, _, e) in zip(chains, side)]
    groups = _groups(run, B)

    def ran_on(tags, launches, what, k, tag=tag):
        if tag is None:
            assert not _vjp_tags(tags), (what, k, tags)
            assert any(t >= 1000 for t in tags), (what, k, tags)                # GEMM-chain launches
        else:
            assert _vjp_tags(tags) == {tag: launches}, (what, k, tags)

    rs = {w: Ratios('%s %s' % (run, w)) for w in ('series', 'series_pair', 'neumann', 'neumann_pair', 'logdet_neumann')}
    _, _, net, x, eps = side[0]
    for k in range(1, n + 1):
        co, nco = one_hot(n, k), one_hot(n + 1, k, first=0)
        got, tags = e_series(net, x, eps, co)
        ran_on(tags, n * groups, 'series', k)
        rs['series'].add(k, got, dots[0][0][k - 1], k * FWD_TOL * dots[0][1][k - 1])
        got, tags = e_neumann(net, x, eps, nco)
        ran_on(tags, n, 'neumann', k)
        w_ref = chains[0][k - 1]
        rs['neumann'].add(k, got - eps.double().cpu(), w_ref, _vec_bound(w_ref, k))
        got, tags = e_logdet_neumann(net, x, eps, nco[:k + 1])      # (w^T J) . eps = eps^T J eps + eps^T J^(k+1) eps
        ran_on(tags, k + 1, 'logdet_neumann', k)
        ref = dots[0][0][0] + dots[0][0][k]
        rs['logdet_neumann'].add(k, got, ref, FWD_TOL * dots[0][1][0] + (k + 1) * FWD_TOL * dots[0][1][k])
        if len(side) == 2:
            (_, _, nx, x, ex), (_, _, nz, z, ez) = side
            got, tags = e_series_pair(nx, nz, x, z, ex, ez, co)
            ran_on(tags, n * groups, 'series_pair', k, pair_tag)
            for i in range(2):
                rs['series_pair'].add(k, got[i], dots[i][0][k - 1], k * FWD_TOL * dots[i][1][k - 1])
            got, tags = e_neumann_pair(nx, nz, x, z, ex, ez, nco)
            ran_on(tags, n * groups, 'neumann_pair', k, pair_tag)
            for i, e in enumerate((ex, ez)):
                w_ref = chains[i][k - 1]
                rs['neumann_pair'].add(k, got[i] - e.double().cpu(), w_ref, _vec_bound(w_ref, k))
    for r in rs.values():
        if r.r:
            r.check()


CONV_SUM_RUNS = ['32px_wide_b3', '32px_2cu_pair_b6', '64px_pair', '128px_single', '128px_pair', '64px_2cu_single', 'group6_of_17',
                 'runtime_lead', 'runtime_first', 'wide_32px', 'ragged_28', 'gemm_chain_hid64', 'sin_lead']


@pytest.mark.parametrize('run', CONV_SUM_RUNS)
def test_conv_sums_on_strong_nets(run, monkeypatch):
    """The whole sums with the ordinary coefficients, one conv shape per kernel family: inf_logdet_series[_pair],
    inf_neumann_vector[_pair] and inf_logdet_neumann against fp64 within 2e-5 max(1, |ref|_inf), on nets where the last
    term alone weighs >= 100 x that bound (tests/test_series_terms_host.py)."""
    side, B, tag, pair_tag = _conv_setup(run, monkeypatch)
    n = CONV_NETS[side[0][0]][4]
    co, nco = series_coeff(n), neumann_coeff(n)
    refs = []
    for name, _, _, _, e in side:
        chain = conv_chain(name)[:n, :B]
        dots, _ = term_dots(chain, e.cpu())
        S = (torch.tensor(co.astype(np.float64)).unsqueeze(1) * dots).sum(0)
        c = torch.tensor(nco[1:].astype(np.float64)).view(-1, *([1] * (chain.dim() - 1)))
        w = e.double().cpu() + (c * chain).sum(0)
        refs.append((S, w))
    _, seqd, net, x, eps = side[0]
    got, tags = e_series(net, x, eps, co)
    assert tag is None or set(_vjp_tags(tags)) == {tag}, tags
    _close_sum(got, refs[0][0], run + ' series')
    got, _ = e_neumann(net, x, eps, nco)
    _close_sum(got, refs[0][1], run + ' neumann')
    # (w^T J) . eps in fp64: one more VJP of the reference w
    ref64 = copy.deepcopy(seqd).cpu().double()
    x64 = x.double().cpu().requires_grad_(True)
    wj = torch.autograd.grad(ref64(x64), x64, refs[0][1])[0]
    got, _ = e_logdet_neumann(net, x, eps, nco)
    _close_sum(got, (wj * eps.double().cpu()).flatten(1).sum(1), run + ' logdet_neumann')
    if len(side) == 2:
        (_, _, nx, x, ex), (_, _, nz, z, ez) = side
        got, tags = e_series_pair(nx, nz, x, z, ex, ez, co)
        assert set(_vjp_tags(tags)) == {pair_tag}, tags
        got_w, _ = e_neumann_pair(nx, nz, x, z, ex, ez, nco)
        for i in range(2):
            _close_sum(got[i], refs[i][0], '%s series_pair[%d]' % (run, i))
            _close_sum(got_w[i], refs[i][1], '%s neumann_pair[%d]' % (run, i))


def _imblock_eval(nx, nz, x, ex, ez, co, T, eps_forward):
    B = x.shape[0]
    z, out, st = torch.empty_like(x), torch.empty(2, B, device=DEV), _hip.BroydenStats()
    tags = _call((nx, nz), nx.ws_bytes(B, T) + nz.ws_bytes(B, 1) + nx.ws_bytes(B, 1), lambda ws, s: nx.lib.inf_imblock_eval(
        nx.handle, nz.handle, _hip.ptr(x), _hip.ptr(z), _hip.ptr(ex), _hip.ptr(ez), _fptr(co), len(co), _hip.ptr(out[0]),
        _hip.ptr(out[1]), B, T, eps_forward, ctypes.byref(st), _hip.ptr(ws), ws.numel(), s))
    return z, out.double().cpu(), st, tags


@pytest.mark.parametrize('overlap', [0, 1])
def test_imblock_eval_on_a_strong_pair(overlap, monkeypatch):
    """inf_imblock_eval on a strong pair of (3, 32, 32) nets, B = 3, both schedules: both returned log-dets against the
    fp64 series evaluated at x and at the returned z (2e-5 max(1, |ref|_inf)); the fp64 residual of
    x + f_x(x) - z - f_z(z) at the solver's tolerance (|r|_F <= eps sqrt(B d) is its stopping rule; the fp32 evaluations
    of f_x and f_z add at most 2e-5 max(1, |f|_inf) per element on top: the bound is their sum in the Frobenius norm); and
    the solve took more steps than on a weak pair (the same layers at their default random initialisation, the kind of
    net the other tests use)."""
    monkeypatch.setenv('INFLOW_NO_FUSED', '0')
    T, tol, n, B = 30, 1e-6, 8, 3
    co = series_coeff(n)
    steps = {}
    for kind in ('strong', 'weak'):
        seqs = [conv_case('s0')[0], conv_case('s0_z')[0]]
        if kind == 'weak':
            seqs = [torch.nn.Sequential(*[get_conv2d(a, b, k, 1, k // 2, coeff=0.9, n_iterations=None, atol=1e-3,
                                                     rtol=1e-3, domain=2, codomain=2) if k else Swish()
                                          for a, b, k in ((3, 512, 3), (0, 0, 0), (512, 512, 1), (0, 0, 0), (512, 3, 3))])
                    for _ in range(2)]
            torch.manual_seed(5)
            with torch.no_grad():
                for s in seqs:
                    s(torch.zeros(1, 3, 32, 32))
        x = conv_case('s0')[1][:B].to(DEV).contiguous()
        ex, ez = (conv_case(nm)[2][:B].to(DEV).contiguous() for nm in ('s0', 's0_z'))
        seqd = [copy.deepcopy(s).to(DEV) for s in seqs]
        nx, nz = (_native(s, (3, 32, 32), 2, ((_hip.INF_OPT_EVAL_OVERLAP, overlap),)) for s in seqd)
        z, out, st, tags = _imblock_eval(nx, nz, x, ex, ez, co, T, tol)
        steps[kind] = st.nstep
        if kind == 'weak':
            continue
        assert not st.prot_break and torch.isfinite(z).all()
        assert _vjp_tags(tags), tags
        z64, x64 = z.double().cpu(), x.double().cpu()
        with torch.no_grad():
            fx, fz = copy.deepcopy(seqs[0]).double()(x64), copy.deepcopy(seqs[1]).double()(z64)
        resid = (x64 + fx - z64 - fz).norm().item()
        bound = (tol + FWD_TOL * max(1.0, fx.abs().max().item(), fz.abs().max().item())) * (x64.numel() ** 0.5)
        print('imblock_eval overlap %d: nstep %d  fp64 residual %.3e (bound %.3e)' % (overlap, st.nstep, resid, bound))
        assert resid <= bound
        for i, (seq, at, e) in enumerate(((seqs[0], x64, ex.cpu()), (seqs[1], z64, ez.cpu()))):
            chain = ref_chain(seq, at, e, n)
            margin = fixture_margin(chain, e, co)            # the fixture condition, at the returned z too
            print('imblock logdet_%s: last term / tolerance %.0f' % ('xz'[i], margin))
            assert margin >= 100.0
            dots, _ = term_dots(chain, e)
            ref = (torch.tensor(co.astype(np.float64)).unsqueeze(1) * dots).sum(0)
            _close_sum(out[i], ref, 'imblock logdet_' + 'xz'[i])
    print('nstep strong %d weak %d' % (steps['strong'], steps['weak']))
    assert steps['strong'] > steps['weak']


# ---------------------------------------------------------------------------------------------------------------------
# fc nets
# ---------------------------------------------------------------------------------------------------------------------
def _fc_setup(name, B=None, no_fused=False, monkeypatch=None):
    if monkeypatch is not None:
        monkeypatch.setenv('INFLOW_NO_FUSED', '1' if no_fused else '0')
    seq, x, eps = fc_case(name)
    B = x.shape[0] if B is None else B
    seqd = copy.deepcopy(seq).to(DEV)
    net = _native(seqd, (x.shape[1],))
    return seq, seqd, net, x[:B].to(DEV).contiguous(), eps[:B].to(DEV).contiguous()


def _fc_series_tag_ok(name, tags):
    """fcseries_kernel exists for d = 6 with five layers and d = 2 with three (f16x3, 128 wide): one launch, nothing else."""
    d, hidden, _, depth = FC_NETS[name][:4]
    if hidden == 128 and (d, depth) in ((6, 5), (2, 3)):
        assert tags == {TAG_FCSERIES: 1}, (name, tags)
    else:
        assert TAG_FCSERIES not in tags and tags, (name, tags)
    if d > 32:                                                      # the skinny GEMM family (gemm_skinny.hip, 960 - 962)
        assert any(960 <= t <= 962 for t in tags), (name, tags)


def _trace_refs(J, n):
    """tr(J^k) and sum_ij |J_ij (J^(k-1))_ji| for k = 1 .. n, each (n, B)."""
    d = J.shape[1]
    P = torch.eye(d, dtype=torch.float64).expand_as(J)
    tr, sc = [], []
    for _ in range(n):
        sc.append((J * P.transpose(1, 2)).abs().sum((1, 2)))
        P = torch.bmm(J, P)
        tr.append(P.diagonal(dim1=1, dim2=2).sum(1))
    return torch.stack(tr), torch.stack(sc)


FC_SERIES_NETS = sorted(FC_NETS)
FC_JAC_NETS = [n for n in FC_SERIES_NETS if FC_NETS[n][0] <= 16]


@pytest.mark.parametrize('name', FC_SERIES_NETS)
def test_fc_terms_one_hot(name, monkeypatch):
    """Term k = 1 .. 8 alone from inf_logdet_series, inf_logdet_series_pair (the net at x beside itself at the reversed
    batch with the negated probes: two different columns per sample index), inf_neumann_vector, inf_logdet_neumann and,
    up to d = 16, inf_logdet_exact_trace: d = 2, 6, 8, 16 at hidden 128 (fcseries_kernel where it exists -- d = 6 with
    five layers, d = 2 with three -- else the fused fc VJP per term), hidden 64 (the generic path), d = 17 and 43 (the
    skinny GEMMs); B = 1, 48, 49, 65 spread over the nets (48 samples per fcseries workgroup, 16 per Jacobian workgroup,
    64 per pairs block).  Bounds: k x 2e-5 at the term's own scale."""
    seq, seqd, net, x, eps = _fc_setup(name, monkeypatch=monkeypatch)
    d, n = x.shape[1], N_FC
    chain = fc_chain(name)
    dots, scale = term_dots(chain, eps.cpu())
    xr, er = x.flip(0).contiguous(), (-eps.flip(0)).contiguous()
    rs = {w: Ratios('%s %s' % (name, w)) for w in ('series', 'series_pair', 'neumann', 'logdet_neumann', 'exact_trace')}
    if d <= 16:
        tr, tr_scale = _trace_refs(ref_jacobian(seq, x), n)
    for k in range(1, n + 1):
        co, nco = one_hot(n, k), one_hot(n + 1, k, first=0)
        got, tags = e_series(net, x, eps, co)
        _fc_series_tag_ok(name, tags)
        rs['series'].add(k, got, dots[k - 1], k * FWD_TOL * scale[k - 1])
        got, tags = e_series_pair(net, net, x, xr, eps, er, co)
        _fc_series_tag_ok(name, tags)
        rs['series_pair'].add(k, got[0], dots[k - 1], k * FWD_TOL * scale[k - 1])
        rs['series_pair'].add(k, got[1], dots[k - 1].flip(0), k * FWD_TOL * scale[k - 1].flip(0))
        got, _ = e_neumann(net, x, eps, nco)
        rs['neumann'].add(k, got - eps.double().cpu(), chain[k - 1], _vec_bound(chain[k - 1], k))
        got, _ = e_logdet_neumann(net, x, eps, nco[:k + 1])
        rs['logdet_neumann'].add(k, got, dots[0] + dots[k], FWD_TOL * scale[0] + (k + 1) * FWD_TOL * scale[k])
        if d <= 16:
            got, tags = e_exact_trace(net, x, co)
            if d in (2, 6) and FC_NETS[name][1] == 128:
                assert 601 in tags, tags                                          # the fused Jacobian (fcnet_kernel<JAC>)
            ref = tr[0] + (tr[k - 1] if k > 1 else 0.0)                       # coeff[0] unused: the bare trace's 1
            bound = FWD_TOL * tr_scale[0] + (k * FWD_TOL * tr_scale[k - 1] if k > 1 else 0.0) + 2.0 ** -23 * tr[0].abs()
            rs['exact_trace'].add(k, got, ref, bound)
    for r in rs.values():
        if r.r:
            r.check()


def test_fc_terms_at_the_table_limit(monkeypatch):
    """n = 128, the limit of CoeffTable, FcSeriesArgs::coeff and SERIES_MAX, one-hot at k = 1, 64, 128 on the strong Sin
    net at d = 6 (fcseries_kernel's in-kernel VJP loop; trace_series_kernel; logdet_pairs_kernel's value in SERIES and
    TRACE mode): bounds k x 2e-5 at the term's own scale."""
    name, n = 'sin6', N_MAX
    seq, seqd, net, x, eps = _fc_setup(name, monkeypatch=monkeypatch)
    chain = ref_chain(seq, x, eps, n)
    dots, scale = term_dots(chain, eps.cpu())
    tr, tr_scale = _trace_refs(ref_jacobian(seq, x), n)
    g = torch.ones(x.shape[0], device=DEV)
    rs = {w: Ratios('%s n=128 %s' % (name, w)) for w in ('series', 'series_pair', 'exact_trace', 'grad_series_value',
                                                         'grad_trace_value')}
    for k in (1, 64, 128):
        co = one_hot(n, k)
        got, tags = e_series(net, x, eps, co)
        assert tags == {TAG_FCSERIES: 1}, tags
        rs['series'].add(k, got, dots[k - 1], k * FWD_TOL * scale[k - 1])
        got, tags = e_series_pair(net, net, x, x, eps, eps, co)
        assert tags == {TAG_FCSERIES: 1}, tags
        for i in range(2):
            rs['series_pair'].add(k, got[i], dots[k - 1], k * FWD_TOL * scale[k - 1])
        got, _ = e_exact_trace(net, x, co)
        ref = tr[0] + (tr[k - 1] if k > 1 else 0.0)
        bound = FWD_TOL * tr_scale[0] + (k * FWD_TOL * tr_scale[k - 1] if k > 1 else 0.0) + 2.0 ** -23 * tr[0].abs()
        rs['exact_trace'].add(k, got, ref, bound)
        value, _, _ = _logdet_grads(net, seqd, x, netgrad.LOGDET_SERIES, eps, co, g)
        rs['grad_series_value'].add(k, value, dots[k - 1], k * FWD_TOL * scale[k - 1])
        value, _, _ = _logdet_grads(net, seqd, x, netgrad.LOGDET_TRACE, None, co, g)
        rs['grad_trace_value'].add(k, value, tr[k - 1], k * FWD_TOL * tr_scale[k - 1])
    for r in rs.values():
        r.check()


def _logdet_grads(net, seqd, x, mode, eps, co, g):
    """netgrad.logdet_grads on a NaN-filled workspace and LDS; (value, {param: grad}, gx) as fp64 CPU tensors."""
    B = x.shape[0]
    n_terms = len(co) if co is not None else 1
    ws = _hip.workspace(x.device, net.lib.inf_logdet_grad_workspace_bytes(net.handle, B, mode, n_terms))
    ws.fill_(255)
    _hip.check(net.lib.inf_debug_poison_lds(_hip.stream_of(x)), 'poison_lds')
    res = netgrad.logdet_grads(net, seqd, x, mode, eps, co, g)
    assert res is not None
    torch.cuda.synchronize()
    value, grads, gx = res
    return value.double().cpu(), {p: t.double().cpu() for p, t in grads.items()}, gx.double().cpu()


def _grad_ref(seq, x, mode, eps, co, g):
    """test_gpu_fcgrad._ref on the CPU module: S, d/dx and {CPU parameter: gradient} of sum_b g_b S_b in fp64."""
    from test_gpu_fcgrad import _ref
    return _ref(seq, x.cpu(), mode, eps.cpu() if eps is not None else None, co, g.cpu())


def _check_grads(r, k, tol, seq, seqd, got, ref):
    """gx and every parameter gradient within tol of the reference tensor's max."""
    (_, grads, gx), (_, gx_ref, gp_ref) = got, ref
    by_name = dict(seqd.named_parameters())
    scale = lambda t: torch.full_like(t, tol * t.abs().max().item())
    r.add(k, gx, gx_ref, scale(gx_ref))
    assert len(gp_ref) >= 6
    for name, p in seq.named_parameters():
        r.add(k, grads[by_name[name]], gp_ref[p], scale(gp_ref[p]))


FC_GRAD_NETS = ['sin2', 'swish2', 'sin6', 'swish6', 'swish8', 'sin16', 'swish16', 'sin6_h64']


@pytest.mark.parametrize('name', FC_GRAD_NETS + ['sin17', 'swish43'])
def test_fc_grad_terms_one_hot(name, monkeypatch):
    """inf_logdet_grad with one-hot coefficients, n = 8: the value is term k and gx and every parameter gradient are the
    gradients of sum_b g_b term_k(x_b) (random g), against fp64 autograd with create_graph as test_gpu_fcgrad._ref.
    SERIES mode (the sums A_m = g sum_j c_(j+m+1) a_j of logdet_pairs_kernel; of series_pairs_wide_kernel at d = 17 and
    43, tag 722) and, up to d = 16, TRACE mode (P = sum k c_k J^(k-1)).  Bounds: value k x 2e-5 at the term's own scale,
    gradients k x 2e-4 of the reference tensor's max."""
    seq, seqd, net, x, eps = _fc_setup(name, monkeypatch=monkeypatch)
    d, n = x.shape[1], N_FC
    g = inputs((x.shape[0],), 77, 1.0).to(DEV)
    modes = [('series', netgrad.LOGDET_SERIES)] + ([('trace', netgrad.LOGDET_TRACE)] if d <= 16 else [])
    for label, mode in modes:
        rv, rg = Ratios('%s grad %s value' % (name, label)), Ratios('%s grad %s gradients' % (name, label))
        for k in range(1, n + 1):
            co = one_hot(n, k)
            e = eps if mode == netgrad.LOGDET_SERIES else None
            _hip.profile_begin(4000)
            try:
                got = _logdet_grads(net, seqd, x, mode, e, co, g)
            finally:
                tags = {s['tag'] for s in _hip.profile_end()}
            assert (722 in tags) == (d > 16), sorted(tags)
            ref = _grad_ref(seq, x, mode, e, co, g)
            if mode == netgrad.LOGDET_SERIES:
                _, vscale = term_dots(fc_chain(name)[k - 1:k], eps.cpu())
                vscale = vscale[0]
            else:
                vscale = _trace_refs(ref_jacobian(seq, x), k)[1][k - 1]
            rv.add(k, got[0], ref[0], k * FWD_TOL * vscale)
            _check_grads(rg, k, k * GRAD_TOL, seq, seqd, got, ref)
        rv.check()
        rg.check()


FC_SUM_NETS = ['sin2', 'swish2', 'sin6', 'swish6', 'sin16', 'swish16', 'sin43', 'swish43']


@pytest.mark.parametrize('name', FC_SUM_NETS)
def test_fc_sums_on_strong_nets(name, monkeypatch):
    """The whole sums on strong fc nets, d = 2, 6, 16, 43: inf_logdet_series[_pair], inf_neumann_vector,
    inf_logdet_neumann and inf_logdet_exact_trace within 2e-5 max(1, |ref|_inf); inf_logdet_grad in SERIES, TRACE and
    EXACT mode (d <= 16; SERIES alone above), value at that bound and gradients within 2e-4 of the tensor's max.  EXACT
    at d = 16 runs logdet_pairs_kernel's Gauss-Jordan through all 16 pivots: the value must be finite (its sign path
    returns NaN for a negative determinant; det(I + J) > 0 for a contraction) and match torch.logdet in fp64."""
    seq, seqd, net, x, eps = _fc_setup(name, monkeypatch=monkeypatch)
    d, n = x.shape[1], FC_NETS[name][6]
    co, nco = series_coeff(n), neumann_coeff(n)
    chain = fc_chain(name)[:n]
    dots, _ = term_dots(chain, eps.cpu())
    S = (torch.tensor(co.astype(np.float64)).unsqueeze(1) * dots).sum(0)
    w = eps.double().cpu() + (torch.tensor(nco[1:].astype(np.float64)).view(-1, 1, 1) * chain).sum(0)
    got, tags = e_series(net, x, eps, co)
    _fc_series_tag_ok(name, tags)
    _close_sum(got, S, name + ' series')
    got, tags = e_series_pair(net, net, x, x.flip(0).contiguous(), eps, eps.flip(0).contiguous(), co)
    _fc_series_tag_ok(name, tags)
    _close_sum(got[0], S, name + ' series_pair[0]')
    _close_sum(got[1], S.flip(0), name + ' series_pair[1]')
    got, _ = e_neumann(net, x, eps, nco)
    _close_sum(got, w, name + ' neumann')
    ref64 = copy.deepcopy(seq).double()
    x64 = x.double().cpu().requires_grad_(True)
    wj = torch.autograd.grad(ref64(x64), x64, w)[0]
    got, _ = e_logdet_neumann(net, x, eps, nco)
    _close_sum(got, (wj * eps.double().cpu()).sum(1), name + ' logdet_neumann')
    g = inputs((x.shape[0],), 78, 1.0).to(DEV)
    modes = [('series', netgrad.LOGDET_SERIES, eps, co)]
    if d <= 16:
        tr, _ = _trace_refs(ref_jacobian(seq, x), n)
        cot = co.copy()
        cot[0] = 1.0
        got, _ = e_exact_trace(net, x, cot)
        _close_sum(got, (torch.tensor(cot.astype(np.float64)).unsqueeze(1) * tr).sum(0), name + ' exact_trace')
        modes += [('trace', netgrad.LOGDET_TRACE, None, cot), ('exact', netgrad.LOGDET_EXACT, None, None)]
    for label, mode, e, c in modes:
        got = _logdet_grads(net, seqd, x, mode, e, c, g)
        ref = _grad_ref(seq, x, mode, e, c, g)
        _close_sum(got[0], ref[0], '%s grad %s value' % (name, label))
        r = Ratios('%s grad %s gradients (sum)' % (name, label))
        _check_grads(r, 0, GRAD_TOL, seq, seqd, got, ref)
        r.check()
