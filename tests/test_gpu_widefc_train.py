"""Training gradients of fc nets wider than 16 features on the engine.

inf_logdet_grad(INF_LOGDET_SERIES) above d = 16 builds its bilinear pairs without a Jacobian: a_j = (J^T)^j eps by the
VJP chain, b_m = J^m eps by a forward-tangent chain over the per-layer GEMMs, stacked by series_pairs_wide_kernel (launch
profile tag 722), then the forward-over-reverse pass every width shares.  imBlock._engine_grads accepts such nets, so a
wide tabular flow's training step takes the recompute gradient and the series' gradient from the engine.

  * inf_logdet_grad against fp64 autograd on the CPU (tests/test_gpu_fcgrad.py's nets and 2e-4 bound), the reference
    built Jacobian-free from repeated autograd.grad(..., create_graph=True);
  * the d = 16 / d = 17 boundary, read from the launch profile;
  * the workspace size, its refusal and its independence of what the workspace held;
  * one imBlock's loss.backward() on the engine route against the autograd route;
  * the d = 43 tabular flow's training step against the reference's own (tests/golden/make_golden_widetrain.py);
  * the fc layout's weight-gradient contraction (grad.hip wgrad_fc_kernel, tag 891) through inf_net_param_grad.

The launch profile is per host thread and autograd runs a backward on its own, so where the gradients are taken in the
backward pass the tests read the tags through _grad_call_tags, which brackets netgrad.logdet_grads on the thread that
calls it.  The shared workspace and the LDS are NaN-filled before every run (test_gpu_widefc.py's _poison_shared)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.density import tabular_nats_graph
from lib.layers import imBlock, netgrad, set_probe_mode
from lib.layers.base import Sin, Swish, get_linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAIR_TAG = 722                  # series_pairs_wide_kernel
INF_ERR_WORKSPACE = 3           # include/inflow.h InfStatus


def _deep_net(d, hidden, act, seed):
    """test_gpu_fcgrad._net's recipe with any number of hidden layers (train_tabular.py's --dims 128-128-128-128)."""
    torch.manual_seed(seed)
    lin = lambda a, b: get_linear(a, b, coeff=0.97, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    dims = [d] + list(hidden) + [d]
    mods = []
    for i in range(len(dims) - 1):
        mods.append(lin(dims[i], dims[i + 1]))
        if i + 2 < len(dims):
            mods.append(act())
    net = torch.nn.Sequential(*mods)
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, 'compute_weight'):
                m.weight.mul_(2.0)
                m.bias.normal_(0, 0.1)
            if isinstance(m, Swish):
                m.beta.fill_(0.7)
        net(torch.zeros(1, d))
    return net


def _series_ref(net, x, eps, coeff, g):
    """S_b = sum_k coeff[k-1] eps^T J^k eps and the gradients of sum_b g_b S_b in fp64 on the CPU, without a Jacobian:
    eps^T J^k by repeated autograd.grad(y, x, v, create_graph=True) (basic_logdet_estimator, implicit_block.py:418-426)."""
    from test_gpu_fcgrad import _eval64, _params64
    swaps = _params64(net)
    x64 = x.detach().double().requires_grad_(True)
    y = _eval64(net, x64, swaps)
    e = eps.detach().double()
    v, S = e, torch.zeros(x.shape[0], dtype=torch.float64)
    for k in range(1, len(coeff) + 1):
        v = torch.autograd.grad(y, x64, v, create_graph=True)[0]
        S = S + float(coeff[k - 1]) * (v * e).sum(1)
    leaves = [x64] + [t for _, t in swaps]
    grads = torch.autograd.grad((S * g.double()).sum(), leaves, allow_unused=True)
    grads = [gr if gr is not None else torch.zeros_like(t) for gr, t in zip(grads, leaves)]
    return S.detach(), grads[0], {p: gr for (p, _), gr in zip(swaps, grads[1:])}


def _inputs(d, B, n_terms, seed):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32) * 0.5)
    eps = torch.from_numpy(rng.integers(0, 2, (B, d)).astype(np.float32) * 2 - 1)
    coeff = np.array([(-1) ** (k + 1) / k * (1.3 if k > 2 else 1.0) for k in range(1, n_terms + 1)], dtype=np.float32)
    g = torch.from_numpy(rng.standard_normal(B).astype(np.float32))
    g[0] = -g[0].abs() - 0.25              # negative entries, and one exact zero
    g[B // 2] = 0.0
    return x, eps, coeff, g


def _native(net, d):
    netd = net.to(DEV)
    native = _hip.native_net(netd, (d,), torch.device(DEV))
    native.refresh_if_needed(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return netd, native


def _engine_series(net, d, x, eps, coeff, g):
    """netgrad.logdet_grads(LOGDET_SERIES) on a NaN-filled workspace -> (result or None, launch-profile tags)."""
    from test_gpu_widefc import _poison_shared
    netd, native = _native(net, d)
    need = int(native.lib.inf_logdet_grad_workspace_bytes(native.handle, x.shape[0], netgrad.LOGDET_SERIES, len(coeff)))
    _poison_shared(max(need, 1 << 20))
    _hip.profile_begin(20000)
    try:
        res = netgrad.logdet_grads(native, netd, x.to(DEV), netgrad.LOGDET_SERIES, eps.to(DEV), coeff, g.to(DEV))
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    return res, tags


def _check_series(net, d, B, n_terms, seed, what):
    from test_gpu_fcgrad import _close
    x, eps, coeff, g = _inputs(d, B, n_terms, seed)
    S_ref, gx_ref, gp_ref = _series_ref(net, x, eps, coeff, g)
    res, tags = _engine_series(net, d, x, eps, coeff, g)
    assert res is not None, '%s: inf_logdet_grad declined the net' % what
    value, grads, gx = res
    rel = lambda got, ref: (got.detach().double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
    print('WIDETRAIN %s: value %.3e gx %.3e worst parameter %.3e (of the tensor max)' % (
        what, rel(value, S_ref), rel(gx, gx_ref), max(rel(grads[p], r) for p, r in gp_ref.items())))
    _close(value, S_ref, 'value')
    _close(gx, gx_ref, 'x')
    for p, ref in gp_ref.items():
        _close(grads[p], ref, 'param %s' % (tuple(p.shape),))
    return tags


# ---- A1: inf_logdet_grad SERIES against fp64 autograd ------------------------------------------------------------------

SERIES_CASES = [(17, 5, 1, Sin), (17, 8, 4, Swish), (43, 5, 3, Sin), (43, 33, 5, Swish), (1025, 3, 2, Sin)]


@pytest.mark.parametrize('d,B,n_terms,act', SERIES_CASES,
                         ids=['d%d-B%d-n%d-%s' % (c[0], c[1], c[2], c[3].__name__) for c in SERIES_CASES])
def test_wide_series_grad_against_fp64_autograd(d, B, n_terms, act):
    """d-128-128-d nets: d = 17 with one term (one pair, no chain step) and with n B = 32 columns on Swish (the aligned
    column count, the beta gradients); d = 43 with n B = 15 (every tail) and 165; d = 1025 (the chunked output stage of
    the VJP chain).  The value, the x-gradient and every weight, bias and beta gradient within 2e-4 of the tensor's max
    of fp64 autograd (test_gpu_fcgrad._close); the pair kernel ran."""
    from test_gpu_fcgrad import _net
    tags = _check_series(_net(d, 128, act, seed=3 + d), d, B, n_terms, 11 + d, 'd %d B %d n %d %s' % (
        d, B, n_terms, act.__name__))
    assert PAIR_TAG in tags, sorted(tags)


def test_wide_series_grad_five_layer_net():
    """d = 43 with four hidden layers (train_tabular.py's 128-128-128-128): the chains' ping-pong buffers over a
    five-layer net, B = 5, 3 terms, Sin, at the same bound."""
    tags = _check_series(_deep_net(43, [128] * 4, Sin, seed=9), 43, 5, 3, 17, 'd 43 five layers')
    assert PAIR_TAG in tags, sorted(tags)


# ---- A2: the boundary ---------------------------------------------------------------------------------------------------

def test_series_grad_boundary_d16_d17():
    """d = 16 keeps the Jacobian route (no pair-kernel launch), d = 17 is the first width on the chains; both within
    the bound (B = 5, 3 terms, Sin)."""
    from test_gpu_fcgrad import _net
    t16 = _check_series(_net(16, 128, Sin, seed=19), 16, 5, 3, 27, 'd 16')
    t17 = _check_series(_net(17, 128, Sin, seed=20), 17, 5, 3, 28, 'd 17')
    assert PAIR_TAG not in t16, sorted(t16)
    assert PAIR_TAG in t17, sorted(t17)


# ---- A3: the workspace --------------------------------------------------------------------------------------------------

def test_wide_series_grad_workspace():
    """The size inf_logdet_grad_workspace_bytes reports succeeds; 256 bytes fewer is INF_ERR_WORKSPACE with an empty
    launch profile; two runs on a NaN-filled workspace give the same bits (d = 43, B = 5, 3 terms)."""
    from test_gpu_fcgrad import _net
    from test_gpu_widefc import _poison
    d, B, n_terms = 43, 5, 3
    x, eps, coeff, g = _inputs(d, B, n_terms, 31)
    netd, native = _native(_net(d, 128, Sin, seed=21), d)
    lib = native.lib
    xd, ed, gd = x.to(DEV), eps.to(DEV), g.to(DEV)
    stream = _hip.stream_of(xd)
    carr = coeff.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    need = int(lib.inf_logdet_grad_workspace_bytes(native.handle, B, netgrad.LOGDET_SERIES, n_terms))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def run(nbytes):
        ng, keep, grads = netgrad._alloc(netd)
        value, gx = torch.empty(B, device=DEV), torch.empty_like(xd)
        _poison(ws, stream)
        _hip.profile_begin(20000)
        try:
            rc = lib.inf_logdet_grad(native.handle, _hip.ptr(xd), netgrad.LOGDET_SERIES, _hip.ptr(ed), carr, n_terms,
                                     _hip.ptr(gd), _hip.ptr(value), _hip.ptr(gx), ctypes.byref(ng), B, _hip.ptr(ws),
                                     nbytes, stream)
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        return rc, tags, [value, gx] + [grads[p] for p in netd.parameters()]
    rc, tags, _ = run(need - 256)
    assert rc == INF_ERR_WORKSPACE and not tags, (rc, sorted(tags))
    rc1, tags1, out1 = run(need)
    rc2, _, out2 = run(need)
    assert rc1 == 0 and rc2 == 0 and PAIR_TAG in tags1, (rc1, rc2, sorted(tags1))
    for a, b in zip(out1, out2):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


# ---- A4: block level ----------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _grad_call_tags(tags, calls):
    """Brackets every netgrad.logdet_grads call in a launch-profile session on the thread that makes it."""
    real = netgrad.logdet_grads

    def spy(*a, **k):
        calls.append(1)
        _hip.profile_begin(20000)
        try:
            out = real(*a, **k)
            torch.cuda.synchronize()
        finally:
            tags.update(s_['tag'] for s_ in _hip.profile_end())
        return out
    netgrad.logdet_grads = spy
    try:
        yield
    finally:
        netgrad.logdet_grads = real


def _block_step(blk, x, seed):
    """One loss and backward() of a training imBlock -> (loss, {name: grad}, x-gradient, tags, logdet_grads calls)."""
    from test_gpu_widefc import _poison_shared
    for p in blk.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    set_probe_mode('reference')
    np.random.seed(seed)
    torch.manual_seed(seed)
    _poison_shared()
    tags, calls = set(), []
    with _grad_call_tags(tags, calls):
        z, delta = blk(xg, torch.zeros(x.shape[0], 1, device=DEV))
        logpx = (-0.5 * np.log(2 * np.pi) - z.pow(2) / 2).sum(1, keepdim=True) - delta
        loss = -torch.mean(logpx)
        loss.backward()
        torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in blk.named_parameters() if p.grad is not None}
    return loss.item(), grads, xg.grad.detach().clone(), tags, len(calls)


class _Fixture(dict):
    files = property(lambda self: list(self))


@pytest.mark.parametrize('grad_in_forward', [False, True], ids=['backward', 'grad_in_forward'])
def test_wide_block_engine_route_against_autograd_route(grad_in_forward):
    """One imBlock over 43-128-128-43 Sin nn.Sequential nets, B = 16, train mode, neumann_grad=False: loss and
    backward() on the engine route (the recompute and the series' gradients from the engine; the pair kernel ran)
    against the same block on the autograd route (_engine_grads_ok_fc forced False), same seeds: the loss within 1e-5,
    every parameter gradient and the input gradient at test_gpu_train._check_grads' bounds.  With exact_trace=True the
    block keeps the autograd branch at this width: no raise, no pair-kernel launch."""
    from test_gpu_train import _check_grads
    from test_gpu_widefc import _arch, _block
    d, B = 43, 16
    blk, sd, layout = _block(_arch(d))
    blk.train()
    blk.neumann_grad, blk.grad_in_forward = False, grad_in_forward
    x = (syn.tabular_batch(B, d, seed=61) * 0.8).to(DEV)
    blk.__dict__.pop('_engine_grads_ok_fc', None)
    assert blk._engine_grads(x) is True
    loss_e, grads_e, gx_e, tags_e, calls_e = _block_step(blk, x, seed=7)
    n_ps = blk.last_n_power_series
    blk.__dict__['_engine_grads_ok_fc'] = False
    loss_a, grads_a, gx_a, tags_a, calls_a = _block_step(blk, x, seed=7)
    assert blk.last_n_power_series == n_ps
    print('WIDETRAIN block grad_in_forward %s: loss engine %.8f autograd %.8f, series length %d' % (
        grad_in_forward, loss_e, loss_a, n_ps))
    assert calls_e == 2 and PAIR_TAG in tags_e, (calls_e, sorted(tags_e))
    assert calls_a == 0
    assert abs(loss_e - loss_a) <= 1e-5, (loss_e, loss_a)
    assert set(grads_e) == set(grads_a)
    ref = _Fixture({'g:' + n: t.cpu().numpy().ravel() for n, t in grads_a.items()})
    for n, p in blk.named_parameters():
        p.grad = grads_e.get(n)
    assert _check_grads(blk, ref) == len(grads_a) >= 10
    scale = gx_a.abs().max().item()
    assert (gx_e - gx_a).abs().max().item() <= 2e-3 * scale + 1e-9
    # exact_trace=True: the engine's exact-trace gradient needs the Jacobian (d <= 16), so the log-det takes the
    # autograd branch while the recompute stays on the engine; against the same block wholly on autograd
    blk.exact_trace = True
    try:
        blk.__dict__['_engine_grads_ok_fc'] = True
        loss_t, grads_t, gx_t, tags_t, calls_t = _block_step(blk, x, seed=7)
        blk.__dict__['_engine_grads_ok_fc'] = False
        loss_u, grads_u, gx_u, _, _ = _block_step(blk, x, seed=7)
    finally:
        blk.exact_trace = False
    assert calls_t == 0 and PAIR_TAG not in tags_t
    assert abs(loss_t - loss_u) <= 1e-5, (loss_t, loss_u)
    assert set(grads_t) == set(grads_u)
    ref = _Fixture({'g:' + n: t.cpu().numpy().ravel() for n, t in grads_u.items()})
    for n, p in blk.named_parameters():
        p.grad = grads_t.get(n)
    assert _check_grads(blk, ref) == len(grads_u) >= 10
    assert (gx_t - gx_u).abs().max().item() <= 2e-3 * gx_u.abs().max().item() + 1e-9


# ---- A5: the reference's own training step ------------------------------------------------------------------------------

def test_tab_d43_training_matches_reference(golden_dir):
    """tab_d43_train_b16: one loss.backward() of the d = 43 tabular flow (four imBlocks, the basic series with the
    graph) against the reference's.  Every block's forward nstep and series length exact, the loss within 1e-5, every
    parameter gradient at test_gpu_train._check_grads' bounds, and the series' gradients came from the pair kernel.
    The backward solves' step counts are not in the fixture (make_golden_widetrain.py)."""
    from test_gpu_train import _check_grads
    from test_gpu_widefc import _poison_shared
    g = np.load(os.path.join(golden_dir, 'tab_d43_train_b16.npz'))
    arch = syn.TAB_D43
    x = torch.from_numpy(g['x']).to(DEV)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV).train()
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    _poison_shared()
    tags, calls = set(), []
    with _grad_call_tags(tags, calls):
        loss, logpx, z = tabular_nats_graph(m, x)
        loss.backward()
        torch.cuda.synchronize()
    blocks = imblocks(m)
    assert len(blocks) == int(g['nblocks']) == 4
    for i, b in enumerate(blocks):
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'block %d forward nstep' % i
        assert {b.last_n_power_series} == {int(v) for v in g['b%d_n_power_series' % i]}, 'block %d n_ps' % i
    print('WIDETRAIN tab_d43 loss %.8f ref %.8f, logdet_grads calls %d' % (loss.item(), float(g['loss']), len(calls)))
    assert abs(loss.item() - float(g['loss'])) <= 1e-5, (loss.item(), float(g['loss']))
    n = _check_grads(m, g)
    assert n == len([k for k in g.files if k.startswith('g:') or k.startswith('gs:')]) >= 80
    assert len(calls) == 2 * len(blocks) and PAIR_TAG in tags, (len(calls), sorted(tags))


# ---- A6: the fc weight-gradient contraction ----------------------------------------------------------------------------

FC_TAG, PLAIN_TAG = 891, 890     # wgrad_fc_kernel, wgrad_kernel


def _contraction_cases():
    from test_widefc_train_host import FC_COLUMNS, FC_SHAPES
    return [(d, hid, B) for d, hid in FC_SHAPES for B in FC_COLUMNS]


@pytest.mark.parametrize('d,hidden,B', _contraction_cases(), ids=['d%d-h%d-B%d' % c for c in _contraction_cases()])
def test_fc_contraction_through_param_grad(d, hidden, B):
    """inf_net_param_grad on d-128-128-d Sin nets at d = 17, 43, 1025 with B = 1, 31, 33, 257, 1030 columns (the float4
    tails, both sides of a 32-column chunk, a count that crosses split boundaries): every weight and bias gradient and
    the x-gradient within 2e-4 of the tensor's max of fp64 autograd on the CPU.  Every data term ran wgrad_fc_kernel
    (one launch per layer, tag 891); wgrad_kernel (890) ran only the three P = 1 dsigma/dW calls, the tiled kernels
    not at all.  The inputs are test_widefc_train_host.py's, whose guard shows that a dropped column would show."""
    from test_gpu_fcgrad import _close, _eval64, _params64
    from test_gpu_widefc import _poison_shared
    from test_widefc_train_host import contraction_inputs
    net, x, gout = contraction_inputs(d, hidden, B)
    swaps = _params64(net)
    x64 = x.double().requires_grad_(True)
    (_eval64(net, x64, swaps) * gout.double()).sum().backward()
    netd, native = _native(net, d)
    _poison_shared(max(int(native.lib.inf_grad_workspace_bytes(native.handle, B)), 1 << 20))
    _hip.profile_begin(20000)
    try:
        res = netgrad.param_grads(native, netd, x.to(DEV), gout.to(DEV), want_x=True)
        torch.cuda.synchronize()
    finally:
        launches = {s_['tag']: s_['launches'] for s_ in _hip.profile_end()}
    assert res is not None
    grads, gx = res
    n_layers = sum(1 for m in netd if hasattr(m, 'compute_weight'))
    wg = {t: c for t, c in launches.items() if 800 <= t < 900}
    assert wg == {FC_TAG: n_layers, PLAIN_TAG: n_layers}, wg
    _close(gx, x64.grad, 'x')
    for p, leaf in swaps:
        _close(grads[p], leaf.grad, 'param %s' % (tuple(p.shape),))
