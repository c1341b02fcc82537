"""The fc kernels at the feature counts and depths they accept, not only POWER's 6-128x4-6 and the toy 2-128-128-2.

The fused fc kernels (fcnet.hip, fcnet_h3.hip) take 1 <= d <= 16 and 2 to 8 layers with 128-wide hidden layers:
launch_fcnet_h3 has instantiations for d = 2, 6, 8 and for run-time d, fcnet.hip one run-time-d forward kernel.  Their
fused Jacobian exists for d = 2 and 6 only: at every other d the log-det takes the generic forward-mode path
(init_tangents_kernel, fwdmode_act_kernel, logdet_small_kernel / trace_series_kernel).  Nets with other hidden widths,
or d > 16, run on the generic GEMM path.

  * net level: inf_net_forward, inf_net_vjp, inf_logdet_exact and inf_logdet_exact_trace against an fp64 evaluation of
    the same net, in both arithmetics of the fused kernels, with test_gpu_fcblock.py::test_fc_f16x3_error_at_fp32_level's
    bounds; workspace and LDS NaN-filled before every call, the kernels that ran read from the launch profile;
  * block level: whole flows of such blocks against the oracle with test_power_bench_batch_matches_oracle's tolerances.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.density import tabular_logpx
from lib.layers import set_probe_mode
from oracle import inflow_oracle as orc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_TRACE = 10
TRACE_CO = np.array([(-1) ** (k + 1) / k for k in range(1, N_TRACE + 1)], dtype=np.float32)


def _arch(**kw):
    return dict(syn.POWER, **kw)


def _model(arch, B):
    sd = syn.make_state_dict(arch, 0)
    m = build_flow(arch, B)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV).eval(), sd


def _fp64_net(sd, prefix, layout_net, coeff):
    """The net in fp64 from the state dict: the oracle's Lipschitz-normalised weights, its Sin and Swish, torch's ELU."""
    sd64 = {k: (t.double() if t.is_floating_point() else t) for k, t in sd.items()}
    ops = []
    for j, layer in enumerate(layout_net):
        key = '%s.%d' % (prefix, j)
        if layer[0] == 'linear':
            W, b = orc.induced_norm_weight(sd64, key, coeff), sd64[key + '.bias']
            ops.append(lambda t, W=W, b=b: F.linear(t, W, b))
        elif layer[0] == 'swish':
            ops.append(lambda t, beta=sd64[key + '.beta']: orc.swish(t, beta))
        else:
            ops.append({'sin': orc.sin_act, 'elu': F.elu}[layer[0]])

    def net(t):
        for op in ops:
            t = op(t)
        return t
    return net


def _fp64_reference(sd, info, coeff, x, v):
    """y, v^T J, log|det(I + J)| and tr(J) + sum_{k >= 2} TRACE_CO[k - 1] tr(J^k), all in fp64."""
    ref = _fp64_net(sd, 'chain.0.nnet_x', info['net'], coeff)
    x64 = x.double().requires_grad_(True)
    y = ref(x64)
    g = torch.autograd.grad(y, x64, v.double())[0]
    J = torch.func.vmap(torch.func.jacrev(lambda t: ref(t.unsqueeze(0)).squeeze(0)))(x.double())
    ld = torch.logdet(torch.eye(x.shape[1], dtype=torch.float64) + J)
    tr, Jk = torch.zeros(x.shape[0], dtype=torch.float64), None
    for k in range(1, N_TRACE + 1):
        Jk = J if Jk is None else torch.bmm(J, Jk)
        tr = tr + (1.0 if k == 1 else float(TRACE_CO[k - 1])) * Jk.diagonal(dim1=1, dim2=2).sum(1)
    return y.detach(), g, ld, tr


def _engine_calls(net, xd, vd, jacobian=True):
    """The four engine calls on `net`, workspace and LDS NaN-filled before each.  Returns the outputs (the log-det calls'
    status instead of a tensor when they decline) and the launch-profile tags of the forward and of the log-dets."""
    lib = net.lib
    B, d = xd.shape
    stream = _hip.stream_of(xd)
    net.refresh_if_needed(stream)
    ws = torch.empty(net.ws_bytes(B), dtype=torch.uint8, device=DEV)

    def poison():
        ws.fill_(255)
        _hip.check(lib.inf_debug_poison_lds(stream), 'poison_lds')
    y, g = torch.empty_like(xd), torch.empty_like(xd)
    ld, tr = torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    poison()
    _hip.profile_begin(1000)
    try:
        _hip.check(lib.inf_net_forward(net.handle, _hip.ptr(xd), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream),
                   'forward')
        torch.cuda.synchronize()
    finally:
        fwd_tags = {s_['tag'] for s_ in _hip.profile_end()}
    poison()
    _hip.check(lib.inf_net_vjp(net.handle, _hip.ptr(xd), _hip.ptr(vd), _hip.ptr(g), B, _hip.ptr(ws), ws.numel(),
                               stream), 'vjp')
    poison()
    _hip.profile_begin(1000)
    try:
        rc_ld = lib.inf_logdet_exact(net.handle, _hip.ptr(xd), _hip.ptr(ld), B, _hip.ptr(ws), ws.numel(), stream)
        poison()
        rc_tr = lib.inf_logdet_exact_trace(net.handle, _hip.ptr(xd), TRACE_CO.ctypes.data_as(
            ctypes.POINTER(ctypes.c_float)), N_TRACE, _hip.ptr(tr), B, _hip.ptr(ws), ws.numel(), stream)
        torch.cuda.synchronize()
    finally:
        jac_tags = {s_['tag'] for s_ in _hip.profile_end()}
    if jacobian:
        _hip.check(rc_ld, 'logdet_exact')
        _hip.check(rc_tr, 'logdet_exact_trace')
        return (y, g, ld, tr), fwd_tags, jac_tags
    return (y, g, rc_ld, rc_tr), fwd_tags, jac_tags


def _rel(a, r):
    a = a.double().cpu()
    assert torch.isfinite(a).all()
    return (a - r).abs().max().item() / max(1.0, r.abs().max().item())


def _errors(arch, B, monkeypatch):
    """Errors against fp64 (forward, VJP, log-det, exact-trace series) relative to max(1, max|ref|) of the fused kernels
    in exact fp32 MFMA (0) and f16x3 (2) and of the generic per-layer path ('generic', INFLOW_NO_FUSED=1)."""
    m, sd = _model(arch, B)
    blk = imblocks(m)[0]
    d = arch['d']
    info = syn.fc_flow_layout(arch)[0][1]
    x = syn.tabular_batch(B, d, seed=31) * 0.8
    v = syn.tabular_batch(B, d, seed=32)
    refs = _fp64_reference(sd, info, arch['coeff'], x, v)
    xd, vd = x.to(DEV), v.to(DEV)
    err, tags = {}, {}
    for mode in (0, 2, 'generic'):
        monkeypatch.setenv('INFLOW_NO_FUSED', '1' if mode == 'generic' else '0')
        net = _hip.NativeNet(_hip.net_entries(blk.nnet_x), (d,), xd.device)      # fresh: reads INFLOW_NO_FUSED
        if mode != 'generic':
            _hip.check(net.lib.inf_net_set_mfma(net.handle, mode), 'set_mfma')
            assert net.lib.inf_net_get_mfma(net.handle) == mode
        outs, fwd_tags, jac_tags = _engine_calls(net, xd, vd)
        err[mode] = tuple(_rel(a, r) for a, r in zip(outs, refs))
        tags[mode] = (fwd_tags, jac_tags)
        del net
    print('d %d dims %s %s B %d: max error vs fp64 (forward, vjp, log-det, trace series): f32 %s  f16x3 %s  generic %s'
          % (d, arch['dims'], arch['act'], B, *['(%s)' % ', '.join('%.2e' % e for e in err[k]) for k in (0, 2, 'generic')]))
    return err, tags


FUSED_NETS = {
    'd1': _arch(d=1), 'd3': _arch(d=3), 'd8': _arch(d=8), 'd10': _arch(d=10), 'd11': _arch(d=11), 'd16': _arch(d=16),
    'swish_d8': _arch(d=8, act='swish'), 'elu_d5': _arch(d=5, act='elu'),
    'l2_d8': _arch(d=8, dims=[128]), 'l8_d8': _arch(d=8, dims=[128] * 7),
}
FUSED_CASES = [(k, 257) for k in FUSED_NETS] + [('d8', 1), ('d8', 49)]


@pytest.mark.parametrize('name,B', FUSED_CASES, ids=['%s-B%d' % c for c in FUSED_CASES])
def test_fused_fc_sizes_error_at_fp32_level(name, B, monkeypatch):
    """Sin nets at d = 1, 3, 8, 10, 11, 16 with four 128-wide hidden layers, Swish at d = 8, ELU at d = 5, 2 and 8
    layers (FC_MAXL) at d = 8; B = 257, and B = 1 and 49 for the tails of the 48-sample forward and 16-sample Jacobian
    workgroups.  Every error relative to max(1, max|ref|) within 2e-6, and the f16x3 kernels' within 2x the exact fp32
    kernels' + 2e-7.  The forward must have run the fused kernel (tag 600) and the log-dets the generic forward-mode
    Jacobian (no tag 601: these d have no fused Jacobian); the generic path is measured beside them and held to the same
    2e-6.  Measured on an MI355X, largest over the cases: forward 7.0e-8 (f16x3; fp32 4.5e-8, generic 1.2e-7), VJP
    1.8e-7, log-det 9.5e-7 (d = 16; it grows with d: 6e-8 at d = 1, 5e-7 at d = 8), trace series 7.7e-8.  The 8-layer
    net stays at 2.4e-8 / 2.5e-9 / 4.6e-7 / 1.7e-9, so no case needs a bound above 2e-6."""
    arch = dict(FUSED_NETS[name], n_blocks=1)
    err, tags = _errors(arch, B, monkeypatch)
    for mode in (0, 2):
        assert 600 in tags[mode][0], sorted(tags[mode][0])
        assert not tags[mode][1] & {600, 601, 602}, sorted(tags[mode][1])
    assert not (tags['generic'][0] | tags['generic'][1]) & {600, 601, 602}
    for e32, e3, eg in zip(err[0], err[2], err['generic']):
        assert e32 <= 2e-6 and e3 <= 2e-6 and eg <= 2e-6, err
        assert e3 <= 2.0 * e32 + 2e-7, err


def test_other_hidden_widths_take_the_generic_path(monkeypatch):
    """dims = [100, 72] at d = 5: hidden widths that are no multiple of the GEMM tiles and not the fused kernels' 128.
    No fused kernel runs (tag 600 absent) and all four results are within 2e-6 of fp64."""
    arch = _arch(d=5, dims=[100, 72], n_blocks=1)
    err, tags = _errors(arch, 257, monkeypatch)
    for mode in (0, 2, 'generic'):
        assert not (tags[mode][0] | tags[mode][1]) & {600, 601, 602}, sorted(tags[mode][0])
        assert all(e <= 2e-6 for e in err[mode]), err


def test_d17_forward_runs_generic_and_logdets_are_declined():
    """d = 17 is past FC_DMAX: inf_net_forward runs on the generic path and matches fp64 within 2e-6 (the VJP too);
    inf_logdet_exact and inf_logdet_exact_trace return INF_ERR_UNSUPPORTED and launch nothing."""
    arch = _arch(d=17, n_blocks=1)
    B = 257
    m, sd = _model(arch, B)
    blk = imblocks(m)[0]
    info = syn.fc_flow_layout(arch)[0][1]
    x = syn.tabular_batch(B, 17, seed=31) * 0.8
    v = syn.tabular_batch(B, 17, seed=32)
    ref = _fp64_net(sd, 'chain.0.nnet_x', info['net'], arch['coeff'])
    x64 = x.double().requires_grad_(True)
    y_ref = ref(x64)
    g_ref = torch.autograd.grad(y_ref, x64, v.double())[0]
    net = _hip.native_net(blk.nnet_x, (17,), torch.device(DEV))
    (y, g, rc_ld, rc_tr), fwd_tags, jac_tags = _engine_calls(net, x.to(DEV), v.to(DEV), jacobian=False)
    assert 600 not in fwd_tags and fwd_tags, sorted(fwd_tags)
    assert rc_ld == _hip.INF_ERR_UNSUPPORTED and rc_tr == _hip.INF_ERR_UNSUPPORTED
    assert not jac_tags, sorted(jac_tags)
    e = (_rel(y, y_ref.detach()), _rel(g, g_ref))
    print('d 17: max error vs fp64 (forward, vjp) %.2e %.2e' % e)
    assert e[0] <= 2e-6 and e[1] <= 2e-6


# ---- whole blocks against the oracle ----------------------------------------------------------------------------------

BLOCK_CASES = {
    # the DD = 8 forward kernel with the fused Broyden update, the generic Jacobian on the d <= 10 exact branch
    'd8': (_arch(d=8, n_blocks=3), None),
    'd8_f32': (_arch(d=8, n_blocks=3), 'f32'),
    # run-time d, 2 layers
    'd3_l2': (_arch(d=3, dims=[128], n_blocks=3), None),
    # d > 10: the power series with the reference's probe stream
    'd11_series': (_arch(d=11, n_blocks=2), None),
}


@pytest.mark.parametrize('name', list(BLOCK_CASES))
def test_fc_blocks_match_oracle(name, monkeypatch):
    """Flows of fc imBlocks at d = 8, d = 3 with 2-layer nets and d = 11 (B = 257) against the oracle on the same
    inputs, seeds and probes: the Broyden step count of every block exact, nats within 1e-5, per-sample log p within
    2e-4.  d8_f32: the exact fp32 MFMA kernels (INFLOW_MFMA=f32) instead of the default f16x3."""
    arch, mfma = BLOCK_CASES[name]
    if mfma:
        monkeypatch.setenv('INFLOW_MFMA', mfma)
    else:
        monkeypatch.delenv('INFLOW_MFMA', raising=False)
    B, seed = 257, 3
    xc = syn.tabular_batch(B, arch['d'], seed=11)
    m, sd = _model(arch, B)
    set_probe_mode('reference')
    np.random.seed(seed)
    torch.manual_seed(seed)
    xd = xc.to(DEV)
    _hip.check(_hip.load().inf_debug_poison_lds(_hip.stream_of(xd)), 'poison_lds')
    _hip.profile_begin(50000)
    try:
        loss, logpx, z = tabular_logpx(m, xd)
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    print(name, 'tags', sorted(tags))
    nets = [n for b in imblocks(m) for net in (b.nnet_x, b.nnet_z) for n in net.__dict__.get('_inf_native', {}).values()]
    assert nets and all(n.lib.inf_net_get_mfma(n.handle) == (0 if mfma else 2) for n in nets)
    assert 600 in tags, sorted(tags)                       # the fused forward kernel
    assert not tags & {601, 602, 610}, sorted(tags)        # no fused Jacobian and no block kernel at these d
    flow = orc.build(arch, sd, syn.fc_flow_layout(arch))
    rec = []
    prev = orc.broyden

    def broyden(*a, **k):
        r = prev(*a, **k)
        rec.append(r['nstep'])
        return r
    orc.broyden = broyden
    try:
        np.random.seed(seed)
        torch.manual_seed(seed)
        ref_loss, ref_logpx, ref_z = orc.tabular_nats(flow, xc)
    finally:
        orc.broyden = prev
    steps = [b.last_broyden['nstep'] for b in imblocks(m)]
    print('%s: steps %s ref %s  nats %.8f ref %.8f  max |dlogp| %.3g' % (
        name, steps, rec, loss.item(), float(ref_loss),
        np.abs(logpx.view(-1).cpu().numpy() - ref_logpx.view(-1).numpy()).max()))
    assert steps == rec
    assert abs(loss.item() - float(ref_loss)) <= 1e-5
    np.testing.assert_allclose(logpx.view(-1).cpu().numpy(), ref_logpx.view(-1).numpy(), rtol=0, atol=2e-4)
