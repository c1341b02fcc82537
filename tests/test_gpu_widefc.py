"""Fully connected nets with more than 32 input features on the engine.

Such nets run the generic GEMM chain with the wide output stage (out_stage.hip fc_out_wide_kernel: a grid over feature
chunks of 1024 and sample blocks, per-chunk fp64 partials), and their Broyden state stays feature-major (d, B): the
update kernels for d > 32 (broyden_fused_kernel, broyden_p1..p4, br_sum_chunks) reach it through their strides.

  * net level: inf_net_forward and inf_net_vjp against an fp64 evaluation of the same net, beside torch's own fp32
    evaluation on the GPU;
  * root solve: inf_root_find against an fp64 fixed-point solution, the update kernels read from the launch profile;
    the per-sample rule against batches of one; the line search against lib.layers.solvers.broyden(ls=True);
  * flows: the fc_end / fc image flows and the d = 43 and d = 63 tabular flows against the reference's own results
    (tests/golden/make_golden_widefc.py);
  * d <= 32 takes the kernels it took before, and the exact log-dets stay declined past d = 16.

The workspace and every CU's LDS are NaN-filled before every direct engine call and before every module-level run
(RootFind, an imBlock, a flow: the shared workspace buffers, _poison_shared)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.density import tabular_logpx
from lib.layers import RootFind, imBlock, set_probe_mode, solvers
from oracle import inflow_oracle as orc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CH = 1024                       # out_stage.hip OUT_CH / broyden.hip BR_CH


def _arch(d, act='sin', **kw):
    return dict(syn.POWER, d=d, dims=[128, 128], n_blocks=1, act=act, **kw)


def _layout(arch, preact):
    net = list(syn.fc_flow_layout(arch)[0][1]['net'])
    return ([(arch['act'],)] if preact else []) + net


def _block(arch, preact=False):
    """One imBlock over d features (128 x 2 hidden) with deterministic weights, optionally with a leading activation
    (FCNet's preact), and its state dict."""
    from lib.implicit_flow import ACT_FNS
    from lib.layers import base as base_layers
    net = _layout(arch, preact)
    sd = {}
    for name in ('nnet_x', 'nnet_z'):
        syn._net_entries(sd, name, net, None, 0, 30)

    def build():
        mods = []
        for layer in net:
            if layer[0] == 'linear':
                mods.append(base_layers.get_linear(layer[1], layer[2], coeff=arch['coeff'], n_iterations=None,
                                                   atol=1e-3, rtol=1e-3, domain=2, codomain=2))
            else:
                mods.append(ACT_FNS[layer[0]](False))
        return torch.nn.Sequential(*mods)
    blk = imBlock(build(), build(), n_dist='geometric', brute_force=False, neumann_grad=False, grad_in_forward=False,
                  eps_forward=arch['eps_forward'])
    blk.load_state_dict(sd, strict=False)
    missing = [k for k in blk.state_dict() if k.startswith(('nnet_x.', 'nnet_z.')) and k not in sd]
    assert not missing, missing
    return blk.to(DEV).eval(), sd, net


def _ref_net(sd, prefix, layout_net, coeff, dtype, device='cpu'):
    """The net from the state dict in `dtype`: the oracle's Lipschitz-normalised weights, its Sin and Swish, torch's
    ELU (test_gpu_fc_sizes.py::_fp64_net)."""
    sdt = {k: (t.to(dtype) if t.is_floating_point() else t) for k, t in sd.items()}
    ops = []
    for j, layer in enumerate(layout_net):
        key = '%s.%d' % (prefix, j)
        if layer[0] == 'linear':          # (the oracle normalises on the CPU, in `dtype`)
            W, b = orc.induced_norm_weight(sdt, key, coeff).to(device), sdt[key + '.bias'].to(device)
            ops.append(lambda t, W=W, b=b: F.linear(t, W, b))
        elif layer[0] == 'swish':
            ops.append(lambda t, beta=sdt[key + '.beta'].to(device): orc.swish(t, beta))
        else:
            ops.append({'sin': orc.sin_act, 'elu': F.elu}[layer[0]])

    def net(t):
        for op in ops:
            t = op(t)
        return t
    return net


def _fwd_vjp(net, x, v):
    xr = x.detach().clone().requires_grad_(True)
    y = net(xr)
    return y.detach(), torch.autograd.grad(y, xr, v)[0]


def _poison(ws, stream):
    ws.fill_(255)
    _hip.check(_hip.load().inf_debug_poison_lds(stream), 'poison_lds')


def _poison_shared(nbytes=1 << 26):
    """NaN-fill the shared workspace buffers the module-level calls (RootFind, imBlock, a whole flow) take -- the
    current stream's, grown to `nbytes` first, and every other cached one -- and the LDS.  (A flow makes many engine
    calls on that buffer: the first finds NaN, the later ones what the earlier ones left.)"""
    ws = _hip.workspace(torch.device(DEV), nbytes)
    for buf in _hip._ws.values():
        buf.fill_(255)
    _poison(ws, _hip.stream_of(ws))


def _rel(a, r):
    a = a.double().cpu()
    assert torch.isfinite(a).all()
    return (a - r).abs().max().item() / max(1.0, r.abs().max().item())


# ---- net level --------------------------------------------------------------------------------------------------------

NET_CASES = ([('sin', d, B) for d in (33, 43) for B in (257, 49, 1)] +
             [('sin', d, 5) for d in (63, 1024, 1025, 3072, 4097)] +
             [('swish_pre', 43, 49), ('elu', 43, 49), ('elu_pre', 43, 49)])


@pytest.mark.parametrize('kind,d,B', NET_CASES, ids=['%s-d%d-B%d' % c for c in NET_CASES])
def test_wide_net_forward_and_vjp_against_fp64(kind, d, B):
    """inf_net_forward and inf_net_vjp of d-128-128-d nets against fp64, relative to max(1, max|ref|): d = 33 (first
    past the narrow kernels), the tabular widths 43 and 63, the 1024 / 1025 chunk edge, 3072 (3 chunks), 4097 (5
    chunks); B = 257, 49 and 1 at d = 33 and 43 (several sample blocks, a block narrower than a wave, one column), 5
    elsewhere; Sin, and at d = 43 Swish with a leading Swish, ELU, and ELU with a leading ELU (the VJP's
    leading-activation derivative).  The engine must be within 4x the error of torch's own fp32 evaluation of the
    same net on the GPU + 2e-7 (the accumulation orders differ), and within the GEMM path's 2e-6.  The forward must
    have run the wide output stage (tag 950) and no fused fc kernel.
    Measured on an MI355X (engine | torch fp32): forward 6.8e-8 | 7.9e-8 at d = 33, 7.6e-8 | 6.0e-8 at 43, 8.5e-8 |
    5.6e-8 at 1024, 9.1e-8 | 5.1e-8 at 1025, 1.4e-7 | 7.0e-8 at 3072, 1.5e-7 | 6.9e-8 at 4097; VJP 1.7e-7 | 1.5e-7,
    1.5e-7 | 1.6e-7, 3.8e-7 | 1.9e-7, 2.9e-7 | 1.6e-7, 3.9e-7 | 2.7e-7, 4.0e-7 | 2.1e-7; Swish with a leading Swish
    2.6e-8 / 3.6e-8, ELU 1.2e-7 / 1.5e-7.  The largest engine error is 4.0e-7 (the VJP at K = 4097) and the engine is at
    most 2.1x torch's error, so 2e-6 holds everywhere with a factor of five to spare (table in DESIGN.md §17)."""
    act, preact = kind.split('_')[0], kind.endswith('_pre')
    arch = _arch(d, act)
    blk, sd, layout = _block(arch, preact)
    x = syn.tabular_batch(B, d, seed=31) * 0.8
    v = syn.tabular_batch(B, d, seed=32)
    y64, g64 = _fwd_vjp(_ref_net(sd, 'nnet_x', layout, arch['coeff'], torch.float64), x.double(), v.double())
    xd, vd = x.to(DEV), v.to(DEV)
    y32, g32 = _fwd_vjp(_ref_net(sd, 'nnet_x', layout, arch['coeff'], torch.float32, DEV), xd, vd)
    e_torch = (_rel(y32, y64), _rel(g32, g64))

    net = _hip.native_net(blk.nnet_x, (d,), torch.device(DEV))
    lib, stream = net.lib, _hip.stream_of(xd)
    net.refresh_if_needed(stream)
    ws = torch.empty(net.ws_bytes(B), dtype=torch.uint8, device=DEV)
    y, g = torch.empty_like(xd), torch.empty_like(xd)
    _poison(ws, stream)
    _hip.profile_begin(1000)
    try:
        _hip.check(lib.inf_net_forward(net.handle, _hip.ptr(xd), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream),
                   'forward')
        torch.cuda.synchronize()
    finally:
        fwd_tags = {s_['tag'] for s_ in _hip.profile_end()}
    _poison(ws, stream)
    _hip.profile_begin(1000)
    try:
        _hip.check(lib.inf_net_vjp(net.handle, _hip.ptr(xd), _hip.ptr(vd), _hip.ptr(g), B, _hip.ptr(ws), ws.numel(),
                                   stream), 'vjp')
        torch.cuda.synchronize()
    finally:
        vjp_tags = {s_['tag'] for s_ in _hip.profile_end()}
    e = (_rel(y, y64), _rel(g, g64))
    print('WIDEFC net %s d %d B %d: forward engine %.3e torch %.3e | vjp engine %.3e torch %.3e' % (
        kind, d, B, e[0], e_torch[0], e[1], e_torch[1]))
    assert 950 in fwd_tags and 954 in vjp_tags and not (fwd_tags | vjp_tags) & {600, 601, 602}, (fwd_tags, vjp_tags)
    for a, t in zip(e, e_torch):
        assert a <= 4.0 * t + 2e-7, (e, e_torch)
        assert a <= 2e-6, (e, e_torch)


# ---- root solve -------------------------------------------------------------------------------------------------------

def _fixed_point64(sd, layout, coeff, x):
    """z with z + f_z(z) = x + f_x(x) in fp64 (the Banach iteration z <- x_embed - f_z(z); the nets contract)."""
    fx = _ref_net(sd, 'nnet_x', layout, coeff, torch.float64)
    fz = _ref_net(sd, 'nnet_z', layout, coeff, torch.float64)
    x64 = x.double()
    xemb = fx(x64) + x64
    z = x64.clone()
    for _ in range(5000):
        zn = xemb - fz(z)
        if (zn - z).abs().max().item() < 1e-14:
            z = zn
            break
        z = zn
    else:
        raise AssertionError('the fp64 fixed-point iteration did not settle')
    return z, xemb, fz


def _update_tags(d):
    nchunk = (d + CH - 1) // CH
    if nchunk <= 4:
        return {716}
    return {710, 711, 712, 713} | ({714} if nchunk >= 32 else set())


ROOT_CASES = [(33, 2), (1025, 2), (4097, 2), (32769, 2)]


@pytest.mark.parametrize('d,B', ROOT_CASES, ids=['d%d' % c[0] for c in ROOT_CASES])
def test_wide_root_find_against_fp64_fixed_point(d, B):
    """inf_root_find on one block at d = 33 and 1025 (broyden_fused_kernel, 1 and 2 chunks), 4097 (broyden_p1..p4, 5
    chunks) and 32 769 (33 chunks: br_sum_chunks in between), B = 2, eps 1e-5: the fp64 residual of the returned z at
    or below eps sqrt(B d), z within 2e-5 max(1, |z|) of the fp64 fixed point, and the launch profile showing exactly
    the size's update kernels, the wide residual stage (952) and, past one chunk, the partial reduction (705)."""
    arch = _arch(d)
    blk, sd, layout = _block(arch)
    x = syn.tabular_batch(B, d, seed=11)
    z64, xemb64, fz64 = _fixed_point64(sd, layout, arch['coeff'], x)
    eps, T = 1e-5, 30
    xd = x.to(DEV)
    nf = _hip.native_net(blk.nnet_z, (d,), torch.device(DEV))
    _poison_shared(nf.ws_bytes(B, T))
    _hip.profile_begin(5000)
    try:
        z = RootFind.apply(blk.nnet_z, blk.nnet_x, xd, xd, 'broyden', eps, T)
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    st = RootFind.last
    zc = z.double().cpu()
    resid = (xemb64 - fz64(zc) - zc).norm().item()
    bound = eps * np.sqrt(B * d)
    err = (zc - z64).abs().max().item() / max(1.0, z64.abs().max().item())
    print('WIDEFC root d %d: nstep %d lowest %d diff %.3e fp64 residual %.3e bound %.3e z err %.3e tags %s' % (
        d, st['nstep'], st['lowest_step'], st['diff'], resid, bound, err, sorted(tags)))
    assert not st['prot_break'] and st['nstep'] >= 2
    assert st['diff'] <= bound and resid <= bound
    assert err <= 2e-5
    assert tags & {710, 711, 712, 713, 714, 715, 716} == _update_tags(d), sorted(tags)
    # one chunk per sample (d <= 1024): the chunk partial is the sample's sum and is read back directly
    assert 952 in tags and (705 in tags) == (d > CH) and not tags & {600, 701, 702}, sorted(tags)


def test_wide_per_sample_rule_equals_batches_of_one():
    """The per-sample rule at d = 43, B = 4 (samples scaled to stop at different steps): each sample's nstep and
    lowest_step, and z within 2e-5 max(1, |z|), equal the four B = 1 runs under the global rule."""
    d, B = 43, 4
    arch = _arch(d)
    blk, sd, layout = _block(arch)
    x = syn.tabular_batch(B, d, seed=12)
    x[1] *= 0.05
    x[2] *= 3.0
    xd = x.to(DEV)
    nz = _hip.native_net(blk.nnet_z, (d,), torch.device(DEV))
    blk.convergence = 'per_sample'
    _poison_shared(nz.ws_bytes(B, int(blk.threshold)))
    with torch.no_grad():
        z = blk(xd)
    st = dict(blk.last_broyden)
    blk.convergence = 'global'
    singles, steps, lows = [], [], []
    for b in range(B):
        _poison_shared(nz.ws_bytes(1, int(blk.threshold)))
        with torch.no_grad():
            singles.append(blk(xd[b:b + 1]))
        assert blk.last_broyden['convergence'] == 'global'
        steps.append(blk.last_broyden['nstep'])
        lows.append(blk.last_broyden['lowest_step'])
    z1 = torch.cat(singles).double().cpu()
    err = (z.double().cpu() - z1).abs().max().item() / max(1.0, z1.abs().max().item())
    print('WIDEFC per-sample d 43: sample_nstep %s singles %s z err %.3e' % (st['sample_nstep'], steps, err))
    assert st['convergence'] == 'per_sample'
    assert st['sample_nstep'] == steps and st['sample_lowest_step'] == lows
    assert len(set(steps)) > 1, steps
    assert err <= 2e-5


def test_wide_line_search_matches_function_level_broyden():
    """INF_OPT_LINE_SEARCH at d = 43 (B = 16): nstep, tnstep and lowest_step equal lib.layers.solvers.broyden(ls=True)
    on the same block, the roots within 2e-5."""
    d, B = 43, 16
    arch = _arch(d)
    blk, sd, layout = _block(arch)
    xd = syn.tabular_batch(B, d, seed=13).to(DEV)
    eps, T = 1e-5, 30
    _poison_shared()
    with torch.no_grad():
        x_embed = blk.nnet_x(xd) + xd
        r = solvers.broyden(lambda z: x_embed - blk.nnet_z(z) - z, torch.zeros_like(xd), T, eps, ls=True)
    nf = _hip.native_net(blk.nnet_z, (d,), torch.device(DEV))
    _poison_shared(nf.ws_bytes(B, T))
    RootFind.line_search = True
    try:
        z = RootFind.apply(blk.nnet_z, blk.nnet_x, xd, xd, 'broyden', eps, T)
        torch.cuda.synchronize()
    finally:
        RootFind.line_search = False
    st = RootFind.last
    print('WIDEFC line search d 43: engine nstep %d tnstep %d lowest %d | function level %d %d %d' % (
        st['nstep'], st['tnstep'], st['lowest_step'], r['nstep'], r['tnstep'], r['lowest_step']))
    assert not st['prot_break'] and not r['prot_break']
    assert (st['nstep'], st['tnstep'], st['lowest_step']) == (r['nstep'], r['tnstep'], r['lowest_step'])
    ref = r['result'].double().cpu()
    assert (z.double().cpu() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


def test_wide_banach_find_root():
    """inf_banach_find_root (find_fixed_point from z0 = x) at d = 1025, both rules: within 2e-5 of the fp64 fixed
    point (eps 1e-12: the iteration stops once (dz)^2 < eps (1 + |x|) for every element, i.e. |dz| < 1e-6)."""
    d, B = 1025, 3
    arch = _arch(d)
    blk, sd, layout = _block(arch)
    x = syn.tabular_batch(B, d, seed=14)
    z64, _, _ = _fixed_point64(sd, layout, arch['coeff'], x)
    xd = x.to(DEV)
    nf = _hip.native_net(blk.nnet_z, (d,), torch.device(DEV))
    for rule in ('global', 'per_sample'):
        nf.set_option(_hip.INF_OPT_CONVERGENCE, _hip.CONVERGENCE[rule])
        _poison_shared(nf.ws_bytes(B))
        z = RootFind.apply(blk.nnet_z, blk.nnet_x, xd, xd, 'banach', 1e-12, 200)
        err = (z.double().cpu() - z64).abs().max().item() / max(1.0, z64.abs().max().item())
        print('WIDEFC banach d 1025 %s: iters %d err %.3e' % (rule, RootFind.last['fixed_point_iters'], err))
        assert 0 < RootFind.last['fixed_point_iters'] <= 200
        assert err <= 2e-5
    nf.set_option(_hip.INF_OPT_CONVERGENCE, _hip.INF_CONV_GLOBAL)


# ---- unchanged below the limit, still declined above FC_DMAX ----------------------------------------------------------

def _root_tags(d, B=64):
    arch = _arch(d)
    blk, sd, layout = _block(arch)
    xd = syn.tabular_batch(B, d, seed=11).to(DEV)
    _poison_shared()
    _hip.profile_begin(5000)
    try:
        RootFind.apply(blk.nnet_z, blk.nnet_x, xd, xd, 'broyden', 1e-5, 30)
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    assert RootFind.last['nstep'] >= 2
    return tags


# The launch-profile tags of one root solve (6-128-128-6 and 32-128-128-32 Sin blocks, B = 64) on the parent commit
PARENT_TAGS_D6 = {600, 702}
PARENT_TAGS_D32 = {702, 715, 1412001, 2222061}


def test_narrow_nets_take_the_kernels_they_took():
    """d = 6 and d = 32 show exactly the parent's launch-profile tags: the fused forward (600) with its folded update
    at d = 6; the generic GEMMs (1412001, 2222061), the one-launch start (702) and broyden_small_kernel (715) at
    d = 32; no wide output stage (95x), no chunked update (710-714, 716), no partial reduction (705).  The literals were
    read from the parent commit's library with this file's _root_tags."""
    t6, t32 = _root_tags(6), _root_tags(32)
    print('WIDEFC narrow tags d6 %s d32 %s' % (sorted(t6), sorted(t32)))
    assert t6 == PARENT_TAGS_D6, sorted(t6)
    assert t32 == PARENT_TAGS_D32, sorted(t32)
    assert 600 in t6 and 715 in t32


def test_exact_logdets_stay_declined_at_d43():
    """inf_logdet_exact, inf_logdet_exact_trace and inf_logdet_grad return INF_ERR_UNSUPPORTED at d = 43 and launch
    nothing."""
    d, B = 43, 8
    blk, sd, layout = _block(_arch(d))
    xd = syn.tabular_batch(B, d, seed=31).to(DEV)
    net = _hip.native_net(blk.nnet_x, (d,), torch.device(DEV))
    lib, stream = net.lib, _hip.stream_of(xd)
    net.refresh_if_needed(stream)
    torch.cuda.synchronize()
    ws = torch.empty(net.ws_bytes(B), dtype=torch.uint8, device=DEV)
    out = torch.empty(B, device=DEV)
    co = np.array([1.0, -0.5], dtype=np.float32)
    carr = co.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    L = len([l for l in layout if l[0] == 'linear'])
    none = (ctypes.c_void_p * L)(*([None] * L))
    gr = _hip.NetGrads(none, none, none, None)
    _hip.profile_begin(100)
    try:
        rc = [lib.inf_logdet_exact(net.handle, _hip.ptr(xd), _hip.ptr(out), B, _hip.ptr(ws), ws.numel(), stream),
              lib.inf_logdet_exact_trace(net.handle, _hip.ptr(xd), carr, 2, _hip.ptr(out), B, _hip.ptr(ws),
                                         ws.numel(), stream),
              lib.inf_logdet_grad(net.handle, _hip.ptr(xd), 1, None, None, 0, None, _hip.ptr(out), None,
                                  ctypes.byref(gr), B, _hip.ptr(ws), ws.numel(), stream)]
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    assert rc == [_hip.INF_ERR_UNSUPPORTED] * 3, rc
    assert not tags, sorted(tags)


def test_workspace_bytes_at_d196608_do_not_wrap():
    """inf_workspace_bytes of a 196 608-128-196 608 net (CelebA-HQ 256 flattened) at B = 128, T = 30 against the carve
    arithmetic in Python integers: past 2^32 bytes, so a 32-bit product anywhere would show.  Nothing is allocated
    beyond the net itself; no forward-mode tangent buffers are carved above d = 16."""
    d, B, T, hid = 196608, 128, 30, 128
    from lib.layers import base as base_layers
    from lib.layers.base.nonlin import Sin
    with torch.device(DEV):
        seq = torch.nn.Sequential(base_layers.get_linear(d, hid, coeff=0.99, n_iterations=None, atol=1e-3, rtol=1e-3,
                                                         domain=2, codomain=2), Sin(),
                                  base_layers.get_linear(hid, d, coeff=0.99, n_iterations=None, atol=1e-3, rtol=1e-3,
                                                         domain=2, codomain=2))
    net = _hip.NativeNet(_hip.net_entries(seq), (d,), torch.device(DEV))

    def expect(B, T):
        off = 0

        def take(n, size=4):
            nonlocal off
            off = (off + 255) & ~255
            off += n * size
        E, nchunk = B * d, (d + CH - 1) // CH
        take(B * hid), take(B * hid), take(B * d)                 # h0, h1, Y
        take(B * hid)                                             # D[0]
        for _ in range(21):
            take(E)
        take(T * E), take(T * E)                                  # U, VT
        take(B * nchunk * 128, 8)                                 # part (SERIES_MAX slabs)
        take(B * nchunk * (3 * T + 2) + 64, 8)                    # bpart
        take(B + 1, 8), take(64), take(B * (8 + T), 8), take(B), take(B)
        return off
    got = net.ws_bytes(B, T)
    # the fcblock exchange words depend on fcblock_grid(B): bound them instead of restating the kernel's grid rule
    lo = expect(B, T)
    print('WIDEFC workspace d 196608 B 128 T 30: %d bytes (vectors and partials alone: %d)' % (got, lo))
    assert got > 2 ** 32
    assert lo <= got <= lo + (1 << 20), (got, lo)
    assert net.ws_bytes(B, 1) < got
    # ext0 / ext1 of the forward-mode Jacobian would be 2 x (d + 1) B d floats here: far beyond what is reported
    assert got < 2 * (d + 1) * B * d * 4


# ---- whole flows against the reference's own results (tests/golden/make_golden_widefc.py) ----------------------------

def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def _flow(arch, g, B, train=False):
    m = build_flow(arch, B)
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


FLOW_FIXTURES = [('fcend_small_b4', 'fcend_small'), ('fc_img_small_b4', 'fc_img_small'),
                 ('tab_d43_b64', 'tab_d43'), ('tab_d63_b64', 'tab_d63')]


@pytest.mark.parametrize('name,arch_name', FLOW_FIXTURES)
def test_wide_flow_matches_reference_fixture(golden_dir, name, arch_name):
    """ImplicitFlow(fc_end=True) and ImplicitFlow(fc=True) on 3 x 8 x 8 (fc blocks over d = 192, ActNorm1d, squeeze) and
    the tabular flows at d = 43 and d = 63 in eval, at test_gpu_acts.py::_check_flow's tolerances: per block nstep /
    lowest_step / series length exact, z within 2e-5 max(1, |z|), log-det within 2e-3 nats; log p within 2e-3 nats,
    the loss within 1e-5.  The wide residual and VJP stages (952, 954) must have run."""
    from test_gpu_acts import _check_flow
    from lib.density import image_logpx
    g = _golden(golden_dir, name)
    arch = syn.CONFIGS[arch_name]
    x = torch.from_numpy(g['x']).to(DEV)
    m = _flow(arch, g, x.shape[0])
    tags = set()

    def run():
        _poison_shared()
        _hip.profile_begin(50000)
        try:
            out = image_logpx(m, x, arch['nvals']) if arch['kind'] == 'conv' else tabular_logpx(m, x)
            torch.cuda.synchronize()
        finally:
            tags.update(s_['tag'] for s_ in _hip.profile_end())
        return out
    _check_flow(m, g, run)
    assert {952, 954} <= tags, sorted(tags)


def test_wide_implicit_backward_against_fp64_solve():
    """inf_imblock_backward at d = 43 and d = 1025 (B = 3; the wide VJP stage and the chunked residual of the backward
    solve, fc_out_wide_kernel modes 954 / 955): dl_dh with dl_dh (I + J_fz(z)) = grad and dl_dx = dl_dh (I + J_fx(x))
    against the fp64 solution with the fp64 Jacobians, within 2e-5 max(1, |ref|) (the project's bound for a
    solved vector; the solve runs to eps_backward = 1e-10 or its 30 steps and returns the lowest iterate)."""
    lib = _hip.load()
    for d in (43, 1025):
        B, T = 3, 30
        arch = _arch(d)
        blk, sd, layout = _block(arch)
        x = syn.tabular_batch(B, d, seed=21)
        z = syn.tabular_batch(B, d, seed=22)
        grad = syn.tabular_batch(B, d, seed=23)
        fx = _ref_net(sd, 'nnet_x', layout, arch['coeff'], torch.float64)
        fz = _ref_net(sd, 'nnet_z', layout, arch['coeff'], torch.float64)
        jac = lambda f, t: torch.func.vmap(torch.func.jacrev(lambda u: f(u.unsqueeze(0)).squeeze(0)))(t.double())
        eye = torch.eye(d, dtype=torch.float64)
        Jz, Jx = jac(fz, z) + eye, jac(fx, x) + eye
        # dl_dh (I + J_fz) = grad by the fp64 iteration h <- grad - h J_fz (|J_fz| < 1; products only)
        g64, Jf = grad.double(), Jz - eye
        h64 = g64.clone()
        for _ in range(5000):
            hn = g64 - torch.einsum('bi,bij->bj', h64, Jf)
            done = (hn - h64).abs().max().item() < 1e-14
            h64 = hn
            if done:
                break
        else:
            raise AssertionError('the fp64 iteration did not settle')
        dx64 = torch.einsum('bi,bij->bj', h64, Jx)
        nx = _hip.native_net(blk.nnet_x, (d,), torch.device(DEV))
        nz = _hip.native_net(blk.nnet_z, (d,), torch.device(DEV))
        xd, zd, gd = x.to(DEV), z.to(DEV), grad.to(DEV)
        stream = _hip.stream_of(xd)
        for n in (nx, nz):
            n.refresh_if_needed(stream)
        ws = torch.empty(max(nz.ws_bytes(B, T), nx.ws_bytes(B, 1)), dtype=torch.uint8, device=DEV)
        dl_dh, dl_dx = torch.empty_like(gd), torch.empty_like(gd)
        st = _hip.BroydenStats()
        _poison(ws, stream)
        _hip.profile_begin(5000)
        try:
            _hip.check(lib.inf_imblock_backward(nx.handle, nz.handle, _hip.ptr(zd), _hip.ptr(xd), _hip.ptr(gd),
                                                _hip.ptr(dl_dh), _hip.ptr(dl_dx), B, T, 1e-10, ctypes.byref(st),
                                                _hip.ptr(ws), ws.numel(), stream), 'inf_imblock_backward')
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        e = (_rel(dl_dh, h64), _rel(dl_dx, dx64))
        print('WIDEFC backward d %d: nstep %d lowest %d diff %.3e | dl_dh err %.3e dl_dx err %.3e' % (
            d, st.nstep, st.lowest_step, st.diff, e[0], e[1]))
        assert {954, 955} <= tags and 716 in tags and (705 in tags) == (d > CH), sorted(tags)
        assert e[0] <= 2e-5 and e[1] <= 2e-5, e


def test_fc_end_inverse_matches_reference(golden_dir):
    """fcend_small_inverse_b4: ImplicitFlow.inverse(z, logpz) in eval.  Every block's root solve (in the order the
    inverse visits them) nstep / lowest_step and series lengths exact, x within 2e-5 max(1, |x|), the returned
    log-density term within 2e-3 nats."""
    g = _golden(golden_dir, 'fcend_small_inverse_b4')
    arch = syn.CONFIGS['fcend_small']
    z = torch.from_numpy(g['z']).to(DEV)
    B = z.shape[0]
    m = _flow(arch, g, B)
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    _poison_shared()
    n_ps = []                                   # both series lengths of every block, in the order they are drawn
    plan = imBlock._series_plan

    def series_plan(self):
        r = plan(self)
        n_ps.append(int(r[0]))
        return r
    imBlock._series_plan = series_plan
    try:
        with torch.no_grad():
            x, logpx = m.inverse(z, torch.zeros(B, 1, device=DEV))
    finally:
        imBlock._series_plan = plan
    torch.cuda.synchronize()
    blocks = list(reversed(imblocks(m)))
    assert len(blocks) == int(g['nblocks'])
    for i, b in enumerate(blocks):
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'solve %d nstep' % i
        assert b.last_broyden['lowest_step'] == int(g['b%d_lowest_step' % i]), 'solve %d lowest_step' % i
        assert int(b.last_broyden['prot_break']) == int(g['b%d_prot_break' % i]) == 0
        # one draw per block serves both branches here; the reference draws once too and records the length per branch
        assert [n_ps[i], n_ps[i]] == [int(v) for v in g['b%d_n_power_series' % i]], 'solve %d n_ps' % i
    assert len(n_ps) == len(blocks)
    xr = torch.from_numpy(g['x']).double()
    err = (x.reshape(B, -1).double().cpu() - xr).abs().max().item()
    print('WIDEFC inverse: max |dx| %.3e (|x| max %.3g), max |dlogp| %.3e' % (
        err, xr.abs().max().item(), np.abs(logpx.view(-1).cpu().numpy() - g['logpx']).max()))
    assert err <= 2e-5 * max(1.0, xr.abs().max().item())
    np.testing.assert_allclose(logpx.view(-1).cpu().numpy(), g['logpx'], rtol=0, atol=2e-3)


@pytest.mark.parametrize('d', [43, 1025])
def test_wide_param_grad_against_fp64_autograd(d):
    """inf_net_param_grad (the recompute graph's backward) on d-128-128-d Sin nets at d = 43 and 1025, B = 5: every
    weight and bias gradient (through the Lipschitz normalisation) and the x-gradient within 2e-4 of the tensor's max
    of fp64 autograd on the CPU, tests/test_gpu_fcgrad.py's nets, reference and bound."""
    from test_gpu_fcgrad import _eval64, _net, _params64
    from lib.layers import netgrad
    from lib.layers.base import Sin
    B = 5
    net = _net(d, 128, Sin, seed=5)
    x = syn.tabular_batch(B, d, seed=41) * 0.5
    gout = syn.tabular_batch(B, d, seed=42)
    swaps = _params64(net)
    x64 = x.double().requires_grad_(True)
    (_eval64(net, x64, swaps) * gout.double()).sum().backward()
    net = net.to(DEV)
    native = _hip.native_net(net, (d,), torch.device(DEV))
    native.refresh_if_needed(_hip.stream_of(x.to(DEV)))
    _poison_shared(int(native.lib.inf_grad_workspace_bytes(native.handle, B)))
    res = netgrad.param_grads(native, net, x.to(DEV), gout.to(DEV), want_x=True)
    assert res is not None
    grads, gx = res
    torch.cuda.synchronize()
    worst = 0.0
    for (p, leaf), q in zip(swaps, [q for m in net for n_ in ('weight', 'bias', 'beta') if hasattr(m, n_)
                                    for q in [getattr(m, n_)]]):
        ref = leaf.grad
        err = (grads[q].double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
        worst = max(worst, err)
    ex = (gx.double().cpu() - x64.grad).abs().max().item() / x64.grad.abs().max().item()
    print('WIDEFC param grad d %d: worst parameter error %.3e, x-gradient %.3e (of the tensor max)' % (d, worst, ex))
    assert worst <= 2e-4 and ex <= 2e-4


def test_fc_end_training_matches_reference(golden_dir):
    """fcend_small_train_b2: one training step's loss.backward() of the fc_end flow (B = 2, train mode).  The fc blocks
    (d = 192) solve forward and backward on the engine (inf_root_find, inf_imblock_backward, inf_neumann_vector on the
    wide path), their nets' parameter gradients, FCWrapper and ActNorm1d go through autograd.  The loss within 1e-5,
    every block's forward nstep and series lengths exact, every parameter gradient at
    test_gpu_train.py::_check_grads' bounds.  The backward solves' step counts are not compared: at eps_backward 1e-10
    they sit at fp32's noise floor and move with the summation order in the reference itself (make_golden_widefc.py);
    the gradients the reference wrote agree between 1 and 8 threads to 1 % of a quarter of these bounds."""
    from test_gpu_train import _check_grads
    from lib.density import image_bits_per_dim_graph
    g = _golden(golden_dir, 'fcend_small_train_b2')
    assert not [k for k in g.files if '_bwd_' in k]
    arch = syn.CONFIGS['fcend_small']
    x = torch.from_numpy(g['x']).to(DEV)
    m = _flow(arch, g, x.shape[0], train=True)
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    _poison_shared()
    _hip.profile_begin(100000)
    try:
        loss, logpx, z = image_bits_per_dim_graph(m, x, arch['nvals'])
        loss.backward()
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    blocks = imblocks(m)
    assert len(blocks) == int(g['nblocks'])
    for i, b in enumerate(blocks):
        assert b.training
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'block %d forward nstep' % i
        assert b.last_n_power_series == int(g['b%d_n_power_series' % i][0]), 'block %d n_ps' % i
        assert not b.last_broyden_backward['prot_break']
    print('WIDEFC train loss %.8f ref %.8f, backward steps %s' % (
        loss.item(), float(g['loss']), [b.last_broyden_backward['nstep'] for b in blocks]))
    # the wide residual and VJP (Neumann vector) stages; the backward solve runs on autograd's thread, outside this
    # thread's launch profile (test_wide_implicit_backward_against_fp64_solve reads its kernels)
    assert {952, 954} <= tags, sorted(tags)
    assert abs(loss.item() - float(g['loss'])) <= 1e-5, (loss.item(), float(g['loss']))
    np.testing.assert_allclose(logpx.detach().view(-1).cpu().numpy(), g['logpx'], rtol=4e-7, atol=2e-3)
    n = _check_grads(m, g)
    assert n == len([k for k in g.files if k.startswith('g:') or k.startswith('gs:')]) >= 80


@pytest.mark.parametrize('d', [43, 1025])
def test_wide_neumann_and_surrogate_against_fp64(d):
    """The training log-det's engine calls on d-128-128-d Sin nets at d = 43 and 1025, B = 5, 8 terms, against fp64
    autograd of the same net (tests/test_gpu_fcgrad.py's nets and reference):
      * inf_neumann_vector and inf_neumann_vector_pair: w = eps + sum_k c_k eps^T J^k within 2e-5 max(1, |w|) (the
        project's bound for a VJP);
      * inf_logdet_neumann: (w^T J) . eps per sample within 2e-3 nats (the project's log-det bound);
      * inf_net_surrogate_grad: the gradients of sum_b w_b^T J(x_b) eps_b with respect to every parameter and x within
        2e-4 of the tensor's max (test_gpu_fcgrad.py's bound)."""
    from test_gpu_fcgrad import _eval64, _net, _params64
    from lib.layers import netgrad
    from lib.layers.base import Sin
    B, K = 5, 8
    net = _net(d, 128, Sin, seed=6)
    x = syn.tabular_batch(B, d, seed=51) * 0.5
    eps = torch.sign(syn.tabular_batch(B, d, seed=52))
    nco = np.array([1.0] + [(-1.0) ** k for k in range(1, K + 1)], dtype=np.float32)
    swaps = _params64(net)
    x64 = x.double().requires_grad_(True)
    y = _eval64(net, x64, swaps)
    e64 = eps.double()
    w64, v = e64.clone(), e64
    for k in range(1, K + 1):
        v = torch.autograd.grad(y, x64, v, retain_graph=True)[0]
        w64 = w64 + float(nco[k]) * v
    gw = torch.autograd.grad(y, x64, w64, create_graph=True)[0]
    ld64 = (gw * e64).sum(1).detach()
    (gw * e64).sum().backward()

    net = net.to(DEV)
    xd, ed = x.to(DEV), eps.to(DEV)
    stream = _hip.stream_of(xd)
    native = _hip.native_net(net, (d,), torch.device(DEV))
    native.refresh_if_needed(stream)
    lib = native.lib
    carr = nco.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ws = torch.empty(2 * native.ws_bytes(B), dtype=torch.uint8, device=DEV)
    w, wa, wb = torch.empty_like(xd), torch.empty_like(xd), torch.empty_like(xd)
    ld = torch.empty(B, device=DEV)
    _poison(ws, stream)
    _hip.check(lib.inf_neumann_vector(native.handle, _hip.ptr(xd), _hip.ptr(ed), carr, K, _hip.ptr(w), B, _hip.ptr(ws),
                                      ws.numel(), stream), 'inf_neumann_vector')
    _poison(ws, stream)
    _hip.check(lib.inf_neumann_vector_pair(native.handle, _hip.ptr(xd), _hip.ptr(ed), native.handle, _hip.ptr(xd),
                                           _hip.ptr(ed), carr, K, _hip.ptr(wa), _hip.ptr(wb), B, _hip.ptr(ws),
                                           ws.numel(), stream), 'inf_neumann_vector_pair')
    _poison(ws, stream)
    _hip.profile_begin(1000)
    try:
        _hip.check(lib.inf_logdet_neumann(native.handle, _hip.ptr(xd), _hip.ptr(ed), carr, K, _hip.ptr(ld), B,
                                          _hip.ptr(ws), ws.numel(), stream), 'inf_logdet_neumann')
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    assert 954 in tags, sorted(tags)
    ew = _rel(w, w64.detach())
    eld = (ld.double().cpu() - ld64).abs().max().item()
    assert torch.equal(wa, w) and torch.equal(wb, w)
    # the surrogate's gradients (fc nets: no per-sample value), with the fp32 w the engine made
    ng, keep, grads = netgrad._alloc(net)
    gx = torch.empty_like(xd)
    gws = torch.empty(int(lib.inf_grad_workspace_bytes(native.handle, B)), dtype=torch.uint8, device=DEV)
    _poison(gws, stream)
    _hip.check(lib.inf_net_surrogate_grad(native.handle, _hip.ptr(xd), _hip.ptr(w), _hip.ptr(ed), None, _hip.ptr(gx),
                                          ctypes.byref(ng), B, _hip.ptr(gws), gws.numel(), stream),
               'inf_net_surrogate_grad')
    torch.cuda.synchronize()
    params = [getattr(m_, n_) for m_ in net for n_ in ('weight', 'bias', 'beta') if hasattr(m_, n_)]
    # (the last bias does not enter J: autograd leaves its gradient unset, the engine writes zeros)
    refs = [leaf.grad if leaf.grad is not None else torch.zeros_like(leaf) for _, leaf in swaps]
    assert sum(1 for _, leaf in swaps if leaf.grad is None) == 1
    worst = max((grads[q].double().cpu() - r).abs().max().item() / max(r.abs().max().item(), 1e-12)
                for r, q in zip(refs, params))
    ex = (gx.double().cpu() - x64.grad).abs().max().item() / x64.grad.abs().max().item()
    print('WIDEFC neumann d %d: w err %.3e, logdet_neumann |d| %.3e nats (max |ref| %.3g), surrogate parameter error '
          '%.3e, x-gradient %.3e' % (d, ew, eld, ld64.abs().max().item(), worst, ex))
    assert ew <= 2e-5 and eld <= 2e-3
    assert worst <= 2e-4 and ex <= 2e-4
