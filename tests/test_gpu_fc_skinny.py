"""The skinny GEMM family of fc nets over more than 32 features (gemm_skinny.hip; INF_OPT_FC_SKINNY).

Every layer of such a net runs on 32 x 32 .. 64 x 64 tiles of exact fp32 MFMA (tag 962); a deep layer with few outputs
splits K into slices whose fp32 partials (960) a second launch sums in slice order in fp64 (961).  Option 0 is the generic
GEMM chain the nets ran before.

  * net level: inf_net_forward / inf_net_vjp against fp64, beside torch's own fp32 evaluation, at the widths, hidden
    widths and batch sizes at which the tiles, the slices and the slab change;
  * the launch profile under both values of the option, and at d = 32;
  * option 0 against option 1, and each bitwise repeatable;
  * the workspace: the slab's size, the exact size succeeding, 256 bytes fewer refused before any launch;
  * a root solve, the gradient chain, and the fc_end flow's reference trajectory under both values.

The workspace and every CU's LDS are NaN-filled before every direct engine call and before every module-level run.  The
helpers restate those of test_gpu_widefc.py / test_gpu_fcgrad.py / test_gpu_acts.py."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.layers import RootFind, imBlock, set_probe_mode
from oracle import inflow_oracle as orc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
INF_MFMA_F32 = 0                # InfMfmaMode (include/inflow.h)
INF_ERR_WORKSPACE = 3           # InfStatus
SKINNY = {960, 961, 962}
SLAB = 512 << 10


def _arch(d, h=128, act='sin'):
    return dict(syn.POWER, d=d, dims=[h, h], n_blocks=1, act=act)


def _block(arch, preact=False, nobias=()):
    """One imBlock over d features (h x 2 hidden) with deterministic weights, optionally with a leading activation and
    with the linear layers at the layout positions `nobias` built without a bias; its state dict and layout."""
    from lib.implicit_flow import ACT_FNS
    from lib.layers import base as base_layers
    net = list(syn.fc_flow_layout(arch)[0][1]['net'])
    net = ([(arch['act'],)] if preact else []) + net
    sd = {}
    for name in ('nnet_x', 'nnet_z'):
        syn._net_entries(sd, name, net, None, 0, 30)
        for j in nobias:
            del sd['%s.%d.bias' % (name, j)]

    def build():
        mods = []
        for j, layer in enumerate(net):
            if layer[0] == 'linear':
                mods.append(base_layers.get_linear(layer[1], layer[2], bias=j not in nobias, coeff=arch['coeff'],
                                                   n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2))
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
    """The net from the state dict in `dtype`: the oracle's Lipschitz-normalised weights, its Sin and Swish, torch's ELU."""
    sdt = {k: (t.to(dtype) if t.is_floating_point() else t) for k, t in sd.items()}
    ops = []
    for j, layer in enumerate(layout_net):
        key = '%s.%d' % (prefix, j)
        if layer[0] == 'linear':
            W = orc.induced_norm_weight(sdt, key, coeff).to(device)
            b = sdt[key + '.bias'].to(device) if key + '.bias' in sdt else None
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
    ws = _hip.workspace(torch.device(DEV), nbytes)
    for buf in _hip._ws.values():
        buf.fill_(255)
    _poison(ws, _hip.stream_of(ws))


def _rel(a, r):
    a = a.double().cpu()
    assert torch.isfinite(a).all()
    return (a - r).abs().max().item() / max(1.0, r.abs().max().item())


# (kind, d, h, B): every d at h = 128, B = 64; every h and every B at d = 1025; the other activations at d = 43, B = 49
D_CASES = [('sin', d, 128, 64) for d in (33, 257, 1025, 3072)]
H_CASES = [('sin', 1025, h, 64) for h in (100, 160)]
B_CASES = [('sin', 1025, 128, B) for B in (1, 5, 65, 1000)] + [('sin', 3072, 128, 200)]
ACT_CASES = [('swish_pre', 43, 128, 49), ('elu_pre', 43, 128, 49), ('sin_nobias', 43, 128, 49)]
NET_CASES = D_CASES + H_CASES + B_CASES + ACT_CASES
AB_CASES = [c for c in NET_CASES if c[1] in (1025, 3072)]
_ids = lambda cases: ['%s-d%d-h%d-B%d' % c for c in cases]


@functools.lru_cache(maxsize=None)
def _case(kind, d, h, B):
    """The case's block, engine net, inputs, fp64 results and torch's fp32 errors: computed once, shared, never
    written."""
    act = kind.split('_')[0]
    arch = _arch(d, h, act)
    # (sin_nobias: the middle linear layer, layout position 2, has no bias)
    blk, sd, layout = _block(arch, kind.endswith('_pre'), nobias=(2,) if kind.endswith('_nobias') else ())
    x = syn.tabular_batch(B, d, seed=31) * 0.8
    v = syn.tabular_batch(B, d, seed=32)
    y64, g64 = _fwd_vjp(_ref_net(sd, 'nnet_x', layout, arch['coeff'], torch.float64), x.double(), v.double())
    xd, vd = x.to(DEV), v.to(DEV)
    y32, g32 = _fwd_vjp(_ref_net(sd, 'nnet_x', layout, arch['coeff'], torch.float32, DEV), xd, vd)
    net = _hip.native_net(blk.nnet_x, (d,), torch.device(DEV))
    net.refresh_if_needed(_hip.stream_of(xd))
    torch.cuda.synchronize()
    return dict(blk=blk, net=net, xd=xd, vd=vd, y64=y64, g64=g64, e_torch=(_rel(y32, y64), _rel(g32, g64)))


def _engine(c, skinny, mode=None, ws_bytes=None, want_rc=False):
    """inf_net_forward and inf_net_vjp of the case's net under INF_OPT_FC_SKINNY = skinny (and an MFMA mode), each on a
    freshly poisoned workspace: (y, g, forward tags, VJP tags); the option and the mode are put back."""
    net, xd, vd = c['net'], c['xd'], c['vd']
    B = xd.shape[0]
    lib, stream = net.lib, _hip.stream_of(xd)
    prev = net.set_option(_hip.INF_OPT_FC_SKINNY, skinny)
    mode0 = lib.inf_net_get_mfma(net.handle)
    if mode is not None:
        _hip.check(lib.inf_net_set_mfma(net.handle, mode), 'set_mfma')
    try:
        ws = torch.empty(net.ws_bytes(B) if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=DEV)
        y, g = torch.empty_like(xd), torch.empty_like(xd)
        tags, rcs = [], []
        for call in ('forward', 'vjp'):
            _poison(ws, stream)
            _hip.profile_begin(1000)
            try:
                if call == 'forward':
                    rc = lib.inf_net_forward(net.handle, _hip.ptr(xd), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream)
                else:
                    rc = lib.inf_net_vjp(net.handle, _hip.ptr(xd), _hip.ptr(vd), _hip.ptr(g), B, _hip.ptr(ws),
                                         ws.numel(), stream)
                torch.cuda.synchronize()
            finally:
                tags.append({s_['tag'] for s_ in _hip.profile_end()})
            rcs.append(rc)
            if not want_rc:
                _hip.check(rc, call)
    finally:
        net.set_option(_hip.INF_OPT_FC_SKINNY, prev)
        _hip.check(lib.inf_net_set_mfma(net.handle, mode0), 'set_mfma')
    return (rcs, tags) if want_rc else (y, g, tags[0], tags[1])


# ---- 1. net level -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', [None, INF_MFMA_F32], ids=['default', 'f32'])
@pytest.mark.parametrize('kind,d,h,B', NET_CASES, ids=_ids(NET_CASES))
def test_skinny_net_forward_and_vjp_against_fp64(kind, d, h, B, mode):
    """d-h-h-d nets on the skinny family against fp64, relative to max(1, max|ref|): d = 33 (first wide width), 257 (a
    slice edge + 1), 1025 (ragged last slice), 3072 (the fc_end shape) at h = 128, B = 64; h = 100 (M and K no multiple
    of 32 / 16) and 160 (a fifth, ragged M tile of the deep layer) and B = 1, 5, 65 (a second N tile of one column), 1000
    (the 64 x 64 tile) at d = 1025; B = 200 at d = 3072 (the 32 x 64 tile); at d = 43, B = 49 Swish with a leading Swish, ELU with a leading ELU, and a Sin net whose middle layer has
    no bias.  Bounds, test_gpu_widefc.py's: at most 4x the error of torch's own fp32 evaluation of the same net + 2e-7,
    and at most 2e-6.  In the net's default MFMA mode and in INF_MFMA_F32 (the family is exact fp32 in both)."""
    c = _case(kind, d, h, B)
    y, g, ft, vt = _engine(c, 1, mode)
    e = (_rel(y, c['y64']), _rel(g, c['g64']))
    print('FCSKINNY net %s d %d h %d B %d mode %s: forward engine %.3e torch %.3e | vjp engine %.3e torch %.3e | tags %s %s'
          % (kind, d, h, B, mode, e[0], c['e_torch'][0], e[1], c['e_torch'][1], sorted(ft), sorted(vt)))
    assert ft & SKINNY and vt & SKINNY and 950 in ft and 954 in vt, (ft, vt)
    for a, t in zip(e, c['e_torch']):
        assert a <= 4.0 * t + 2e-7, (e, c['e_torch'])
        assert a <= 2e-6, (e, c['e_torch'])


# ---- 2. the launch profile ----------------------------------------------------------------------------------------------

def test_skinny_launch_profile():
    """d = 3072, h = 128, B = 64: forward and VJP show the split-K pair (960, 961: the 3072 -> 128 layer and its
    transpose) and the small tile (962: 128 x 128 and 128 -> 3072), and no generic GEMM (tags from 1 000 000); with the
    option at 0 no 96x tag and the generic GEMMs.  At d = 32 no 96x tag under either value."""
    c = _case('sin', 3072, 128, 64)
    _, _, ft, vt = _engine(c, 1)
    for t in (ft, vt):
        assert SKINNY <= t and not [x for x in t if x >= 1000000], sorted(t)
    _, _, ft0, vt0 = _engine(c, 0)
    for t in (ft0, vt0):
        assert not t & set(range(960, 970)) and [x for x in t if x >= 1000000], sorted(t)
    n = _case('sin', 32, 128, 64)
    for value in (0, 1):
        _, _, ft, vt = _engine(n, value)
        assert not (ft | vt) & set(range(960, 970)) and [x for x in ft | vt if x >= 1000000], (sorted(ft), sorted(vt))


# ---- 3. option 0 against option 1 -------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind,d,h,B', AB_CASES, ids=_ids(AB_CASES))
def test_skinny_against_generic_and_repeatable(kind, d, h, B):
    """The d = 1025 and d = 3072 cases under both values of the option: forward and VJP agree within 4e-6 max(1,
    max|ref|) (the sum of the two paths' 2e-6 bounds), and each value's results are bitwise equal over two calls on
    freshly poisoned workspace (no atomics, the partials summed in slice order)."""
    c = _case(kind, d, h, B)
    res = {}
    for value in (0, 1):
        y, g, _, _ = _engine(c, value)
        y2, g2, _, _ = _engine(c, value)
        assert torch.equal(y, y2) and torch.equal(g, g2), value
        res[value] = (y.double().cpu(), g.double().cpu())
    for i, ref in enumerate((c['y64'], c['g64'])):
        diff = (res[0][i] - res[1][i]).abs().max().item() / max(1.0, ref.abs().max().item())
        print('FCSKINNY option 0 vs 1 %s d %d h %d B %d %s: %.3e' % (kind, d, h, B, ('forward', 'vjp')[i], diff))
        assert diff <= 4e-6


# ---- 4. workspace -----------------------------------------------------------------------------------------------------

def test_skinny_workspace():
    """d = 3072, B = 64: inf_workspace_bytes exceeds the vectors-only size by the slab (it is carved whatever the option
    says, so the two values report the same bytes, within 512 KiB + alignment of each other); a forward and a VJP with
    exactly that many bytes succeed; with 256 bytes fewer both return INF_ERR_WORKSPACE and launch nothing."""
    c = _case('sin', 3072, 128, 64)
    net, B = c['net'], 64
    need = net.ws_bytes(B)
    prev = net.set_option(_hip.INF_OPT_FC_SKINNY, 0)
    need0 = net.ws_bytes(B)
    net.set_option(_hip.INF_OPT_FC_SKINNY, prev)
    print('FCSKINNY workspace d 3072 B 64: %d bytes, option 0 %d' % (need, need0))
    assert 0 <= need - need0 <= SLAB + 256
    y, g, ft, vt = _engine(c, 1, ws_bytes=need)
    assert _rel(y, c['y64']) <= 2e-6 and _rel(g, c['g64']) <= 2e-6 and {960, 961} <= ft
    rcs, tags = _engine(c, 1, ws_bytes=need - 256, want_rc=True)
    assert rcs == [INF_ERR_WORKSPACE] * 2 and not tags[0] and not tags[1], (rcs, tags)


# ---- 5. a root solve ----------------------------------------------------------------------------------------------------

def test_skinny_root_find_against_fp64_fixed_point():
    """RootFind on a d = 1025 Sin block at B = 2, eps 1e-5, against the fp64 fixed point of z + f_z(z) = x + f_x(x)
    (test_gpu_widefc.py's construction): z within 2e-5 max(1, |z|), the split-K launches among the tags."""
    d, B = 1025, 2
    arch = _arch(d)
    blk, sd, layout = _block(arch)
    x = syn.tabular_batch(B, d, seed=11)
    fx = _ref_net(sd, 'nnet_x', layout, arch['coeff'], torch.float64)
    fz = _ref_net(sd, 'nnet_z', layout, arch['coeff'], torch.float64)
    x64 = x.double()
    xemb = fx(x64) + x64
    z64 = x64.clone()
    for _ in range(5000):
        zn = xemb - fz(z64)
        done = (zn - z64).abs().max().item() < 1e-14
        z64 = zn
        if done:
            break
    else:
        raise AssertionError('the fp64 fixed-point iteration did not settle')
    xd = x.to(DEV)
    nf = _hip.native_net(blk.nnet_z, (d,), torch.device(DEV))
    _poison_shared(nf.ws_bytes(B, 30))
    _hip.profile_begin(5000)
    try:
        z = RootFind.apply(blk.nnet_z, blk.nnet_x, xd, xd, 'broyden', 1e-5, 30)
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    st = RootFind.last
    err = (z.double().cpu() - z64).abs().max().item() / max(1.0, z64.abs().max().item())
    print('FCSKINNY root d 1025: nstep %d lowest %d z err %.3e tags %s' % (st['nstep'], st['lowest_step'], err,
                                                                          sorted(tags)))
    assert not st['prot_break'] and st['nstep'] >= 2
    assert err <= 2e-5
    assert {960, 961} <= tags and not [t for t in tags if t >= 1000000], sorted(tags)


# ---- 6. the gradient chain ----------------------------------------------------------------------------------------------

def test_skinny_param_grad_against_fp64_autograd():
    """inf_net_param_grad on a 1025-128-128-1025 Sin net at B = 5 (test_gpu_fcgrad.py's nets and reference): every
    weight and bias gradient through the Lipschitz normalisation and the x-gradient within 2e-4 of the tensor's max of
    fp64 autograd; the chain's layer-forward and input-gradient GEMMs ran on the skinny family."""
    from lib.layers import netgrad
    from lib.layers.base import Sin, get_linear
    d, B = 1025, 5
    torch.manual_seed(5)
    lin = lambda a, b: get_linear(a, b, coeff=0.97, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    net = torch.nn.Sequential(lin(d, 128), Sin(), lin(128, 128), Sin(), lin(128, d))
    with torch.no_grad():
        for m in net.modules():
            if hasattr(m, 'compute_weight'):
                m.weight.mul_(2.0)
                m.bias.normal_(0, 0.1)
        net(torch.zeros(1, d))
    swaps = [(getattr(m, name), getattr(m, name).detach().double().requires_grad_(True))
             for m in net for name in ('weight', 'bias') if hasattr(m, name)]
    leaf = {id(p): t for p, t in swaps}

    def eval64(t):
        for m in net:
            if hasattr(m, 'compute_weight'):
                W = leaf[id(m.weight)]
                sigma = torch.dot(m.u.double(), torch.mv(W, m.v.double()))
                factor = torch.max(torch.ones(1, dtype=torch.float64), sigma / m.coeff)
                t = F.linear(t, W / factor, leaf[id(m.bias)])
            else:
                t = torch.sin(2 * np.pi * t) / (2 * np.pi)
        return t
    x = syn.tabular_batch(B, d, seed=41) * 0.5
    gout = syn.tabular_batch(B, d, seed=42)
    x64 = x.double().requires_grad_(True)
    (eval64(x64) * gout.double()).sum().backward()
    net = net.to(DEV)
    native = _hip.native_net(net, (d,), torch.device(DEV))
    native.refresh_if_needed(_hip.stream_of(x.to(DEV)))
    _poison_shared(int(native.lib.inf_grad_workspace_bytes(native.handle, B)))
    _hip.profile_begin(5000)
    try:
        res = netgrad.param_grads(native, net, x.to(DEV), gout.to(DEV), want_x=True)
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    assert res is not None
    grads, gx = res
    params = [getattr(m, n_) for m in net for n_ in ('weight', 'bias') if hasattr(m, n_)]
    worst = max((grads[q].double().cpu() - t.grad).abs().max().item() / max(t.grad.abs().max().item(), 1e-12)
                for (_, t), q in zip(swaps, params))
    ex = (gx.double().cpu() - x64.grad).abs().max().item() / x64.grad.abs().max().item()
    print('FCSKINNY param grad d 1025: worst parameter error %.3e, x-gradient %.3e, tags %s' % (worst, ex, sorted(tags)))
    assert worst <= 2e-4 and ex <= 2e-4
    assert tags & SKINNY and not [t for t in tags if t >= 1000000], sorted(tags)


# ---- 7. one flow ----------------------------------------------------------------------------------------------------------

def _engine_nets(m):
    """Every engine net the flow's modules have created so far (lib._hip's per-module caches)."""
    return [n for mod in m.modules() if isinstance(mod.__dict__.get('_inf_native'), dict)
            for n in mod.__dict__['_inf_native'].values() if isinstance(n, _hip.NativeNet)]


def test_skinny_fc_end_flow_trajectory_under_both_values(golden_dir):
    """fcend_small_b4 (fc blocks over d = 192) with INF_OPT_FC_SKINNY at 1 (the default its nets are created with) and
    then set to 0 on every engine net of the flow: each block's nstep / lowest_step equal between the two runs and equal
    to the reference fixture's, the loss within 1e-5 of the fixture's both times; the skinny tags appear under 1 only."""
    from lib.density import image_logpx
    g = np.load(os.path.join(golden_dir, 'fcend_small_b4.npz'))
    arch = syn.CONFIGS['fcend_small']
    x = torch.from_numpy(g['x']).to(DEV)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV).eval()
    traj = {}
    for value in (1, 0):
        nets = _engine_nets(m)                           # (none before the first run: the nets are created on first use)
        for n in nets:
            n.set_option(_hip.INF_OPT_FC_SKINNY, value)
        set_probe_mode('reference')
        np.random.seed(int(g['seed']))
        torch.manual_seed(int(g['seed']))
        _poison_shared()
        _hip.profile_begin(50000)
        try:
            loss = image_logpx(m, x, arch['nvals'])[0]
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        nets = _engine_nets(m)
        assert len(nets) >= 2 * int(g['nblocks']) and all(n.get_option(_hip.INF_OPT_FC_SKINNY) == value for n in nets)
        blocks = imblocks(m)
        assert len(blocks) == int(g['nblocks'])
        traj[value] = [(b.last_broyden['nstep'], b.last_broyden['lowest_step']) for b in blocks]
        print('FCSKINNY flow fcend_small_b4 option %d: trajectory %s loss %.8f ref %.8f' % (
            value, traj[value], loss.item(), float(g['loss'])))
        assert bool(tags & SKINNY) == bool(value), sorted(tags)
        assert traj[value] == [(int(g['b%d_nstep' % i]), int(g['b%d_lowest_step' % i])) for i in range(len(blocks))]
        assert abs(loss.item() - float(g['loss'])) <= 1e-5
    assert traj[0] == traj[1]


# ---- the option's values ------------------------------------------------------------------------------------------------

def test_option_default_and_range():
    """A new net has INF_OPT_FC_SKINNY = 1; 0 and 1 are accepted and read back, 2 is refused and changes nothing."""
    from lib.layers import base as base_layers
    seq = torch.nn.Sequential(base_layers.get_linear(40, 40, coeff=0.9, n_iterations=None, atol=1e-3, rtol=1e-3,
                                                     domain=2, codomain=2)).to(DEV)
    net = _hip.native_net(seq, (40,), torch.device(DEV))
    assert net.get_option(_hip.INF_OPT_FC_SKINNY) == 1
    assert net.set_option(_hip.INF_OPT_FC_SKINNY, 0) == 1 and net.get_option(_hip.INF_OPT_FC_SKINNY) == 0
    with pytest.raises(_hip.HipError):
        net.set_option(_hip.INF_OPT_FC_SKINNY, 2)
    assert net.get_option(_hip.INF_OPT_FC_SKINNY) == 0
    assert net.set_option(_hip.INF_OPT_FC_SKINNY, 1) == 0
