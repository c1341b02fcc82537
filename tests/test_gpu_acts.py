"""The activation table's other entries (nn.ELU, nn.Softplus, nn.ReLU, LipschitzCube, Identity, Zero) and bias-free
layers on the MI355X engine.  The oracle knows only Swish and Sin, so the references here are fp64 torch evaluations of
the same modules and fixtures from the reference itself (tests/golden/make_golden_acts.py).

Tolerances (the project's, tests/test_gpu_parity.py):
  * net forward / VJP / z:     |delta| <= 2e-5 * max(1, |ref|_inf)
  * fused against generic:     1e-5 * max(1, |ref|_inf)
  * per-sample log p:          |delta| <= 2e-3 nats (plus 2 fp32 ulps of |log p|, which reaches 2e4 nats at 3x32x32)
  * bits/dim, nats per batch:  |delta| <= 1e-5
  * Broyden nstep / lowest_step and the series lengths: exact
Workspace and LDS are filled with NaN before every direct engine call.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, engine_nets, imblocks
from lib.density import image_bits_per_dim_graph, image_logpx, normal_logprob_sum, tabular_logpx
from lib.implicit_flow import ACT_FNS
from lib.layers import imBlock, set_probe_mode
from lib.layers.base import get_conv2d, get_linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NEW_ACTS = ('elu', 'softplus', 'relu', 'lcube', 'identity', 'zero')


def _close(a, b, rel=2e-5):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    print('max abs err %.3e (bound %.3e)' % (err, rel * scale))
    assert torch.isfinite(a).all()
    assert err <= rel * scale, 'max abs err %g > %g' % (err, rel * scale)


def _conv(a, b, k, bias=True, coeff=0.9):
    return get_conv2d(a, b, k, 1, k // 2, coeff=coeff, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2,
                      bias=bias)


def _lin(a, b, coeff=0.99):
    return get_linear(a, b, coeff=coeff, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)


def _engine(seq, shape, x, v, mfma=None, series=0, k128=None):
    """inf_net_forward, inf_net_vjp and (series > 0) a `series`-term inf_logdet_series of a fresh engine net of `seq`,
    NaN-poisoned workspace and LDS before every call.  Returns (y, g, ld or None, launch-profile tags)."""
    B = x.shape[0]
    net = _hip.NativeNet(_hip.net_entries(seq), shape, x.device)      # fresh: reads INFLOW_NO_FUSED / INFLOW_MFMA
    if mfma is not None:
        _hip.check(net.lib.inf_net_set_mfma(net.handle, mfma), 'set_mfma')
    if k128 is not None:
        net.set_option(_hip.INF_OPT_FUSED_K128, k128)
    stream = _hip.stream_of(x)
    net.refresh_if_needed(stream)
    ws = torch.empty(net.ws_bytes(B), dtype=torch.uint8, device=DEV)

    def poison():
        ws.fill_(255)
        _hip.check(net.lib.inf_debug_poison_lds(stream), 'poison_lds')
    y, g, ld = torch.empty_like(x), torch.empty_like(x), None
    _hip.profile_begin(20000)
    try:
        poison()
        _hip.check(net.lib.inf_net_forward(net.handle, _hip.ptr(x), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream),
                   'fwd')
        poison()
        _hip.check(net.lib.inf_net_vjp(net.handle, _hip.ptr(x), _hip.ptr(v), _hip.ptr(g), B, _hip.ptr(ws), ws.numel(),
                                       stream), 'vjp')
        if series:
            co = np.array([(-1) ** (k + 1) / k for k in range(1, series + 1)], dtype=np.float32)
            ld = torch.empty(B, device=DEV)
            poison()
            _hip.check(net.lib.inf_logdet_series(net.handle, _hip.ptr(x), _hip.ptr(torch.sign(v)),
                                                 co.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), series, _hip.ptr(ld),
                                                 B, _hip.ptr(ws), ws.numel(), stream), 'series')
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    return y, g, ld, tags


def _fp64(seq, x, v):
    """The same modules on the CPU in fp64: y = seq(x) and v^T dy/dx (zeros where y does not depend on x: Zero)."""
    ref = copy.deepcopy(seq).cpu().double()
    xr = x.detach().cpu().double().requires_grad_(True)
    y = ref(xr)
    g = torch.autograd.grad(y, xr, v.detach().cpu().double(), allow_unused=True)[0]
    return y.detach(), torch.zeros_like(xr) if g is None else g


# Inputs that put every branch of every activation's definition on the leading activation: 0, +-1 (LipschitzCube's
# pieces meet there), +-25 (past Softplus's threshold 20, and exp(-25) for ELU), +-1e-3 (inside the cube)
SPECIAL = [0., 1., -1., 25., -25., 1e-3, -1e-3]


def _with_specials(x, off_kink):
    """x with its first elements of every sample overwritten by SPECIAL.  off_kink (the derivative comparison): the exact
    kink values moved off the kink -- +-1 by one ulp outwards, 0 to +-1e-30 in turn -- because torch's own backward at
    a kink (ReLU at 0) is a convention, not something to pin."""
    x = x.clone()
    flat = x.view(x.shape[0], -1)
    vals = torch.tensor(SPECIAL)
    if off_kink:
        vals = torch.tensor([1e-30, float(np.nextafter(np.float32(1), np.float32(2))),
                             float(np.nextafter(np.float32(-1), np.float32(-2))), 25., -25., 1e-3, -1e-3])
    n = min(len(vals), flat.shape[1])          # d = 6 holds six of the seven: the values rotate over the samples
    for b in range(flat.shape[0]):
        row = vals * torch.tensor([-1., 1, 1, 1, 1, 1, 1]) if off_kink and b % 2 else vals
        flat[b, :n] = torch.roll(row, b)[:n]
    return x


@pytest.mark.parametrize('kind', ['conv', 'fc'])
@pytest.mark.parametrize('act', NEW_ACTS)
def test_formulas_match_fp64_torch(act, kind, monkeypatch):
    """Generic path (INFLOW_NO_FUSED=1): GEMM epilogue EP_ACT_ANY, the loader's leading activation, conv_out's
    derivative multiply, against fp64 torch.  conv: (3, 8, 8), hidden 64, kernels 3-1-3, leading activation, B = 3;
    fc: d = 6, 128-128, B = 33."""
    monkeypatch.setenv('INFLOW_NO_FUSED', '1')
    torch.manual_seed(3)
    A = lambda: ACT_FNS[act](False)
    if kind == 'conv':
        shape, B = (3, 8, 8), 3
        seq = torch.nn.Sequential(A(), _conv(3, 64, 3), A(), _conv(64, 64, 1), A(), _conv(64, 3, 3)).to(DEV)
    else:
        shape, B = (6,), 33
        seq = torch.nn.Sequential(_lin(6, 128), A(), _lin(128, 128), A(), _lin(128, 6)).to(DEV)
    with torch.no_grad():
        seq(torch.zeros(1, *shape, device=DEV))              # lazy u/v (engine power iteration)
    x0 = torch.randn(B, *shape) * 0.7
    v = torch.randn(B, *shape).to(DEV)
    for off_kink in (False, True):
        x = _with_specials(x0, off_kink).to(DEV)
        y, g, _, tags = _engine(seq, shape, x, v)
        assert not any(500 <= t < 700 for t in tags), sorted(tags)        # no fused kernel
        y_ref, g_ref = _fp64(seq, x, v)
        _close(y, y_ref)
        if off_kink:
            _close(g, g_ref)


def _net313(act, C, H, hid):
    torch.manual_seed(2)
    A = lambda: ACT_FNS[act](False)
    seq = torch.nn.Sequential(A(), _conv(C, hid, 3), A(), _conv(hid, hid, 1), A(), _conv(hid, C, 3)).to(DEV)
    with torch.no_grad():
        seq(torch.zeros(1, C, H, H, device=DEV))             # lazy u/v (engine power iteration)
    return seq


# (C, H, hid, B): scale 0 (at B = 2 its grid is under 256 64-pixel tiles, so the launcher takes 32-pixel tiles whatever
# INF_OPT_FUSED_K128 says; B = 16 is the smallest batch at which policy 2 reaches the 128-pixel kernel), the
# one-row-block-per-wave hid-256 instantiation, and the wide kernel
FUSED_SHAPES = [(3, 32, 512, 2), (3, 32, 512, 16), (12, 16, 256, 2), (48, 8, 512, 3)]


@pytest.mark.parametrize('C,H,hid,B', FUSED_SHAPES)
@pytest.mark.parametrize('act', ['elu', 'softplus', 'relu'])
def test_fused_313_matches_generic(act, C, H, hid, B, monkeypatch):
    """The fused 3-1-3 kernels' ELU / Softplus / ReLU instantiations (forward-mode epilogues, the halo staging's
    leading activation and its derivative in series chaining) against the generic GEMM chain: inf_net_forward,
    inf_net_vjp and a 6-term inf_logdet_series within 1e-5 max(1, |ref|), in all three inf_net_set_mfma modes, at
    (3, 32, 512, B) under INF_OPT_FUSED_K128 0 and 2; a fused kernel must have run (launch profile)."""
    seq = _net313(act, C, H, hid)
    x = (torch.randn(B, C, H, H) * 0.5).to(DEV)
    v = torch.randn(B, C, H, H).to(DEV)
    monkeypatch.setenv('INFLOW_NO_FUSED', '1')
    ref = _engine(seq, (C, H, H), x, v, series=6)
    assert not any(500 <= t < 550 for t in ref[3]), sorted(ref[3])
    monkeypatch.setenv('INFLOW_NO_FUSED', '0')
    for mfma in (0, 1, 2):
        for k128 in ((0, 2) if (C, H) == (3, 32) else (None,)):
            out = _engine(seq, (C, H, H), x, v, mfma=mfma, series=6, k128=k128)
            fused = sorted(t for t in out[3] if 500 <= t < 550)
            print(act, (C, H, hid, B), 'mfma', mfma, 'k128', k128, 'fused tags', fused)
            # forward (EVAL), derivative-saving forward (SAVE) and VJP launches of a fused family
            assert {t % 10 for t in fused} >= {0, 1, 2}, sorted(out[3])
            if k128 == 2 and mfma == 2 and B == 16:
                assert {530, 531, 532} <= set(fused), fused               # the 128-pixel kernel: EVAL, SAVE, VJP
            if k128 == 0:
                assert not any(530 <= t < 540 for t in fused), fused
            # ReLU at B = 16 (a shape added here to reach the 128-pixel instantiations, 16.8 M hidden units): the
            # forward only.  Its derivative is a step, and at this size some unit's pre-activation lies within the
            # arithmetic modes' rounding of 0: bf16x6 against the fp32 GEMM chain agreed to 4.5e-8 in the forward and
            # differed by 1.6e-3 in one VJP element, a flipped unit, which is not an error of either side.  The three
            # smaller shapes get no allowance (an fp32 and an fp64 evaluation of exactly these inputs differ by <= 4e-7 max|ref|); ELU and
            # Softplus exercise the same instantiations' derivative stores at B = 16.
            n_cmp = 1 if (act == 'relu' and B == 16) else 3
            for a, b in zip(out[:n_cmp], ref[:n_cmp]):
                _close(a, b, rel=1e-5)
            assert all(torch.isfinite(a).all() for a in out[:3])


def _mixed_block(act_x, act_z, C, hid):
    def nnet(act):
        A = lambda: ACT_FNS[act](False)
        return torch.nn.Sequential(A(), _conv(C, hid, 3), A(), _conv(hid, hid, 1), A(), _conv(hid, C, 3))
    return imBlock(nnet(act_x), nnet(act_z), n_dist='poisson', n_power_series=None, exact_trace=False,
                   brute_force=False, n_samples=1, n_exact_terms=10, neumann_grad=True, grad_in_forward=True,
                   eps_forward=1e-6)


@pytest.mark.parametrize('act_x,act_z', [('swish', 'elu'), ('elu', 'swish'), ('relu', 'softplus')])
def test_block_with_nets_of_different_fused_families(act_x, act_z, monkeypatch):
    """An imBlock whose two nets are both fused 3-1-3 nets of one shape but of different activations.  A pair launch
    picks one instantiation for both nets (Swish epilogues reading the betas, or the kind switch), so a Swish net and an
    ELU / Softplus / ReLU net must not share one: the engine runs them net by net.  Two kinds of the switch family may
    share a launch (the kind is per net).  The block's z and log-det against the same block on the generic path."""
    C, H, hid, B = 12, 16, 256, 2
    torch.manual_seed(4)
    blk = _mixed_block(act_x, act_z, C, hid).to(DEV)
    with torch.no_grad():
        for net in (blk.nnet_x, blk.nnet_z):
            net(torch.zeros(1, C, H, H, device=DEV))                      # lazy u / v (engine power iteration)
    blk.eval()
    x = (torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV)
    res = {}
    for mode in ('generic', 'fused'):
        monkeypatch.setenv('INFLOW_NO_FUSED', '1' if mode == 'generic' else '0')
        b = copy.deepcopy(blk)                                            # its own engine nets: reads INFLOW_NO_FUSED
        set_probe_mode('reference')
        np.random.seed(11)
        torch.manual_seed(11)
        _hip.profile_begin(20000)
        try:
            with torch.no_grad():
                z, lp = b(x, torch.zeros(B, 1, device=DEV))
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        assert any(500 <= t < 550 for t in tags) == (mode == 'fused'), sorted(tags)
        res[mode] = (z, lp, b.last_broyden['nstep'], b.last_n_power_series)
    assert res['fused'][2:] == res['generic'][2:]
    _close(res['fused'][0], res['generic'][0], rel=1e-5)
    _close(res['fused'][1], res['generic'][1], rel=1e-5)


def test_other_activations_stay_on_the_generic_path():
    """LipschitzCube has no fused form: a net of the shape (12, 16, 256, 2) takes no fused kernel; nor does a net whose
    hidden activations differ, or whose leading activation is of another kind than the hidden ones."""
    C, H, hid, B = 12, 16, 256, 2
    x = (torch.randn(B, C, H, H, generator=torch.Generator().manual_seed(2)) * 0.5).to(DEV)
    v = torch.sign(x)
    ELU, ReLU = torch.nn.ELU, torch.nn.ReLU
    seqs = [_net313('lcube', C, H, hid),
            torch.nn.Sequential(_conv(C, hid, 3), ELU(), _conv(hid, hid, 1), ReLU(), _conv(hid, C, 3)).to(DEV),
            torch.nn.Sequential(ReLU(), _conv(C, hid, 3), ELU(), _conv(hid, hid, 1), ELU(), _conv(hid, C, 3)).to(DEV)]
    for seq in seqs:
        with torch.no_grad():
            seq(torch.zeros(1, C, H, H, device=DEV))
        y, g, _, tags = _engine(seq, (C, H, H), x, v)
        assert not any(500 <= t < 550 for t in tags), sorted(tags)
        y_ref, g_ref = _fp64(seq, x, v)
        _close(y, y_ref)
        _close(g, g_ref)


def test_zero_flow_end_to_end():
    """The reference cannot evaluate a Zero flow (make_golden_acts.py), so there is no fixture; on the engine every net
    is then a constant (its last bias), so each block's log-det is exactly 0 and the flow equals its fp64 evaluation
    with the nets replaced by those constants: z_block = x + b_x - b_z."""
    arch = syn.CONFIGS['cifar10_small_zero']
    m = build_flow(arch, 2)
    m.load_state_dict(syn.make_state_dict(arch, 0), strict=True)
    m = m.to(DEV).eval()
    x = syn.image_batch(2, seed=3).to(DEV)
    rec = []

    def hook(mod, args, kwargs, out):
        lp_in = args[1] if len(args) > 1 else kwargs.get('logpx')
        rec.append((args[0].detach(), out[0].detach(), (lp_in - out[1]).detach()))
    hooks = [b.register_forward_hook(hook, with_kwargs=True) for b in imblocks(m)]
    try:
        np.random.seed(7)
        torch.manual_seed(7)
        loss, logpx, z = image_logpx(m, x, arch['nvals'])
        torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    assert len(rec) == 6 and torch.isfinite(logpx).all()
    for blk, (xin, zout, ld) in zip(imblocks(m), rec):
        assert float(ld.abs().max()) == 0.0
        bx, bz = blk.nnet_x[-1].bias.detach(), blk.nnet_z[-1].bias.detach()
        want = xin.double() + (bx.double() - bz.double()).view(1, -1, 1, 1)
        _close(zout, want)


@pytest.mark.parametrize('mfma', ['f16x3', 'f32'])
@pytest.mark.parametrize('name', ['power_elu', 'toy_softplus'])
def test_fused_fc_matches_generic(name, mfma, monkeypatch):
    """fcnet_kernel / fcnet_h3_kernel instantiated for ELU and Softplus (FWD, and JAC + LU for the toy net's exact
    log-det) against the generic per-layer path, as test_fused_fc_net_matches_generic does for Sin: the same Broyden
    steps per block, nats within 1e-5, per-sample log p within 2e-4, z within 2e-5.  The POWER-shaped net's power
    series runs per launch (the one-launch series kernel has no ELU instantiation): tag 620 must not appear."""
    arch = syn.CONFIGS[name]
    B = 200
    x = syn.tabular_batch(B, arch['d'], seed=17).to(DEV)
    monkeypatch.setenv('INFLOW_MFMA', mfma)
    res = {}
    for mode in ('generic', 'fused'):
        monkeypatch.setenv('INFLOW_NO_FUSED', '1' if mode == 'generic' else '0')
        m = build_flow(arch, B)
        m.load_state_dict(syn.make_state_dict(arch, 0), strict=True)
        m = m.to(DEV).eval()
        np.random.seed(5)
        torch.manual_seed(5)
        _hip.profile_begin(20000)
        try:
            loss, logpx, z = tabular_logpx(m, x)
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        assert (600 in tags) == (mode == 'fused'), sorted(tags)
        if arch['brute_force']:
            assert (601 in tags or 602 in tags) == (mode == 'fused'), sorted(tags)
        assert 610 not in tags and 620 not in tags, sorted(tags)
        if mode == 'fused':
            want = 2 if mfma == 'f16x3' else 0
            nets = engine_nets(m)
            assert nets and all(n.lib.inf_net_get_mfma(n.handle) == want for n in nets)
        res[mode] = (loss.item(), logpx.view(-1).cpu().double(), z.cpu(), [b.last_broyden['nstep'] for b in imblocks(m)])
    (lg, pg, zg, ng), (lf, pf, zf, nf) = res['generic'], res['fused']
    print('nats generic %.8f fused %.8f; max |d log p| %.2e' % (lg, lf, (pg - pf).abs().max().item()))
    assert ng == nf
    assert abs(lg - lf) <= 1e-5
    assert (pg - pf).abs().max().item() <= 2e-4
    _close(zf, zg)


def test_fused_fc_per_sample_falls_back_from_block_kernel():
    """Under the per-sample rule inf_imblock_eval_exact asks the block kernel (fcblock.hip) first; it has no Softplus
    instantiation and refuses, and the launch-per-iteration path takes the block: no tag 610, the fused JAC launches
    run, and the result agrees with the global rule's to the solves' own tolerance (eps_forward 1e-6 per element)."""
    arch = syn.CONFIGS['toy_softplus']
    B = 64
    x = syn.checkerboard_batch(B, seed=3).to(DEV)
    m = build_flow(arch, B)
    m.load_state_dict(syn.make_state_dict(arch, 0), strict=True)
    m = m.to(DEV).eval()
    out = {}
    for rule in ('global', 'per_sample'):
        for b in imblocks(m):
            b.convergence = rule
        _hip.profile_begin(20000)
        try:
            loss, logpx, z = tabular_logpx(m, x)
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        assert 610 not in tags and (601 in tags or 602 in tags), sorted(tags)
        assert all(b.last_broyden['convergence'] == rule and not b.last_broyden['prot_break'] for b in imblocks(m))
        out[rule] = (loss.item(), logpx.view(-1).cpu().double(), z.cpu())
    assert torch.isfinite(out['per_sample'][1]).all()
    # both rules stop at |g| <= eps_forward per element of the block: z agrees to ~n_blocks * 1e-6 / (1 - Lip)
    assert (out['global'][2] - out['per_sample'][2]).abs().max().item() <= 1e-3
    assert abs(out['global'][0] - out['per_sample'][0]) <= 1e-3


# ---- fixtures of the reference ---------------------------------------------------------------------------------
def _golden(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def _check_flow(m, g, run, hooked=True):
    """run() evaluates m on the fixture's input with the fixture's seeds; per imBlock nstep / lowest_step / series length
    exact, z within 2e-5 max(1, |z|), log-det within 2e-3 nats; per-sample log p within 2e-3 nats + 2 ulps; the loss
    within 1e-5; the flow output within 2e-5 max(1, |z|).  hooked=False: run() does not call the blocks' forward (the
    fc chain call, one engine call for all blocks), so there is no per-block z / log-det to compare."""
    rec = []

    def hook(mod, args, kwargs, out):
        lp_in = args[1] if len(args) > 1 else kwargs.get('logpx')
        z, lp_out = out
        rec.append((z.detach().reshape(z.shape[0], -1).cpu(), (lp_in - lp_out).detach().view(-1).cpu()))
    hooks = [b.register_forward_hook(hook, with_kwargs=True) for b in imblocks(m)]
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    try:
        loss, logpx, z = run()
        torch.cuda.synchronize()
    finally:
        for h in hooks:
            h.remove()
    blocks = imblocks(m)
    assert len(blocks) == int(g['nblocks']) and len(rec) == (len(blocks) if hooked else 0)
    for i, b in enumerate(blocks):
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'block %d nstep' % i
        assert b.last_broyden['lowest_step'] == int(g['b%d_lowest_step' % i]), 'block %d lowest_step' % i
        assert int(b.last_broyden['prot_break']) == int(g['b%d_prot_break' % i]) == 0
        if 'b%d_n_power_series' % i in g:
            assert b.last_n_power_series == int(g['b%d_n_power_series' % i][0]), 'block %d n_ps' % i
        if hooked:
            zr = torch.from_numpy(g['b%d_z' % i]).reshape(rec[i][0].shape)
            _close(rec[i][0], zr)
            np.testing.assert_allclose(rec[i][1].numpy(), g['b%d_logdet' % i], rtol=0, atol=2e-3)
    print('loss %.8f ref %.8f |d| %.2e' % (loss.item(), float(g['loss']), abs(loss.item() - float(g['loss']))))
    assert abs(loss.item() - float(g['loss'])) <= 1e-5
    np.testing.assert_allclose(logpx.view(-1).cpu().numpy(), g['logpx'], rtol=4e-7, atol=2e-3)
    _close(z.reshape(z.shape[0], -1), torch.from_numpy(g['z']))


FLOW_FIXTURES = ([('act_%s_small_b2' % a, 'cifar10_small_' + a) for a in NEW_ACTS if a != 'zero'] +
                 [('act_%s_full_b2' % a, 'cifar10_' + a) for a in ('elu', 'softplus', 'relu')] +
                 [('act_elu_power_b64', 'power_elu'), ('act_softplus_toy_b64', 'toy_softplus')])


@pytest.mark.parametrize('name,arch_name', FLOW_FIXTURES)
def test_flow_matches_reference_fixture(golden_dir, name, arch_name):
    """(No 'zero' flow: the reference itself cannot evaluate one, see make_golden_acts.py.)"""
    g = _golden(golden_dir, name)
    arch = syn.CONFIGS[arch_name]
    x = torch.from_numpy(g['x']).to(DEV)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV).eval()
    if arch['kind'] == 'conv':
        _check_flow(m, g, lambda: image_logpx(m, x, arch['nvals']))
    else:
        # the model's own eval: all blocks in one engine call (SequentialFlow.forward -> inf_flow_eval_exact_chain)
        _check_flow(m, g, lambda: tabular_logpx(m, x), hooked=False)
        assert all(n.lib.inf_net_get_mfma(n.handle) == 2 for n in engine_nets(m))    # fused fc kernels, f16x3

        def block_by_block():
            with torch.no_grad():
                z, lp = x, torch.zeros(x.shape[0], 1, device=DEV)
                for blk in m.chain:
                    z, lp = blk(z, lp)
                logpx = normal_logprob_sum(z) - lp
            return -torch.mean(logpx), logpx, z
        _check_flow(m, g, block_by_block)


def _nobias_block():
    p = dict(hidden=64, coeff=0.9)
    nnet = lambda: torch.nn.Sequential(_conv(3, p['hidden'], 3, bias=False, coeff=p['coeff']), torch.nn.ReLU(),
                                       _conv(p['hidden'], 3, 3, coeff=p['coeff']))
    return imBlock(nnet(), nnet(), n_dist='poisson', n_power_series=None, exact_trace=False, brute_force=False,
                   n_samples=1, n_exact_terms=10, neumann_grad=True, grad_in_forward=True, eps_forward=1e-6)


def test_bias_free_block_matches_reference_fixture(golden_dir):
    """One imBlock on (3, 8, 8) whose first conv has bias=None (InfLayerDesc.bias NULL: the engine's zero vector)."""
    g = _golden(golden_dir, 'nobias_relu_b4')
    blk = _nobias_block()
    sd = {k[3:]: torch.from_numpy(np.asarray(g[k])) for k in g.files if k.startswith('sd:')}
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(DEV).eval()
    assert blk.nnet_x[0].bias is None and blk.nnet_z[0].bias is None
    x = torch.from_numpy(g['x']).to(DEV)

    def run():
        with torch.no_grad():
            z, delta = blk(x, torch.zeros(x.shape[0], 1, device=DEV))
            logpx = normal_logprob_sum(z) - delta
        return -torch.mean(logpx), logpx, z
    _check_flow(blk, g, run)


@pytest.mark.parametrize('act', ['elu', 'lcube'])
def test_inverse_roundtrip(act):
    arch = syn.CONFIGS['cifar10_small_' + act]
    m = build_flow(arch, 3)
    m.load_state_dict(syn.make_state_dict(arch, 0), strict=True)
    m = m.to(DEV).eval()
    blk = imblocks(m)[2]
    torch.manual_seed(0)
    x = torch.randn(3, 12, 16, 16, device=DEV) * 0.5
    with torch.no_grad():
        z = blk(x)
        xr = blk.inverse(z)
    _close(xr, x, rel=1e-4)


def test_training_takes_autograd_and_matches_reference(golden_dir):
    """act_elu_small_train_b2: the engine's parameter-gradient kernels carry Swish / Sin only, so an ELU flow trains
    through the autograd route (_engine_grads false); loss, step counts and every parameter gradient against the
    reference's loss.backward(), at test_gpu_train.py's tolerances."""
    from test_gpu_train import _check_grads
    g = _golden(golden_dir, 'act_elu_small_train_b2')
    arch = syn.CONFIGS['cifar10_small_elu']
    x = torch.from_numpy(g['x']).to(DEV)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV).train()
    set_probe_mode('reference')
    np.random.seed(int(g['seed']))
    torch.manual_seed(int(g['seed']))
    loss, logpx, z = image_bits_per_dim_graph(m, x, arch['nvals'])
    loss.backward()
    torch.cuda.synchronize()
    blocks = imblocks(m)
    for i, b in enumerate(blocks):
        assert b._engine_grads(torch.empty(1, 1, 1, 1)) is False
        assert b.last_broyden['nstep'] == int(g['b%d_nstep' % i]), 'block %d forward nstep' % i
        assert b.last_broyden_backward['nstep'] == int(g['b%d_bwd_nstep' % i]), 'block %d bwd nstep' % i
    print('loss %.8f ref %.8f' % (loss.item(), float(g['loss'])))
    assert abs(loss.item() - float(g['loss'])) <= 1e-5, (loss.item(), float(g['loss']))
    n = _check_grads(m, g)
    assert n == len([k for k in g.files if k.startswith('g:') or k.startswith('gs:')])


def test_still_refused():
    """A net that ends in an activation (the classification blocks, out of scope) and non-default activation parameters
    raise HipError; there is no fallback."""
    x = torch.zeros(2, 3, 8, 8, device=DEV)
    tail = torch.nn.Sequential(_conv(3, 8, 3), torch.nn.ELU(), _conv(8, 3, 3), torch.nn.ELU()).to(DEV)
    with pytest.raises(_hip.HipError):
        _hip.native_net(tail, x.shape[1:], x.device)
    for mod in (torch.nn.ELU(alpha=0.5), torch.nn.Softplus(beta=2)):
        seq = torch.nn.Sequential(_conv(3, 8, 3), mod, _conv(8, 3, 3)).to(DEV)
        with pytest.raises(_hip.HipError):
            _hip.native_net(seq, x.shape[1:], x.device)
