"""The fused 3-1-3 kernels on images that do not cut into whole tiles (ragged whole-row tiles): a tile is
rows = min(H, floor(bn / W)) whole image rows, so it has bn - rows * W dead pixel columns, and the last tile of an image
may hold fewer live rows.  The MNIST scales (28x28, 14x14, 7x7) are the reference's own such shapes.

Tolerances (the project's, tests/test_gpu_acts.py):
  * fused against the GEMM chain:  1e-5 * max(1, |ref|_inf)
  * the generic shape against fp64: 2e-6 * max(1, |ref|_inf)
  * the reference fixture:          test_gpu_acts._check_flow's (trajectories exact, z 2e-5, log p 2e-3 nats, loss 1e-5)
  * parameter gradients:            2e-4 of the tensor's largest element (see test_training_step_...)
Workspace and LDS are filled with NaN before every direct engine call; the kernels that ran are read from the launch
profile (tags 50x net313_kernel, 51x _h, 52x _w, 53x the 128-pixel kernel, 54x the two-per-CU kernel).
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.density import image_logpx
from lib.implicit_flow import ACT_FNS
from lib.layers import imBlock, set_probe_mode
from lib.layers.base import get_conv2d

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N_TERMS = 6


def _close(a, b, rel):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    print('max abs err %.3e (bound %.3e)' % (err, rel * scale))
    assert torch.isfinite(a).all()
    assert err <= rel * scale, 'max abs err %g > %g' % (err, rel * scale)


def _conv(a, b, k):
    return get_conv2d(a, b, k, 1, k // 2, coeff=0.9, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)


def _net313(act, C, H, W, hid):
    """[act], conv3 C -> hid, act, conv1 hid -> hid, act, conv3 hid -> C on (C, H, W), u / v initialised."""
    torch.manual_seed(2)
    A = lambda: ACT_FNS[act](False)
    seq = torch.nn.Sequential(A(), _conv(C, hid, 3), A(), _conv(hid, hid, 1), A(), _conv(hid, C, 3)).to(DEV)
    with torch.no_grad():
        seq(torch.zeros(1, C, H, W, device=DEV))             # lazy u/v (engine power iteration)
    return seq


def _engine(seq, shape, x, v, mfma=None, k128=None):
    """inf_net_forward, inf_net_vjp, a 6-term inf_logdet_series and a 6-term inf_neumann_vector of a fresh engine net of
    `seq` (it reads INFLOW_NO_FUSED), NaN-poisoned workspace and LDS before every call.  Returns ((y, g, ld, w), tags)."""
    B = x.shape[0]
    net = _hip.NativeNet(_hip.net_entries(seq), shape, x.device)
    if mfma is not None:
        _hip.check(net.lib.inf_net_set_mfma(net.handle, mfma), 'set_mfma')
    if k128 is not None:
        net.set_option(_hip.INF_OPT_FUSED_K128, k128)
    stream = _hip.stream_of(x)
    net.refresh_if_needed(stream)
    ws = torch.empty(net.ws_bytes(B), dtype=torch.uint8, device=DEV)
    eps = torch.sign(v)
    co = np.array([(-1) ** (k + 1) / k for k in range(1, N_TERMS + 1)], dtype=np.float32)
    nco = np.array([(-1) ** k * (1.0 if k < 4 else 0.5) for k in range(N_TERMS + 1)], dtype=np.float32)
    fptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def poison():
        ws.fill_(255)
        _hip.check(net.lib.inf_debug_poison_lds(stream), 'poison_lds')
    y, g, ld, w = torch.empty_like(x), torch.empty_like(x), torch.empty(B, device=DEV), torch.empty_like(x)
    _hip.profile_begin(20000)
    try:
        poison()
        _hip.check(net.lib.inf_net_forward(net.handle, _hip.ptr(x), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream),
                   'fwd')
        poison()
        _hip.check(net.lib.inf_net_vjp(net.handle, _hip.ptr(x), _hip.ptr(v), _hip.ptr(g), B, _hip.ptr(ws), ws.numel(),
                                       stream), 'vjp')
        poison()
        _hip.check(net.lib.inf_logdet_series(net.handle, _hip.ptr(x), _hip.ptr(eps), fptr(co), N_TERMS, _hip.ptr(ld), B,
                                             _hip.ptr(ws), ws.numel(), stream), 'series')
        poison()
        _hip.check(net.lib.inf_neumann_vector(net.handle, _hip.ptr(x), _hip.ptr(eps), fptr(nco), N_TERMS, _hip.ptr(w), B,
                                              _hip.ptr(ws), ws.numel(), stream), 'neumann')
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    return (y, g, ld, w), tags


def _fused(tags):
    return sorted(t for t in tags if 500 <= t < 550)


def _inputs(C, H, W, B):
    gen = torch.Generator().manual_seed(5)
    x = (torch.randn(B, C, H, W, generator=gen) * 0.5).to(DEV)
    v = torch.randn(B, C, H, W, generator=gen).to(DEV)
    return x, v


def _chain_reference(seq, shape, x, v, monkeypatch):
    """The GEMM chain: a deep copy of the net whose engine net is created under INFLOW_NO_FUSED=1."""
    monkeypatch.setenv('INFLOW_NO_FUSED', '1')
    ref, tags = _engine(copy.deepcopy(seq), shape, x, v)
    monkeypatch.setenv('INFLOW_NO_FUSED', '0')
    assert not _fused(tags), sorted(tags)
    return ref


# (C, H, W, hid, B), the smallest shapes that reach each failure mode, and the 32-pixel (51x / 52x) or 64-pixel (50x)
# family the launcher must pick:
RAGGED_SHAPES = [
    (1, 28, 28, 512, 2, 32),     # dead columns, 32-pixel variants: 1 row of 28 per tile
    (1, 28, 28, 512, 19, 64),    # 14 x 19 = 266 64-pixel tiles >= 256: the 64-pixel variant is kept (2 rows, 56 / 64)
    (4, 14, 14, 256, 2, 32),     # short last tile: 2 of 4 rows at 64 pixels, 7 full tiles of 2 rows at 32
    (16, 7, 7, 512, 3, 32),      # the whole image in one 64-pixel tile; P = 49 (taps not 16-byte aligned), 9C = 144
    (3, 5, 12, 256, 3, 32),      # H no multiple of rows at 32 pixels (2 + 2 + 1); one 60-column tile at 64
    (2, 3, 31, 256, 2, 32),      # odd W: one dead column per one-row tile
    (2, 4, 40, 256, 2, 64),      # 32 < W <= 64: only the 64-pixel variant tiles it, however small the grid
    # At B = 2 or 3 the grids above are so small that every 32-pixel case lands on the wide kernel (52x).  Two more
    # batches of the 14x14 shape reach the other two kernels' ragged code:
    (4, 14, 14, 256, 64, 64),    # 4 x 64 = 256 64-pixel tiles: net313_kernel with a short last tile (2 of 4 rows)
    (4, 14, 14, 256, 40, 'h'),   # 160 64-pixel tiles < 256 < 280 32-pixel tiles: the two-per-CU net313_kernel_h (51x)
]
CASES = [('swish',) + s for s in RAGGED_SHAPES] + [('elu', 4, 14, 14, 256, 2, 32), ('softplus', 16, 7, 7, 512, 3, 32)]


@pytest.mark.parametrize('act,C,H,W,hid,B,family', CASES)
def test_ragged_fused_matches_gemm_chain(act, C, H, W, hid, B, family, monkeypatch):
    """inf_net_forward, inf_net_vjp, a 6-term inf_logdet_series (each term stages the previous one's taps and forms the
    trace partial per tile) and a 6-term inf_neumann_vector (the staging's acc_w write) of the fused kernels on ragged
    shapes against the GEMM chain, within 1e-5 max(1, |ref|), in all three inf_net_set_mfma modes.  A NaN that a dead
    column read from poisoned LDS, or a dead column's value stored to the taps or added to a trace partial, shows in
    these.  Swish nets with a leading Swish; one ELU and one Softplus net for the ACTK = 1 forwards.  No ReLU: its
    derivative's kink makes a flipped unit a legitimate difference."""
    seq = _net313(act, C, H, W, hid)
    x, v = _inputs(C, H, W, B)
    ref = _chain_reference(seq, (C, H, W), x, v, monkeypatch)
    for mfma in (0, 1, 2):
        out, tags = _engine(seq, (C, H, W), x, v, mfma=mfma)
        fused = _fused(tags)
        print(act, (C, H, W, hid, B), 'mfma', mfma, 'fused tags', fused)
        # forward (EVAL), derivative-saving forward (SAVE) and VJP launches of a fused family
        assert {t % 10 for t in fused} >= {0, 1, 2}, sorted(tags)
        if family == 64:
            assert all(t < 510 for t in fused), fused
        elif family == 'h':
            assert all(510 <= t < 520 for t in fused), fused
        else:
            assert all(510 <= t < 530 for t in fused), fused
        for a, b in zip(out, ref):
            _close(a, b, rel=1e-5)


@pytest.mark.parametrize('policy', [2, 3])
def test_k128_policies_fall_back_to_the_64_pixel_kernel(policy, monkeypatch):
    """INF_OPT_FUSED_K128 = 2 / 3 ask for the 128-pixel and the two-per-CU kernels, which take exact tiles only: on
    (1, 28, 28) at B = 19 the launcher must fall back to net313_kernel without an error, with the same results."""
    C, H, W, hid, B = 1, 28, 28, 512, 19
    seq = _net313('swish', C, H, W, hid)
    x, v = _inputs(C, H, W, B)
    ref = _chain_reference(seq, (C, H, W), x, v, monkeypatch)
    base, tags0 = _engine(seq, (C, H, W), x, v, mfma=2, k128=0)
    out, tags = _engine(seq, (C, H, W), x, v, mfma=2, k128=policy)
    print('policy', policy, 'fused tags', _fused(tags))
    assert not tags & {530, 532, 542}, sorted(tags)
    assert {500, 501, 502} <= tags, sorted(tags)
    for a, b, c in zip(out, base, ref):
        assert torch.equal(a, b)                      # the same kernel, the same launch: the same bits
        _close(a, c, rel=1e-5)


def test_segment_tiles_that_do_not_divide_stay_generic():
    """W = 72 > 64 with W % 64 != 0 (segment tiles) is not covered: no fused kernel, and the GEMM chain's forward and
    VJP are within 2e-6 max(1, |ref|) of an fp64 evaluation of the same modules."""
    C, H, W, hid, B = 2, 4, 72, 256, 2
    seq = _net313('swish', C, H, W, hid)
    x, v = _inputs(C, H, W, B)
    (y, g, ld, w), tags = _engine(seq, (C, H, W), x, v)
    assert not _fused(tags), sorted(tags)
    ref = copy.deepcopy(seq).cpu().double()
    xr = x.detach().cpu().double().requires_grad_(True)
    y_ref = ref(xr)
    g_ref = torch.autograd.grad(y_ref, xr, v.detach().cpu().double())[0]
    _close(y, y_ref, rel=2e-6)
    _close(g, g_ref, rel=2e-6)


def _block(C, hid):
    def nnet():
        A = lambda: ACT_FNS['swish'](False)
        return torch.nn.Sequential(A(), _conv(C, hid, 3), A(), _conv(hid, hid, 1), A(), _conv(hid, C, 3))
    return imBlock(nnet(), nnet(), n_dist='poisson', n_power_series=None, exact_trace=False, brute_force=False,
                   n_samples=1, n_exact_terms=10, neumann_grad=True, grad_in_forward=True, eps_forward=1e-6)


def _mnist_block(seed):
    torch.manual_seed(seed)
    blk = _block(1, 256).to(DEV)
    with torch.no_grad():
        for net in (blk.nnet_x, blk.nnet_z, blk.nnet_x_copy, blk.nnet_z_copy):
            net(torch.zeros(1, 1, 28, 28, device=DEV))                    # lazy u / v (engine power iteration)
    return blk


@pytest.mark.parametrize('overlap', ['1', '0'])
def test_block_fused_matches_generic(overlap, monkeypatch):
    """One (1, 28, 28) imBlock, idim 256, B = 3 (pair launches, ensure_f0, the root solve, both series): fused against
    generic under the overlapped (default) and the sequential schedule: the same Broyden steps and series length, z and
    log-det within 1e-5 max(1, |ref|)."""
    B = 3
    blk = _mnist_block(4).eval()
    x = (torch.randn(B, 1, 28, 28, generator=torch.Generator().manual_seed(5)) * 0.5).to(DEV)
    monkeypatch.setenv('INFLOW_EVAL_OVERLAP', overlap)
    res = {}
    for mode in ('generic', 'fused'):
        monkeypatch.setenv('INFLOW_NO_FUSED', '1' if mode == 'generic' else '0')
        b = copy.deepcopy(blk)                                            # its own engine nets: reads the environment
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
        assert bool(_fused(tags)) == (mode == 'fused'), sorted(tags)
        nets = [n for net in (b.nnet_x, b.nnet_z) for n in net.__dict__['_inf_native'].values()]
        assert nets and all(n.get_option(_hip.INF_OPT_EVAL_OVERLAP) == int(overlap) for n in nets)
        res[mode] = (z, lp, b.last_broyden['nstep'], b.last_n_power_series)
    print('nstep', res['fused'][2], 'series', res['fused'][3])
    assert res['fused'][2:] == res['generic'][2:]
    _close(res['fused'][0], res['generic'][0], rel=1e-5)
    _close(res['fused'][1], res['generic'][1], rel=1e-5)


def test_mnist_flow_matches_reference_fixture(golden_dir):
    """mnist_b2 (tests/golden/make_golden_ragged.py): the reference's ImplicitFlow on (2, 1, 28, 28), one block per
    scale at idim 256, with test_gpu_acts.test_flow_matches_reference_fixture's comparisons; every scale of it runs on
    fused kernels."""
    from test_gpu_acts import _check_flow
    g = np.load(os.path.join(golden_dir, 'mnist_b2.npz'))
    arch = syn.CONFIGS['mnist_small']
    x = torch.from_numpy(g['x']).to(DEV)
    assert tuple(x.shape) == (2, 1, 28, 28)
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(syn.make_state_dict(arch, int(g['weight_seed'])), strict=True)
    m = m.to(DEV).eval()
    _hip.profile_begin(20000)
    try:
        _check_flow(m, g, lambda: image_logpx(m, x, arch['nvals']))
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    assert _fused(tags), sorted(tags)
    assert not any(1000 <= t for t in tags), sorted(tags)                 # no GEMM-chain launch: all three scales fused


def test_training_step_fused_matches_generic(monkeypatch):
    """One loss.backward() of a train-mode (1, 28, 28) imBlock, idim 256, B = 2: the forward, the root solves and the
    Neumann pair run on the fused kernels (ragged tiles), the parameter gradients on the GEMM chain (the engine's
    gradient kernels).  Against the same block created under INFLOW_NO_FUSED=1.

    Bound, per tensor: 2e-4 of the reference tensor's largest element, the cap of test_gpu_conv_grads.py's per-tensor
    bound min(2e-4, max(8 e32, 1e-6)).  Its e32 term needs an fp64 evaluation of the whole implicit step, which does
    not exist; what separates the two runs here is the fused kernels' forward (1e-5 of the chain's, above) carried
    through two root solves stopped at 1e-6 per element, not the rounding of one contraction, so the cap is the
    applicable part."""
    B = 2
    blk = _mnist_block(6)
    x = (torch.randn(B, 1, 28, 28, generator=torch.Generator().manual_seed(7)) * 0.5).to(DEV)
    res = {}
    for mode in ('generic', 'fused'):
        monkeypatch.setenv('INFLOW_NO_FUSED', '1' if mode == 'generic' else '0')
        b = copy.deepcopy(blk).train()
        set_probe_mode('reference')
        np.random.seed(13)
        torch.manual_seed(13)
        _hip.profile_begin(20000)
        try:
            z, lp = b(x, torch.zeros(B, 1, device=DEV))
            logpz = (-0.5 * np.log(2 * np.pi) - z.pow(2) / 2).view(B, -1).sum(1, keepdim=True)
            loss = -torch.mean(logpz - lp)
            loss.backward()
            torch.cuda.synchronize()
        finally:
            tags = {s_['tag'] for s_ in _hip.profile_end()}
        assert bool(_fused(tags)) == (mode == 'fused'), sorted(tags)
        grads = {k: p.grad.detach().double().cpu() for k, p in b.named_parameters() if p.grad is not None}
        res[mode] = (loss.item(), grads, b.last_broyden['nstep'], b.last_broyden_backward['nstep'])
    print('loss generic %.8f fused %.8f; nstep fwd/bwd %s / %s' % (res['generic'][0], res['fused'][0],
                                                                    res['fused'][2:], res['generic'][2:]))
    assert res['fused'][2:] == res['generic'][2:]
    assert abs(res['fused'][0] - res['generic'][0]) <= 1e-5 * max(1.0, abs(res['generic'][0]))
    assert res['generic'][1] and set(res['fused'][1]) == set(res['generic'][1])
    bad = []
    for k, ref in res['generic'][1].items():
        got = res['fused'][1][k]
        scale = max(ref.abs().max().item(), 1e-12)
        err = (got - ref).abs().max().item() / scale
        print('%-28s rel err %.3e (bound 2e-4) scale %.3e' % (k, err, scale))
        assert torch.isfinite(got).all()
        if not err <= 2e-4:
            bad.append('%s: %.3e' % (k, err))
    assert not bad, bad
