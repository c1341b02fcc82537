"""Which schedule and which fused VJP kernel inf_imblock_eval takes per batch size and INF_OPT_FUSED_K128 policy.

The overlapped eval schedule (INF_OPT_EVAL_OVERLAP = 1, the default) queues the x- and z-branch log-det series as
single-net launches; the sequential one runs them as one pair launch per term.  The 128-pixel K-chunked VJP
(fused313k.hip, launch tag 532) is taken where the launch's grid covers every CU, so a pair launch can reach it where
a single-net launch falls back to the 64-pixel kernel (tag 502; 512 its 32-pixel two-per-CU variant).  Where that
happens the overlapped schedule hands the block to the sequential pair path; everywhere else it is unchanged.

One imBlock's pair of 3-1-3 Swish nets of hidden width 512 on (C, H, W) = (12, 16, 16) (the CIFAR-10 model's
16x16 scale), the smallest shape at which the pair's 128-pixel grid covers 256 CUs (B = 64) and the single net's does
not; 3 series terms, a solve of at most 6 steps; workspace and every CU's LDS NaN-poisoned before each call.
"""
import ctypes

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks

DEV = 'cuda:0'
N_TERMS = 3
T = 6
K128_VJP, V64_VJP, VHALF_VJP = 532, 502, 512
# inf_net313_kernel_family's values (include/inflow.h)
FAM_64, FAM_HALF, FAM_WIDE, FAM_K128, FAM_P64 = 0, 1, 2, 3, 4
MODE_EVAL, MODE_VJP = 0, 2


@pytest.fixture(scope='module')
def block():
    """The first 16x16 imBlock of the CIFAR-10 model (12 channels, hidden width 512), on the device, in eval."""
    arch = syn.CIFAR10
    m = build_flow(arch, 2)
    m.load_state_dict(syn.make_state_dict(arch, 0, power_iters=5), strict=True)
    m = m.to(DEV).eval()
    blk = imblocks(m)[2]
    assert blk.nnet_x[-1].weight.shape[0] == 12 and blk.nnet_x[-1].weight.shape[1] == 512
    return blk


def _eval(blk, B, overlap, k128=None):
    """One inf_imblock_eval call on seeded inputs; returns the results on the host and the launch count per tag."""
    g = torch.Generator().manual_seed(100 + B)
    x = (torch.randn(B, 12, 16, 16, generator=g) * 0.5).to(DEV)
    eps = [torch.sign(torch.randn(B, 12, 16, 16, generator=g)).to(DEV) for _ in range(2)]
    nx, nz, stream = blk._native(x)
    prev = {n: (n.get_option(_hip.INF_OPT_EVAL_OVERLAP), n.get_option(_hip.INF_OPT_FUSED_K128)) for n in (nx, nz)}
    for n in (nx, nz):
        n.set_option(_hip.INF_OPT_EVAL_OVERLAP, overlap)
        if k128 is not None:
            n.set_option(_hip.INF_OPT_FUSED_K128, k128)
    co = np.array([(-1) ** (k + 1) / k for k in range(1, N_TERMS + 1)], dtype=np.float32)
    ws = _hip.workspace(x.device, nx.ws_bytes(B, T) + nz.ws_bytes(B, 1) + nx.ws_bytes(B, 1))
    z = torch.empty_like(x)
    out = torch.empty(2, B, device=DEV)
    st = _hip.BroydenStats()
    ws.fill_(255)
    _hip.check(nx.lib.inf_debug_poison_lds(stream), 'poison_lds')
    _hip.profile_begin(2000)
    try:
        _hip.check(nx.lib.inf_imblock_eval(nx.handle, nz.handle, _hip.ptr(x), _hip.ptr(z), _hip.ptr(eps[0]),
                                           _hip.ptr(eps[1]), co.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                           N_TERMS, _hip.ptr(out[0]), _hip.ptr(out[1]), B, T, float(blk.eps_forward),
                                           ctypes.byref(st), _hip.ptr(ws), ws.numel(), stream), 'inf_imblock_eval')
        torch.cuda.synchronize()
    finally:
        launches = {s['tag']: s['launches'] for s in _hip.profile_end()}
        for n, (ov, kp) in prev.items():
            n.set_option(_hip.INF_OPT_EVAL_OVERLAP, ov)
            n.set_option(_hip.INF_OPT_FUSED_K128, kp)
    res = {'z': z.cpu(), 'logdet_x': out[0].cpu(), 'logdet_z': out[1].cpu(), 'nstep': st.nstep,
           'lowest_step': st.lowest_step}
    for k in ('z', 'logdet_x', 'logdet_z'):
        assert torch.isfinite(res[k]).all(), k
    vjp = {t: launches.get(t, 0) for t in (K128_VJP, V64_VJP, VHALF_VJP)}
    print('B %d overlap %d k128 %s: VJP launches %s, nstep %d' % (B, overlap, k128, vjp, st.nstep))
    return res, vjp


def _within_overlap_tolerances(a, b):
    """test_eval_overlap_matches_sequential's bounds: the same solve, per-sample log-dets within 2e-3 nats; z within
    the fp32 bound of the net comparisons, 2e-5 max(1, |z|_inf)."""
    assert a['nstep'] == b['nstep'] and a['lowest_step'] == b['lowest_step']
    for k in ('logdet_x', 'logdet_z'):
        np.testing.assert_allclose(a[k].numpy(), b[k].numpy(), rtol=0, atol=2e-3)
    scale = max(1.0, b['z'].abs().max().item())
    assert (a['z'] - b['z']).abs().max().item() <= 2e-5 * scale


@pytest.mark.gpu
def test_demoted_single_launch_takes_the_pair_schedule(block):
    """B = 64, default options: the pair launch reaches the 128-pixel kernel (2 * 64 * 2 = 256 tiles) and a single-net
    launch would not (128), so the block runs the sequential pair path: one 128-pixel launch per term, no 64-pixel VJP,
    and every result bit for bit that of INF_OPT_EVAL_OVERLAP = 0 (the same launches)."""
    res, vjp = _eval(block, 64, 1)
    ref, vjp0 = _eval(block, 64, 0)
    assert vjp == {K128_VJP: N_TERMS, V64_VJP: 0, VHALF_VJP: 0}
    assert vjp0 == vjp
    assert res['nstep'] == ref['nstep'] and res['lowest_step'] == ref['lowest_step']
    for k in ('z', 'logdet_x', 'logdet_z'):
        assert torch.equal(res[k], ref[k]), k


@pytest.mark.gpu
def test_pair_below_the_128_pixel_grid_stays_overlapped(block):
    """B = 63: the pair has 252 128-pixel tiles, so neither launch takes the 128-pixel kernel and the overlapped
    schedule runs as before, 2 * n_terms single-net launches.  They are launches of the 64-pixel family: at 252
    64-pixel tiles a single-net launch takes its 32-pixel two-per-CU variant (tag 512), as it always has below 256
    tiles; the sequential pair launch (504 tiles) takes the 64-pixel kernel (502)."""
    res, vjp = _eval(block, 63, 1)
    ref, vjp0 = _eval(block, 63, 0)
    assert vjp[K128_VJP] == 0 and vjp[V64_VJP] + vjp[VHALF_VJP] == 2 * N_TERMS
    assert vjp == {K128_VJP: 0, V64_VJP: 0, VHALF_VJP: 2 * N_TERMS}
    assert vjp0 == {K128_VJP: 0, V64_VJP: N_TERMS, VHALF_VJP: 0}
    _within_overlap_tolerances(res, ref)


@pytest.mark.gpu
def test_single_launch_on_the_128_pixel_grid_stays_overlapped(block):
    """B = 128: a single-net launch has 256 128-pixel tiles, so both schedules run the 128-pixel kernel and the
    overlapped one is kept: 2 * n_terms launches of 532, none of 502."""
    res, vjp = _eval(block, 128, 1)
    ref, vjp0 = _eval(block, 128, 0)
    assert vjp == {K128_VJP: 2 * N_TERMS, V64_VJP: 0, VHALF_VJP: 0}
    assert vjp0 == {K128_VJP: N_TERMS, V64_VJP: 0, VHALF_VJP: 0}
    _within_overlap_tolerances(res, ref)


@pytest.mark.gpu
@pytest.mark.parametrize('k128,tag', [(0, V64_VJP), (2, K128_VJP)])
def test_forced_policies_stay_overlapped(block, k128, tag):
    """B = 64 with INF_OPT_FUSED_K128 = 0 (64-pixel kernel only) and 2 (128-pixel wherever it fits): single-net and
    pair launches run the same kernel, so the overlapped schedule is kept, 2 * n_terms launches of that kernel."""
    res, vjp = _eval(block, 64, 1, k128)
    ref, vjp0 = _eval(block, 64, 0, k128)
    other = K128_VJP if tag == V64_VJP else V64_VJP
    assert vjp == {tag: 2 * N_TERMS, other: 0, VHALF_VJP: 0}
    assert vjp0 == {tag: N_TERMS, other: 0, VHALF_VJP: 0}
    _within_overlap_tolerances(res, ref)


# (C, H, W, B, nnets, layout_nets, policy, mode) -> kernel family, hidden width 512, f16x3 operands.  Tiles are counted
# per image: H * W / 64 for the 64-pixel layout, H * W / 128 for the 128-pixel kernel.
FAMILY_TABLE = [
    # the 16x16 scale: the pair reaches the 128-pixel kernel at B = 64, a single net at B = 128
    ((12, 16, 16, 64, 2, 2, 1, MODE_VJP), FAM_K128),
    ((12, 16, 16, 64, 1, 1, 1, MODE_VJP), FAM_64),
    ((12, 16, 16, 64, 1, 2, 1, MODE_VJP), FAM_64),
    ((12, 16, 16, 64, 1, 2, 1, MODE_EVAL), FAM_64),
    ((12, 16, 16, 63, 2, 2, 1, MODE_VJP), FAM_64),
    ((12, 16, 16, 63, 1, 1, 1, MODE_VJP), FAM_HALF),     # 252 64-pixel tiles: two 32-pixel workgroups per CU
    ((12, 16, 16, 128, 1, 1, 1, MODE_VJP), FAM_K128),
    ((12, 16, 16, 128, 2, 2, 1, MODE_VJP), FAM_K128),
    ((12, 16, 16, 32, 2, 2, 1, MODE_VJP), FAM_64),       # 256 64-pixel tiles, 128 128-pixel ones
    # the policies: 0 never, 2 wherever the 64-pixel layout holds, 3 the two-per-CU VJP (VJP launches only)
    ((12, 16, 16, 64, 2, 2, 0, MODE_VJP), FAM_64),
    ((12, 16, 16, 64, 1, 1, 2, MODE_VJP), FAM_K128),
    ((12, 16, 16, 64, 1, 1, 3, MODE_VJP), FAM_P64),
    ((12, 16, 16, 64, 1, 1, 3, MODE_EVAL), FAM_64),
    # below 256 64-pixel tiles no policy reaches it: 32-pixel tiles, two per CU above 256 of them, else one (wide)
    ((12, 16, 16, 40, 1, 1, 2, MODE_VJP), FAM_HALF),
    ((12, 16, 16, 16, 1, 1, 2, MODE_VJP), FAM_WIDE),
    # the 32x32 scale at B = 64: every launch covers the CUs
    ((3, 32, 32, 64, 1, 1, 1, MODE_VJP), FAM_K128),
    ((3, 32, 32, 64, 2, 2, 1, MODE_VJP), FAM_K128),
    # the 8x8 scale: one 64-pixel tile per image, no 128-pixel tile
    ((48, 8, 8, 64, 1, 1, 1, MODE_VJP), FAM_WIDE),
    ((48, 8, 8, 64, 2, 2, 1, MODE_VJP), FAM_WIDE),
    ((48, 8, 8, 64, 2, 2, 2, MODE_VJP), FAM_WIDE),
    # B = 256 and the CelebA-HQ 256 flow at B = 4: single-net and pair launches run the same family at every scale
    ((12, 16, 16, 256, 1, 1, 1, MODE_VJP), FAM_K128),
    ((12, 16, 16, 256, 2, 2, 1, MODE_VJP), FAM_K128),
    ((3, 256, 256, 4, 1, 1, 1, MODE_VJP), FAM_K128),
    ((3, 256, 256, 4, 2, 2, 1, MODE_VJP), FAM_K128),
    ((12, 128, 128, 4, 1, 1, 1, MODE_VJP), FAM_K128),
    ((12, 128, 128, 4, 2, 2, 1, MODE_VJP), FAM_K128),
    ((48, 64, 64, 4, 1, 1, 1, MODE_VJP), FAM_WIDE),
    ((48, 64, 64, 4, 2, 2, 1, MODE_VJP), FAM_WIDE),
    ((192, 32, 32, 4, 1, 1, 1, MODE_VJP), FAM_WIDE),
    ((192, 32, 32, 4, 2, 2, 1, MODE_VJP), FAM_WIDE),
]


def test_kernel_family_table():
    """The launcher's decision as a pure function (inf_net313_kernel_family, no device needed): the table above, an
    unsupported hidden width, and the operands' arithmetic (the 128-pixel kernel is f16x3 only)."""
    lib = _hip.load()
    for (C, H, W, B, nnets, layout, pol, mode), want in FAMILY_TABLE:
        got = lib.inf_net313_kernel_family(512, C, H, W, B, nnets, layout, pol, mode, 1)
        assert got == want, ((C, H, W, B, nnets, layout, pol, mode), got, want)
    assert lib.inf_net313_kernel_family(384, 12, 16, 16, 64, 2, 2, 1, MODE_VJP, 1) < 0
    assert lib.inf_net313_kernel_family(512, 12, 16, 16, 64, 3, 3, 1, MODE_VJP, 1) < 0
    assert lib.inf_net313_kernel_family(512, 12, 16, 16, 64, 2, 2, 1, MODE_VJP, 0) == FAM_64
