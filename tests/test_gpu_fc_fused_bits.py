"""Bit-level relations between the copies of the fused fc arithmetic: the block kernel (fcblock.hip:
mlp_jac2, mlp_pass, the LDS Broyden update) against the launch-per-iteration path (fcnet_h3.hip: the JAC and FWD
kernels, the update in global memory), and the JAC kernels' primal column against the FWD kernels.  The code comments
promise equal bits ("fcnet_h3.hip's JAC arithmetic", "same products, same order, same scales", "the JAC primal column
keeps the FWD kernel's bits"); these tests pin what a shared definition of the layer must keep.

  R1  the x-branch log-det (lx) of inf_imblock_eval_exact, INF_OPT_FC_BLOCK 2 against 0, both convergence rules;
  R2  under the global rule nstep, lowest_step and z of the same two runs;
  R3  on the launch path, z of inf_imblock_eval_exact against z of inf_imblock_forward, exact fp32 and f16x3.

Every relation is asserted with rtol = atol = 0; each was measured on the parent of the change that folded the copies
(profiles/r21/fused_bits_on_parent.txt).  Small nets with fixed seeds, B = 50 (two block / FWD workgroups of 48, the
second ragged: the global rule's exchange crosses workgroups; four JAC workgroups of 16) and B = 3, T = 8.
"""
import ctypes

import pytest
import torch

from lib import _hip
from lib.implicit_flow import ACT_FNS
from lib.layers.base import get_linear

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T = 8
EPS = 1e-6
TAG_FWD, TAG_JAC, TAG_BLOCK = 600, 601, 610
MFMA_F32, MFMA_F16X3 = 0, 2
# (d, hidden 128 x 128 layers, activation): the block kernel's four instantiations, then the other JAC activations
BLOCK_NETS = [(6, 3, 'sin'), (6, 3, 'swish'), (2, 1, 'sin'), (2, 1, 'swish')]
JAC_NETS = BLOCK_NETS + [(6, 3, 'elu'), (6, 3, 'softplus')]
_ids = lambda nets: ['d%d_h%d_%s' % n for n in nets]


def _seq(d, nh, act):
    lin = lambda a, b: get_linear(a, b, coeff=0.99, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    A = lambda: ACT_FNS[act](False)
    mods = [lin(d, 128)]
    for _ in range(nh):
        mods += [A(), lin(128, 128)]
    return torch.nn.Sequential(*mods, A(), lin(128, d))


_NETS = {}


def _nets(d, nh, act):
    """The block's two engine nets, built once per shape and shared by the tests (options are set per run)."""
    key = (d, nh, act)
    if key not in _NETS:
        out = []
        for seed in (3, 4):
            torch.manual_seed(seed)
            seq = _seq(d, nh, act).to(DEV)
            with torch.no_grad():
                seq(torch.zeros(1, d, device=DEV))             # lazy u / v
            out.append((seq, _hip.NativeNet(_hip.net_entries(seq), (d,), torch.device(DEV))))
        _NETS[key] = out
    (_, nx), (_, nz) = _NETS[key]
    return nx, nz


def _input(B, d):
    gen = torch.Generator().manual_seed(7 + B)
    return (torch.randn(B, d, generator=gen) * 0.5).to(DEV)


def _run(nx, nz, x, call, mfma, fc_block, per_sample):
    """One profiled inf_imblock_eval_exact / inf_imblock_forward: (z, lx, lz, stats, tags)."""
    B = x.shape[0]
    lib = nx.lib
    stream = _hip.stream_of(x)
    prev = []                                                  # (net, its arithmetic, its two options) to put back
    for n in (nx, nz):
        n.refresh_if_needed(stream)
        prev.append((n, lib.inf_net_get_mfma(n.handle), n.set_option(_hip.INF_OPT_FC_BLOCK, fc_block),
                     n.set_option(_hip.INF_OPT_CONVERGENCE, int(per_sample))))
        _hip.check(lib.inf_net_set_mfma(n.handle, mfma), 'set_mfma')
    ws = _hip.workspace(x.device, max(nx.ws_bytes(B, T), nz.ws_bytes(B, T), 1 << 24))
    W = (_hip.ptr(ws), ws.numel(), stream)
    z, lx, lz = torch.empty_like(x), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    st = _hip.BroydenStats()
    if per_sample:
        st.want_samples(B)
    _hip.profile_begin(20000)
    try:
        if call == 'eval_exact':
            _hip.check(lib.inf_imblock_eval_exact(nx.handle, nz.handle, _hip.ptr(x), _hip.ptr(z), _hip.ptr(lx),
                                                  _hip.ptr(lz), B, T, EPS, ctypes.byref(st), *W), call)
        else:
            _hip.check(lib.inf_imblock_forward(nx.handle, nz.handle, _hip.ptr(x), _hip.ptr(z), B, T, EPS,
                                               ctypes.byref(st), *W), call)
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
        for n, mode, fcb, conv in prev:
            _hip.check(lib.inf_net_set_mfma(n.handle, mode), 'set_mfma')
            n.set_option(_hip.INF_OPT_FC_BLOCK, fcb)
            n.set_option(_hip.INF_OPT_CONVERGENCE, conv)
    return z, lx, lz, st.as_dict(T), tags


def _maxdiff(a, b):
    return (a.double() - b.double()).abs().max().item()


def _block_and_launch(net, B, per_sample):
    nx, nz = _nets(*net)
    x = _input(B, net[0])
    blk = _run(nx, nz, x, 'eval_exact', MFMA_F16X3, 2, per_sample)
    per = _run(nx, nz, x, 'eval_exact', MFMA_F16X3, 0, per_sample)
    assert TAG_BLOCK in blk[4] and not blk[4] & {TAG_FWD, TAG_JAC}, sorted(blk[4])
    assert TAG_BLOCK not in per[4] and {TAG_FWD, TAG_JAC} <= per[4], sorted(per[4])
    return blk, per


@pytest.mark.parametrize('per_sample', [False, True], ids=['global', 'per_sample'])
@pytest.mark.parametrize('B', [50, 3])
@pytest.mark.parametrize('net', BLOCK_NETS, ids=_ids(BLOCK_NETS))
def test_r1_block_kernel_x_logdet_equals_jac_kernel(net, B, per_sample):
    """mlp_jac2 (two row tiles x two column groups per wave) against the fcnet_h3 JAC kernel (one row tile, every
    column block per wave): the same per-column arithmetic, so the x-branch log-det has the same bits."""
    blk, per = _block_and_launch(net, B, per_sample)
    print('R1 %s B %d: max |lx block - lx launch| %.3e' % (net, B, _maxdiff(blk[1], per[1])))
    torch.testing.assert_close(blk[1], per[1], rtol=0, atol=0)


@pytest.mark.parametrize('B', [50, 3])
@pytest.mark.parametrize('net', BLOCK_NETS, ids=_ids(BLOCK_NETS))
def test_r2_block_kernel_solve_equals_launch_path_global_rule(net, B):
    """The block kernel's solve (the update on LDS state, mlp_pass with resident weights, the norm exchanged between
    the workgroups) against the FWD kernel with the in-kernel update on global state, under the global rule: the same
    step count, lowest step and z, bit for bit."""
    blk, per = _block_and_launch(net, B, False)
    print('R2 %s B %d: nstep %d / %d, lowest_step %d / %d, max |z block - z launch| %.3e' % (
        net, B, blk[3]['nstep'], per[3]['nstep'], blk[3]['lowest_step'], per[3]['lowest_step'],
        _maxdiff(blk[0], per[0])))
    assert blk[3]['nstep'] == per[3]['nstep']
    assert blk[3]['lowest_step'] == per[3]['lowest_step']
    torch.testing.assert_close(blk[0], per[0], rtol=0, atol=0)


@pytest.mark.parametrize('mfma', [MFMA_F32, MFMA_F16X3], ids=['f32', 'f16x3'])
@pytest.mark.parametrize('B', [50, 3])
@pytest.mark.parametrize('net', JAC_NETS, ids=_ids(JAC_NETS))
def test_r3_jac_primal_column_keeps_fwd_bits(net, B, mfma):
    """On the launch path inf_imblock_eval_exact takes f_x(x) from the JAC launch's primal column and recomputes z in
    the z-branch JAC launch's staging; inf_imblock_forward takes f_x(x) from the FWD kernel and z from its OM_RECOMP
    epilogue.  The primal column keeps the FWD kernel's bits, so both give the same z."""
    nx, nz = _nets(*net)
    x = _input(B, net[0])
    ev = _run(nx, nz, x, 'eval_exact', mfma, 0, False)
    fw = _run(nx, nz, x, 'forward', mfma, 0, False)
    assert {TAG_FWD, TAG_JAC} <= ev[4] and TAG_BLOCK not in ev[4], sorted(ev[4])
    assert TAG_FWD in fw[4] and not fw[4] & {TAG_JAC, TAG_BLOCK}, sorted(fw[4])
    print('R3 %s B %d mfma %d: nstep %d / %d, max |z eval_exact - z forward| %.3e' % (
        net, B, mfma, ev[3]['nstep'], fw[3]['nstep'], _maxdiff(ev[0], fw[0])))
    assert ev[3]['nstep'] == fw[3]['nstep']
    torch.testing.assert_close(ev[0], fw[0], rtol=0, atol=0)
