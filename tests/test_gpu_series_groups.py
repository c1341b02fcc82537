"""The fused conv nets' power series run in sample groups (INF_OPT_SERIES_GROUP) against the same series as one group.

A series is independent per sample, so the engine may run it as one complete chain of terms per group of samples, the
group's derivative-saving forward in front of its terms, every per-sample buffer (inputs, probes, the two taps buffers,
the derivative planes, the Neumann accumulator, the trace slab) sliced by pointer.  Each group launches on the kernel
family of the whole batch and its tiles do the whole batch's arithmetic, so the condition is equality bit for bit, not
a tolerance: every entry runs once with INF_SERIES_GROUP_OFF and once per forced group size on a NaN-filled workspace
(and NaN-filled LDS), and the outputs are compared with torch.equal.

Shapes: the CIFAR-10 model's 512-wide 3-1-3 Swish nets at B = 3 and B = 5 --
  (3, 32, 32) under INF_OPT_FUSED_K128 = 2 and 0, (12, 16, 16), (48, 8, 8) (the wide 32-pixel kernel);
group sizes 1, 2, B and B + 3 (2 gives 2 + 1 and 2 + 2 + 1: a short last group; B and B + 3 are one group);
1, 2 and 5 terms (1: only the closing conv_out term; even / odd: the Y / Y2 ping-pong and the serpentine parity, which
restart with every group).
Below 256 64-pixel tiles the launcher takes the 32-pixel variants whatever the policy, so at B = 3 and 5 both policies
of the 32x32 shape run those.  The 64-pixel kernel (policy 0, launch tag 502) and the 128-pixel kernel (policy 2, 532)
run in groups at the smallest batches that keep the 64-pixel layout at 32x32, 16 tiles per image: B = 17 for one net
(groups of 6: 6 + 6 + 5) and B = 9 for a pair (groups of 4: 4 + 4 + 1), an odd batch each, checked by the launch
profile; inf_imblock_eval at B = 17 on both schedules, where the x-branch planes (overlap 1) or the x-net's (overlap 0)
are saved by one whole-batch launch and read by the groups, so a group's slice must start at the layout's own stride.
The same on a ragged shape (3, 28, 28), whose planes are wider than H * W per sample.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OFF = _hip.INF_SERIES_GROUP_OFF
T = 6
V64_VJP, K128_VJP = 502, 532
# (imBlock index, (C, H, W), INF_OPT_FUSED_K128 or None for the default)
SHAPES = {
    's0_k128': (0, (3, 32, 32), 2),
    's0_k128_off': (0, (3, 32, 32), 0),
    's1': (2, (12, 16, 16), None),
    's2_wide': (4, (48, 8, 8), None),
}
TERMS = (1, 2, 5)
BATCHES = (3, 5)


@pytest.fixture(scope='module')
def model():
    arch = syn.CIFAR10
    m = build_flow(arch, 2)
    m.load_state_dict(syn.make_state_dict(arch, 0, power_iters=5), strict=True)
    return m.to(DEV).eval()


def _inputs(shape, B):
    g = torch.Generator().manual_seed(1000 + B + shape[0])
    x = (torch.randn(B, *shape, generator=g) * 0.5).to(DEV)
    z = (torch.randn(B, *shape, generator=g) * 0.5).to(DEV)
    eps = [torch.sign(torch.randn(B, *shape, generator=g)).to(DEV) for _ in range(2)]
    return x, z, eps


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _coeff(n):
    return np.array([(-1) ** (k + 1) / k for k in range(1, n + 1)], dtype=np.float32)


class _Options:
    """Sets INF_OPT_SERIES_GROUP (and optionally FUSED_K128 / EVAL_OVERLAP) on the nets, restoring them on exit."""

    def __init__(self, nets, group, k128=None, overlap=None):
        self.nets, self.want = nets, {_hip.INF_OPT_SERIES_GROUP: group}
        if k128 is not None:
            self.want[_hip.INF_OPT_FUSED_K128] = k128
        if overlap is not None:
            self.want[_hip.INF_OPT_EVAL_OVERLAP] = overlap

    def __enter__(self):
        self.prev = [{o: n.set_option(o, v) for o, v in self.want.items()} for n in self.nets]

    def __exit__(self, *exc):
        for n, prev in zip(self.nets, self.prev):
            for o, v in prev.items():
                n.set_option(o, v)


def _poisoned(nets, nbytes, stream):
    ws = _hip.workspace(torch.device(DEV), nbytes)
    ws.fill_(255)
    _hip.check(nets[0].lib.inf_debug_poison_lds(stream), 'poison_lds')
    return ws


def _series_single(nx, nz, stream, x, z, eps, n):
    B = x.shape[0]
    out = torch.empty(B, device=DEV)
    ws = _poisoned((nx,), nx.ws_bytes(B), stream)
    _hip.check(nx.lib.inf_logdet_series(nx.handle, _hip.ptr(x), _hip.ptr(eps[0]), _fptr(_coeff(n)), n, _hip.ptr(out), B,
                                        _hip.ptr(ws), ws.numel(), stream), 'series')
    return {'logdet': out}


def _series_pair(nx, nz, stream, x, z, eps, n):
    B = x.shape[0]
    out = torch.empty(2, B, device=DEV)
    ws = _poisoned((nx, nz), 2 * max(nx.ws_bytes(B), nz.ws_bytes(B)), stream)
    _hip.check(nx.lib.inf_logdet_series_pair(nx.handle, _hip.ptr(x), _hip.ptr(eps[0]), nz.handle, _hip.ptr(z),
                                             _hip.ptr(eps[1]), _fptr(_coeff(n)), n, _hip.ptr(out[0]), _hip.ptr(out[1]),
                                             B, _hip.ptr(ws), ws.numel(), stream), 'series_pair')
    return {'logdet': out}


def _neumann_pair(nx, nz, stream, x, z, eps, n):
    B = x.shape[0]
    nco = np.array([(-1) ** k * (1.0 if k < 4 else 0.5) for k in range(n + 1)], dtype=np.float32)
    wa, wb = torch.empty_like(x), torch.empty_like(z)
    ws = _poisoned((nx, nz), 2 * max(nx.ws_bytes(B), nz.ws_bytes(B)), stream)
    _hip.check(nx.lib.inf_neumann_vector_pair(nx.handle, _hip.ptr(x), _hip.ptr(eps[0]), nz.handle, _hip.ptr(z),
                                              _hip.ptr(eps[1]), _fptr(nco), n, _hip.ptr(wa), _hip.ptr(wb), B,
                                              _hip.ptr(ws), ws.numel() // 2 * 2, stream), 'neumann_pair')
    return {'wa': wa, 'wb': wb}


def _imblock_eval(nx, nz, stream, x, z, eps, n, eps_forward=1e-6):
    B = x.shape[0]
    zo = torch.empty_like(x)
    out = torch.empty(2, B, device=DEV)
    st = _hip.BroydenStats()
    ws = _poisoned((nx, nz), nx.ws_bytes(B, T) + nz.ws_bytes(B, 1) + nx.ws_bytes(B, 1), stream)
    _hip.check(nx.lib.inf_imblock_eval(nx.handle, nz.handle, _hip.ptr(x), _hip.ptr(zo), _hip.ptr(eps[0]), _hip.ptr(eps[1]),
                                       _fptr(_coeff(n)), n, _hip.ptr(out[0]), _hip.ptr(out[1]), B, T, eps_forward,
                                       ctypes.byref(st), _hip.ptr(ws), ws.numel(), stream), 'inf_imblock_eval')
    torch.cuda.synchronize()
    # (log p's step is logdet_x - logdet_z: both terms must match; the series lengths are the caller's n)
    return {'z': zo, 'logdet': out, 'steps': torch.tensor([st.nstep, st.lowest_step, n])}


def _groups_match(entry, nets, stream, x, z, eps, n, groups, k128=None, overlap=None):
    """`entry` with the series as one group, then under every forced group size: finite, and bit for bit the same."""
    def run(group):
        with _Options(nets, group, k128, overlap):
            res = entry(*nets, stream, x, z, eps, n)
            torch.cuda.synchronize()
        return {k: v.cpu() for k, v in res.items()}
    ref = run(OFF)
    for k, v in ref.items():
        assert torch.isfinite(v.float()).all(), k
    for group in groups:
        got = run(group)
        for k, v in ref.items():
            assert torch.equal(got[k], v), (entry.__name__, 'group', group, k, (got[k].float() - v.float()).abs().max())


def _block_nets(model, case, B):
    idx, shape, k128 = SHAPES[case]
    blk = imblocks(model)[idx]
    x, z, eps = _inputs(shape, B)
    nx, nz, stream = blk._native(x)
    return (nx, nz), stream, x, z, eps, k128


@pytest.mark.parametrize('n', TERMS)
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('case', sorted(SHAPES))
@pytest.mark.parametrize('entry', [_series_single, _series_pair, _neumann_pair], ids=lambda f: f.__name__.strip('_'))
def test_series_entries_in_groups(model, entry, case, B, n):
    """inf_logdet_series, inf_logdet_series_pair and inf_neumann_vector_pair: groups of 1, 2, B and B + 3 samples."""
    nets, stream, x, z, eps, k128 = _block_nets(model, case, B)
    _groups_match(entry, nets, stream, x, z, eps, n, (1, 2, B, B + 3), k128)


@pytest.mark.parametrize('n', TERMS)
@pytest.mark.parametrize('overlap', [0, 1])
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('case', sorted(SHAPES))
def test_imblock_eval_in_groups(model, case, B, overlap, n):
    """inf_imblock_eval on the sequential pair schedule (overlap 0) and with the x-branch series on the side stream
    (overlap 1, its planes saved by the whole-batch x_embed launch): z, both log-dets (log p's step), the solve's steps
    and the series length."""
    nets, stream, x, z, eps, k128 = _block_nets(model, case, B)
    _groups_match(_imblock_eval, nets, stream, x, z, eps, n, (1, 2, B, B + 3), k128, overlap)


def _vjp_launches(entry, nets, stream, x, z, eps, n, group, k128, overlap=None):
    """Launch count per fused VJP tag (5x2) of one run of `entry` under the forced group."""
    with _Options(nets, group, k128, overlap):
        _hip.profile_begin(2000)
        try:
            entry(*nets, stream, x, z, eps, n)
            torch.cuda.synchronize()
        finally:
            launches = {s['tag']: s['launches'] for s in _hip.profile_end()}
    return {t: c for t, c in launches.items() if t % 10 == 2 and 500 <= t < 600}


@pytest.mark.parametrize('k128,tag', [(0, V64_VJP), (2, K128_VJP)], ids=['64px', '128px'])
@pytest.mark.parametrize('entry,B,group', [(_series_single, 17, 6), (_series_pair, 9, 4), (_neumann_pair, 9, 4)],
                         ids=['single_b17', 'pair_b9', 'neumann_pair_b9'])
def test_groups_on_the_64_and_128_pixel_kernels(model, entry, B, group, k128, tag):
    """The smallest batches that keep the 64-pixel layout at 32x32 (256 64-pixel tiles: B = 16 for one net, 8 for a
    pair; one more for an odd batch), under policy 0 (the 64-pixel kernel) and 2 (the 128-pixel kernel): the groups,
    6 + 6 + 5 and 4 + 4 + 1, alone would fall below that grid and run on the whole batch's kernel all the same (launch
    profile: every VJP launch carries the kernel's tag, 3 groups x 5 terms of them)."""
    nets, stream, x, z, eps, _ = _block_nets(model, 's0_k128', B)
    _groups_match(entry, nets, stream, x, z, eps, 5, (group, 1), k128)
    assert _vjp_launches(entry, nets, stream, x, z, eps, 5, group, k128) == {tag: 15}


@pytest.mark.parametrize('k128,tag', [(0, V64_VJP), (2, K128_VJP)], ids=['64px', '128px'])
@pytest.mark.parametrize('overlap', [0, 1])
def test_imblock_eval_groups_read_whole_batch_planes(model, overlap, k128, tag):
    """inf_imblock_eval at 32x32, B = 17, groups of 6 and of 1: the x_embed launch saves the x-net's planes for the whole
    batch in the 64-pixel layout and every group of its series reads its slice of them (a wrong plane stride shows
    here and nowhere else); 2 x 3 x 5 VJP launches of the kernel's tag with overlap 1, 3 x 5 pair launches with 0."""
    nets, stream, x, z, eps, _ = _block_nets(model, 's0_k128', 17)
    _groups_match(_imblock_eval, nets, stream, x, z, eps, 5, (6, 1), k128, overlap)
    assert _vjp_launches(_imblock_eval, nets, stream, x, z, eps, 5, 6, k128, overlap) == {tag: 30 if overlap else 15}


def test_ragged_shape_in_groups():
    """(3, 28, 28), which tiles with dead columns: the derivative planes hold hidden x tiles x tile width floats per
    sample, more than hidden x H x W.  The series entries save the planes per group; inf_imblock_eval saves the x-net's
    once for the whole batch, so its groups' slices must start at that stride."""
    from lib.layers.base import InducedNormConv2d, Swish
    C, H, W, B = 3, 28, 28, 5
    torch.manual_seed(3)
    conv = lambda a, b, k: InducedNormConv2d(a, b, k, 1, k // 2, coeff=0.9, atol=1e-3, rtol=1e-3)
    seqs = []
    for _ in range(2):
        seq = torch.nn.Sequential(Swish(), conv(C, 512, 3), Swish(), conv(512, 512, 1), Swish(), conv(512, C, 3)).to(DEV)
        with torch.no_grad():
            seq(torch.zeros(1, C, H, W, device=DEV))
        seqs.append(seq)
    x, z, eps = _inputs((C, H, W), B)
    stream = _hip.stream_of(x)
    nets = tuple(_hip.native_net(s, x.shape[1:], x.device) for s in seqs)
    for n in nets:
        n.refresh_if_needed(stream)
    for entry in (_series_single, _series_pair, _neumann_pair):
        _groups_match(entry, nets, stream, x, z, eps, 5, (1, 2), None)
    for overlap in (0, 1):
        _groups_match(_imblock_eval, nets, stream, x, z, eps, 5, (1, 2), None, overlap)


def test_training_step_in_groups(model):
    """One training forward + backward of the 32x32 imBlock on the engine gradients (B = 3, a fixed 5-term Neumann
    series: inf_neumann_vector_pair feeds the surrogate's gradients): z, log p, the input's and every parameter's
    gradient with groups of 2 (2 + 1) against one group."""
    from lib.layers import set_probe_mode
    B = 3
    x0, _, _ = _inputs((3, 32, 32), B)
    pristine = copy.deepcopy(imblocks(model)[0]).train()
    pristine.n_power_series = 5

    def step(group):
        blk = copy.deepcopy(pristine)
        x = x0.clone().requires_grad_(True)
        nets = blk._native(x.detach())[:2]
        set_probe_mode('device', seed=77)
        np.random.seed(5)
        torch.manual_seed(5)
        try:
            with _Options(nets, group):
                _hip.workspace(torch.device(DEV), 1 << 20).fill_(255)
                zt, logp = blk(x, torch.zeros(B, 1, device=DEV))
                (0.1 * zt.sum() + logp.sum()).backward()
                torch.cuda.synchronize()
        finally:
            set_probe_mode('reference')
        assert blk.__dict__.get('_engine_grads_ok')
        out = {'z': zt.detach().cpu(), 'logp': logp.detach().cpu(), 'gx': x.grad.cpu()}
        for name, p in blk.named_parameters():
            if p.grad is not None:
                out['g:' + name] = p.grad.cpu()
        return out

    ref = step(OFF)
    got = step(2)
    assert sum(k.startswith('g:') for k in ref) >= 6 and set(got) == set(ref)
    for k, v in ref.items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(got[k], v), (k, (got[k] - v).abs().max())
