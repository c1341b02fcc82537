"""The limited-memory Broyden update (broyden.hip launch_broyden_update, through inf_broyden_update) at every size
its launcher dispatches on, against broyden.py:174-181 restated in fp64 (oracle _rmatvec / _matvec on the fp32 inputs):

  * small      d <= 32:            broyden_small_d_kernel<2 | 6 | 8> or the generic broyden_small_kernel      tag 715
  * fused      1 to 4 chunks of 1024: broyden_fused_kernel, one workgroup per sample                            tag 716
  * chunked    5 to 31 chunks:     broyden_p1..p4, every block re-sums the chunk partials                      tags 710-713
  * pre-summed 32 chunks or more:  broyden_p1..p4 with br_sum_chunks in between (nsum = 1)                     + tag 714

and the per-sample `active` mask of the chunked and pre-summed kernels through an imBlock under the per-sample stopping
rule.  Before every engine call the workspace and every CU's LDS are filled with NaN; the kernels that ran are read from
the launch profile.  Tolerances are test_gpu_edges.py::test_broyden_update_small_d_matches_reference_algebra's."""
import numpy as np
import pytest
import torch

from lib import _hip, synthetic as syn
from lib.configs import build_flow, imblocks
from lib.density import image_logpx
from lib.layers import set_convergence, set_probe_shard
from oracle.inflow_oracle import _matvec, _rmatvec

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CH = 1024                      # broyden.hip BR_CH


def _regime(d):
    nchunk = (d + CH - 1) // CH
    return 'small' if d <= 32 else 'fused' if nchunk <= 4 else 'chunked' if nchunk < 32 else 'presummed'


def _expected_tags(d, nstep):
    r = _regime(d)
    if r == 'small':
        return {715}
    if r == 'fused':
        return {716}
    tags = {711, 712, 713} | ({710} if nstep > 1 else set())     # (no old columns at nstep 1: broyden_p1 has no work)
    return tags | ({714} if r == 'presummed' else set())


def _boundary(d):
    """The element indices at which a chunked kernel can go wrong: both ends, the first chunk boundary, the first
    element of the last chunk."""
    last = ((d - 1) // CH) * CH
    return sorted({i for i in (0, CH - 1, CH, last, d - 1) if 0 <= i < d})


def _inputs(d, T, nstep, B, degenerate=None):
    """fp32 inputs as the small-d test draws them (columns 0.3 N(0, 1), dg += 2 dx to keep v^T dg away from 0, the
    columns j >= nstep zero).  d > 32: at the _boundary indices every tensor's magnitude is raised by half its standard
    deviation and then enlarged by d^(1/4), so that one of them dropped from a sum moves the result by far more than the
    tolerance (_guard).  The factor: a dot of two independent vectors is a sum of d terms of either sign, about sqrt(d)
    large; an element enlarged by d^(1/4) in both carries sqrt(d) itself, as much as all the others together.  At
    sqrt(d) / 4 the five enlarged elements carry d / 16 each and are all that is left of every sum at large d: fp32
    arithmetic in the kernels' order (fp64 dots rounded to fp32, fp32 chains), emulated on the CPU, then misses this
    tolerance by up to 1.9x at d >= 31745, where with d^(1/4) it stays below 6 % of it in every case."""
    gen = torch.Generator().manual_seed(1000003 * T + 100 * d + nstep + 7 * B)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    U0, VT0 = rnd(T, B, d) * 0.3, rnd(T, B, d) * 0.3
    dx, dg, gx, x = rnd(B, d), rnd(B, d), rnd(B, d), rnd(B, d)
    dg = dg + 2.0 * dx
    spiked = _boundary(d) if d > 32 else []
    if spiked:
        f = float(np.float32(d ** 0.25))
        for t, scale in ((U0, 0.3), (VT0, 0.3), (dx, 1.0), (dg, 1.0), (gx, 1.0)):
            v = t[..., spiked]
            t[..., spiked] = f * torch.where(v < 0, -1.0, 1.0) * (0.5 * scale + v.abs())    # none of them near 0
    U0[nstep:] = 0.0
    VT0[nstep:] = 0.0
    if degenerate is not None:
        dx[degenerate] = 0.0
        dg[degenerate] = 0.0
    return U0, VT0, dx, dg, gx, x, spiked


def _reference(U0, VT0, dx, dg, gx, nstep):
    """broyden.py:174-181 in fp64: (u, vT) of column m = nstep - 1, NaN scrubbed to 0 (:177-178), and the update."""
    m = nstep - 1
    Us, VTs = U0.permute(1, 2, 0), VT0.permute(1, 0, 2)          # (B, d, T), (B, T, d) views
    vT = _rmatvec(Us[:, :, :m], VTs[:, :m], dx)
    u = (dx - _matvec(Us[:, :, :m], VTs[:, :m], dg)) / torch.einsum('bi, bi -> b', vT, dg)[:, None]
    vT = torch.where(vT != vT, torch.zeros_like(vT), vT)
    u = torch.where(u != u, torch.zeros_like(u), u)
    Us = torch.cat([Us[:, :, :m], u[:, :, None]], 2)
    VTs = torch.cat([VTs[:, :m], vT[:, None]], 1)
    return u, vT, -_matvec(Us, VTs, gx)


def _tols(ref, spiked):
    """rtol 1e-4, atol 1e-5 max|ref| with the maximum taken over the elements that were not enlarged."""
    keep = torch.ones(ref.shape[-1], dtype=torch.bool)
    keep[spiked] = False
    return dict(rtol=1e-4, atol=1e-5 * float(ref[..., keep].abs().max()))


def _guard(ins64, nstep, update, spiked, skip_sample=None):
    """Input check, on the reference alone: with any one boundary index zeroed in every input (what a kernel that drops
    the element from its sums computes), the fp64 update of every sample moves by at least 10x the tolerance at some
    other element."""
    tol = _tols(update, spiked)
    bound = 10.0 * (tol['atol'] + tol['rtol'] * update.abs())
    for i in spiked:
        saved = [t[..., i].clone() for t in ins64]
        for t in ins64:
            t[..., i] = 0.0
        moved = _reference(*ins64, nstep)[2]
        for t, s in zip(ins64, saved):
            t[..., i] = s
        far = (moved - update).abs() >= bound
        far[:, i] = False
        for b in range(update.shape[0]):
            if b != skip_sample:
                assert far[b].any(), 'dropping element %d would go unnoticed in sample %d' % (i, b)


def _run(U0, VT0, dx, dg, gx, x, T, nstep, poison_cols):
    lib = _hip.load()
    B, d = dx.shape
    U, VT = U0.clone(), VT0.clone()
    if poison_cols:
        U[nstep:] = float('nan')
        VT[nstep:] = float('nan')
    U, VT = U.to(DEV), VT.to(DEV)
    args = [t.contiguous().to(DEV) for t in (dx, dg, gx, x)]
    upd, xn, dxn = (torch.empty(B, d, device=DEV) for _ in range(3))
    ws = torch.empty(lib.inf_broyden_workspace_bytes(B, d, T), dtype=torch.uint8, device=DEV)
    stream = _hip.stream_of(U)
    ws.fill_(255)
    _hip.check(lib.inf_debug_poison_lds(stream), 'poison_lds')
    _hip.profile_begin(100)
    try:
        _hip.check(lib.inf_broyden_update(_hip.ptr(U), _hip.ptr(VT), *[_hip.ptr(t) for t in args], _hip.ptr(upd),
                                          _hip.ptr(xn), _hip.ptr(dxn), B, d, T, nstep, _hip.ptr(ws), ws.numel(),
                                          stream), 'inf_broyden_update')
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
    return (U.cpu(), VT.cpu(), upd.cpu(), xn.cpu(), dxn.cpu()), tags


def _check_case(d, T, nstep, B, degenerate=None):
    U0, VT0, dx, dg, gx, x, spiked = _inputs(d, T, nstep, B, degenerate)
    m = nstep - 1
    ins64 = [t.double() for t in (U0, VT0, dx, dg, gx)]
    u, vT, update = _reference(*ins64, nstep)
    assert torch.isfinite(update).all()
    # with one stored column and a degenerate sample, that sample's update is -(-gx): nothing is summed for it
    _guard(ins64, nstep, update, spiked, skip_sample=degenerate if nstep == 1 else None)

    zero, tags = _run(U0, VT0, dx, dg, gx, x, T, nstep, False)
    pois, _ = _run(U0, VT0, dx, dg, gx, x, T, nstep, True)
    assert tags == _expected_tags(d, nstep), (sorted(tags), _regime(d))
    for a, b in zip(zero[2:], pois[2:]):                 # the columns j >= nstep are never read
        assert torch.equal(a, b)
    assert torch.equal(zero[0][:nstep], pois[0][:nstep]) and torch.equal(zero[1][:nstep], pois[1][:nstep])
    U, VT, upd, xn, dxn = zero
    assert torch.equal(U[:m], U0[:m]) and torch.equal(VT[:m], VT0[:m])      # the old columns stay as they were
    for name, got, ref in (('U_m', U[m], u), ('VT_m', VT[m], vT), ('update', upd, update),
                           ('x_next', xn, x.double() + update)):
        tol = _tols(update if name == 'x_next' else ref, spiked)
        err = (got.double() - ref).abs()
        print('%s d %d T %d nstep %d: max err %.3g (atol %.3g)' % (name, d, T, nstep, err.max().item(), tol['atol']))
        torch.testing.assert_close(got.double(), ref, msg=lambda s: name + ': ' + s, **tol)
    torch.testing.assert_close(dxn, xn - x, rtol=0, atol=0)
    return zero, (U0, VT0, dx, dg, gx, x)


T30 = 30
SMALL = [(d, T30, n) for d in (1, 3, 5, 32) for n in (1, 2, 30)] + [(7, 64, 64), (6, 64, 64)]
FUSED = ([(33, T30, n) for n in (1, 2, 30)] +
         [(d, T30, n) for d in (1000, 1024, 1025, 3072, 4000, 4096) for n in (1, 2, 30)] + [(1025, 64, 64)])
CHUNKED = [(d, T30, n) for d in (4097, 24576, 31744) for n in (1, 7, 30)]
PRESUMMED = [(d, T30, n) for d in (31745, 32768, 66000, 196608) for n in (1, 2, 30)] + [(66000, 64, 64)]
CASES = ([c + (3,) for c in SMALL + FUSED + CHUNKED + PRESUMMED] +
         [(5, T30, 7, 300),                                   # more than one block of the thread-per-sample kernels
          (3, T30, 30, 1), (3072, T30, 30, 1), (4097, T30, 7, 1), (31745, T30, 2, 1)])


def test_cases_cover_every_regime():
    assert {_regime(c[0]) for c in CASES} == {'small', 'fused', 'chunked', 'presummed'}
    assert [_regime(d) for d in (32, 33, 4096, 4097, 31744, 31745)] == ['small', 'fused', 'fused', 'chunked',
                                                                         'chunked', 'presummed']


@pytest.mark.parametrize('d,T,nstep,B', CASES)
def test_broyden_update_matches_reference_algebra(d, T, nstep, B):
    """U_m, VT_m, update and x_next within rtol 1e-4 and atol 1e-5 max|ref| of the fp64 algebra (max|ref| over the
    elements that were not enlarged, which is the stricter reading), dx_next bitwise x_next - x, the old columns
    untouched, the result with NaN in the columns j >= nstep bitwise the zero-filled one, and the launch profile showing
    the regime's kernels and no others.  The inputs pass _guard first: dropping any one boundary element would move the
    reference by 10x the tolerance."""
    _check_case(d, T, nstep, B)


@pytest.mark.parametrize('d,T,nstep', [(5, T30, 7), (6, T30, 7), (1025, T30, 7), (4097, T30, 7), (31745, T30, 7),
                                       (4097, T30, 1)])
def test_degenerate_sample_is_scrubbed(d, T, nstep):
    """One sample with dx = dg = 0 exactly: v^T dg = 0, u = 0 / 0, and broyden.py:177-178 scrubs the NaN to 0.  Its
    U_m and VT_m rows are exactly 0, its update is finite and the reference's from the remaining columns (checked by
    _check_case with the whole batch), and the other samples' results are bitwise those of the run in which the sample
    is an ordinary one."""
    B, deg = 3, 1
    m = nstep - 1
    (U, VT, upd, xn, dxn), (U0, VT0, dx, dg, gx, x) = _check_case(d, T, nstep, B, degenerate=deg)
    assert (U[m, deg] == 0).all() and (VT[m, deg] == 0).all()
    assert torch.isfinite(upd[deg]).all() and torch.isfinite(xn[deg]).all()
    U0n, VT0n, dxn_, dgn, gxn, xn_, _ = _inputs(d, T, nstep, B)
    others = [b for b in range(B) if b != deg]
    for a, b in zip((dx, dg, gx, x), (dxn_, dgn, gxn, xn_)):
        assert torch.equal(a[others], b[others])
    plain, _ = _run(U0n, VT0n, dxn_, dgn, gxn, xn_, T, nstep, False)
    for got, ref in zip((U[m], VT[m], upd, xn, dxn), (plain[0][m], plain[1][m], plain[2], plain[3], plain[4])):
        assert torch.equal(got[others], ref[others])


# ---- the per-sample mask on the chunked and the pre-summed kernels ---------------------------------------------------

def _flow_run(arch, sd, x, seed, lo=None, hi=None, n=None):
    m = build_flow(arch, x.shape[0])
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    if lo is not None:
        set_probe_shard(lo, hi, n)
    xd = x.to(DEV)
    _hip.check(_hip.load().inf_debug_poison_lds(_hip.stream_of(xd)), 'poison_lds')
    _hip.profile_begin(50000)
    try:
        np.random.seed(seed)
        torch.manual_seed(seed)
        bpd, logpx, _ = image_logpx(m, xd, arch['nvals'])
        torch.cuda.synchronize()
    finally:
        tags = {s_['tag'] for s_ in _hip.profile_end()}
        set_probe_shard()
    return logpx.view(-1).cpu().numpy().astype(np.float64), [dict(b.last_broyden) for b in imblocks(m)], tags


@pytest.mark.parametrize('hw,presummed', [(40, False), (104, True)])
def test_per_sample_mask_on_chunked_kernels(hw, presummed):
    """One imBlock flow at d = 3 x 40 x 40 = 4800 (5 chunks) and d = 3 x 104 x 104 = 32448 (32 chunks, pre-summed), B = 3
    under the per-sample stopping rule, against its three shards of one sample each: sample_nstep and sample_lowest_step
    exact, per-sample log p within 2e-4.  Sample 1 is squeezed into [0.45, 0.55] (after the logit transform a small
    input: the reference's solver, run on it alone, stops after 3 steps) and sample 2 into [0.9, 1] (5 steps) beside the
    plain sample 0 (4 steps); the samples are asserted to stop at different steps, so broyden_p1..p4 and br_sum_chunks
    run with stopped samples in the batch (p1..p3 and the pre-sum return early for them, p4 writes x_next = x)."""
    arch = dict(syn.CIFAR10_SMALL, n_blocks=[1], input_size=(3, hw, hw))
    B, seed = 3, 3
    sd = syn.make_state_dict(arch, 0)
    x = syn.image_batch(B, input_size=arch['input_size'], seed=seed)
    x[1] = 0.45 + 0.1 * x[1]
    x[2] = 0.9 + 0.1 * x[2]
    set_convergence('per_sample')
    try:
        lp, st, tags = _flow_run(arch, sd, x, seed)
        parts = [_flow_run(arch, sd, x[b:b + 1], seed, b, b + 1, B) for b in range(B)]
    finally:
        set_convergence('global')
    assert {710, 711, 712, 713} <= tags and (714 in tags) == presummed, sorted(tags)
    assert not tags & {715, 716}, sorted(tags)
    assert len(st) == 1 and st[0]['convergence'] == 'per_sample'
    nsteps = st[0]['sample_nstep']
    print('sample_nstep', nsteps, 'lowest', st[0]['sample_lowest_step'])
    assert len(set(nsteps)) > 1, nsteps                  # otherwise no launch ever saw a stopped sample
    assert nsteps == [p[1][0]['sample_nstep'][0] for p in parts]
    assert st[0]['sample_lowest_step'] == [p[1][0]['sample_lowest_step'][0] for p in parts]
    lp_sh = np.concatenate([p[0] for p in parts])
    print('max |dlogp| %.3g nats' % np.abs(lp_sh - lp).max())
    assert np.abs(lp_sh - lp).max() <= 2e-4
