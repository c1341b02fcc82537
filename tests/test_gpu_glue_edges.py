"""The small solver and glue kernels through the C ABI at the sizes where they take another branch, against fp64 torch
on the CPU: the line-search trial point (broyden.hip line_step_kernel), ActNorm (glue.hip actnorm_kernel: the float4
path, the scalar path for hw % 4 != 0 or pointers off a 16-byte boundary, the channel loop for C > 256), the logit
transform, the standard-normal log-prob, squeeze and the Rademacher generator.

Values: test_gpu_parity.py's _close (2e-5 of max(1, max|ref|)).  Per-sample sums: the fp64 sum of the same terms
evaluated in fp32 on the CPU, within 1e-6 relative; every term of a sum has the sign of logp_in's contribution, so
nothing cancels and a relative bound is meaningful."""
import numpy as np
import pytest
import torch

from lib import _hip

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _close(a, b, rel=2e-5):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    scale = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item()
    assert torch.isfinite(a).all()
    assert err <= rel * scale, 'max abs err %g > %g' % (err, rel * scale)


def _sums_close(got, ref):
    got, ref = got.detach().double().cpu().view(-1), ref.double().view(-1)
    err = ((got - ref).abs() / ref.abs()).max().item()
    assert torch.isfinite(got).all()
    assert err <= 1e-6, 'max relative err %g' % err


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _poison_lds(t):
    """NaN into every CU's LDS ahead of an engine call on t's stream (the sums' reduction scratch lives there)."""
    _hip.check(_hip.load().inf_debug_poison_lds(_hip.stream_of(t)), 'poison_lds')


# ---- inf_broyden_line_step -------------------------------------------------------------------------------------------

@pytest.mark.parametrize('step', [1.0, 0.5, 0.3, 1e-3])
@pytest.mark.parametrize('n', [1, 255, 257, 100003])
def test_line_step_rounds_product_and_sum_separately(n, step):
    """x_est = x0 + step * update with the product and the sum each rounded to fp32 (broyden.py:79,94,99 are two tensor
    ops), dx = x_est - x0: bitwise the CPU's fp32 result.  For a step that is no power of two the inputs hold, at the
    first and the last element, values at which a fused multiply-add (the product kept exact: computed in fp64 and rounded
    once) gives another fp32 result, asserted on the CPU before the device runs; with step 1 or 0.5 the product is exact
    and the two forms cannot differ."""
    g = _gen(1000 * n + int(step * 1000))
    pool_x, pool_u = torch.randn(n + 4096, generator=g), torch.randn(n + 4096, generator=g)
    s32 = torch.tensor(step, dtype=torch.float32)
    two_step = lambda x, u: x + s32 * u
    fma = lambda x, u: (x.double() + s32.double() * u.double()).float()
    x0, upd = pool_x[:n].clone(), pool_u[:n].clone()
    sensitive = float(np.log2(step)) != round(float(np.log2(step)))
    if sensitive:
        cand = torch.nonzero(two_step(pool_x[n:], pool_u[n:]) != fma(pool_x[n:], pool_u[n:])).view(-1) + n
        assert cand.numel() >= 2
        for pos, c in ((0, cand[0]), (n - 1, cand[1])):
            x0[pos], upd[pos] = pool_x[c], pool_u[c]
    ref = two_step(x0, upd)
    differs = ref != fma(x0, upd)
    assert bool(differs.any()) == sensitive
    if sensitive:
        assert differs[0] and differs[n - 1]
    lib = _hip.load()
    xd, ud = x0.to(DEV), upd.to(DEV)
    xe, dx = torch.full((n + 1,), 7.0, device=DEV), torch.full((n + 1,), 7.0, device=DEV)
    _poison_lds(xd)
    _hip.check(lib.inf_broyden_line_step(_hip.ptr(xd), _hip.ptr(ud), float(step), _hip.ptr(xe), _hip.ptr(dx), n,
                                         _hip.stream_of(xd)), 'inf_broyden_line_step')
    torch.cuda.synchronize()
    assert torch.equal(xe[:n].cpu(), ref)
    assert torch.equal(dx[:n].cpu(), ref - x0)
    assert xe[n].item() == 7.0 and dx[n].item() == 7.0          # nothing written past n


# ---- inf_actnorm_forward ---------------------------------------------------------------------------------------------

def _actnorm(x, w, b, lin, want_logp=True):
    lib = _hip.load()
    B, C, hw = x.shape
    y = torch.empty_like(x)
    lout = torch.full((B,), float('nan'), device=DEV) if want_logp else None
    _poison_lds(x)
    _hip.check(lib.inf_actnorm_forward(_hip.ptr(x), _hip.ptr(y), _hip.ptr(w), _hip.ptr(b), _hip.ptr(lin),
                                       _hip.ptr(lout), B, C, hw, _hip.stream_of(x)), 'inf_actnorm_forward')
    torch.cuda.synchronize()
    return y, lout


def _actnorm_inputs(B, C, hw):
    g = _gen(100 * C + hw + B)
    x = torch.randn(B, C, hw, generator=g)
    w = torch.rand(C, generator=g) * 0.25 + 0.05           # positive: the log-det terms all have one sign
    b = torch.rand(C, generator=g) * 0.6 - 0.3
    lin = -torch.rand(B, generator=g) * 5.0 - 1.0          # negative, as is -hw sum(w): nothing cancels
    return x, w, b, lin


def _actnorm_check(x, w, b, lin, y, lout):
    B, C, hw = x.shape
    y_ref = (x.double() + b.double().view(1, C, 1)) * torch.exp(w.double()).view(1, C, 1)
    _close(y, y_ref)
    if lout is not None:
        ld = (w.double() * hw).sum()
        _sums_close(lout, (lin.double() if lin is not None else torch.zeros(B, dtype=torch.float64)) - ld)


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('with_logp', [False, True])
@pytest.mark.parametrize('C,hw', [(3, 9), (5, 25), (3, 4), (7, 1028), (300, 1), (12, 256)])
def test_actnorm_shapes(C, hw, with_logp, B):
    """y = (x + bias_c) exp(weight_c) and logp_out = logp_in - hw sum_c weight_c at hw % 4 != 0 (9, 25, 1: the scalar
    path, a thread's four elements crossing channels), hw = 4 and 1028 (float4; 7 x 1028 takes several blocks per
    sample with a ragged last one), C = 300 (more channels than the block's threads in the log-det sum) and (12, 256);
    logp_in null and given."""
    x, w, b, lin = _actnorm_inputs(B, C, hw)
    if not with_logp:
        lin = None
    y, lout = _actnorm(x.to(DEV), w.to(DEV), b.to(DEV), lin.to(DEV) if lin is not None else None)
    _actnorm_check(x, w, b, lin, y, lout)


@pytest.mark.parametrize('C,hw', [(3, 4), (12, 256)])
def test_actnorm_unaligned_pointers(C, hw):
    """x and y one float off a 16-byte boundary (slices of larger tensors) at hw % 4 == 0: the launcher must leave the
    float4 path.  The result is the aligned call's bit for bit (both evaluate (x + b) * expf(w) per element), the
    float before y stays untouched, and the call without logp_out writes only y."""
    B = 3
    x, w, b, lin = _actnorm_inputs(B, C, hw)
    wd, bd, lind = w.to(DEV), b.to(DEV), lin.to(DEV)
    y_al, lout_al = _actnorm(x.to(DEV), wd, bd, lind)
    big_x = torch.zeros(B * C * hw + 1, device=DEV)
    big_y = torch.full((B * C * hw + 1,), 7.0, device=DEV)
    xs, ys = big_x[1:].view(B, C, hw), big_y[1:].view(B, C, hw)
    xs.copy_(x)
    assert xs.data_ptr() % 16 == 4 and ys.data_ptr() % 16 == 4
    lib = _hip.load()
    lout = torch.empty(B, device=DEV)
    _poison_lds(xs)
    _hip.check(lib.inf_actnorm_forward(_hip.ptr(xs), _hip.ptr(ys), _hip.ptr(wd), _hip.ptr(bd), _hip.ptr(lind),
                                       _hip.ptr(lout), B, C, hw, _hip.stream_of(xs)), 'inf_actnorm_forward')
    torch.cuda.synchronize()
    _actnorm_check(x, w, b, lin, ys, lout)
    assert torch.equal(ys, y_al) and torch.equal(lout, lout_al)
    assert big_y[0].item() == 7.0
    y2, _ = _actnorm(x.to(DEV), wd, bd, None, want_logp=False)
    assert torch.equal(y2, y_al)


# ---- inf_logit_forward / inf_normal_logprob ----------------------------------------------------------------------------

@pytest.mark.parametrize('with_logp', [False, True])
@pytest.mark.parametrize('per', [1, 255, 257, 3071])
def test_logit_sizes(per, with_logp):
    """y = logit(alpha + (1 - 2 alpha) x) and logp_out = logp_in - sum(-log(s - s^2) + log(1 - 2 alpha)) at per-sample
    sizes below, at and around the block's 256 threads, and 3071 (twelve strides less one)."""
    lib = _hip.load()
    B, alpha = 3, 0.05
    g = _gen(per)
    x = torch.rand(B, per, generator=g) * 0.98 + 0.01
    lin = (-torch.rand(B, generator=g) * 5.0 - 1.0) if with_logp else None
    xd = x.to(DEV)
    y, lout = torch.empty_like(xd), torch.full((B,), float('nan'), device=DEV)
    lind = lin.to(DEV) if with_logp else None
    _poison_lds(xd)
    _hip.check(lib.inf_logit_forward(_hip.ptr(xd), _hip.ptr(y), _hip.ptr(lind), _hip.ptr(lout), B, per, alpha,
                                     _hip.stream_of(xd)), 'inf_logit_forward')
    torch.cuda.synchronize()
    s64 = alpha + (1 - 2 * alpha) * x.double()
    _close(y, torch.log(s64) - torch.log(1 - s64))
    a32 = torch.tensor(alpha, dtype=torch.float32)
    c32 = 1.0 - 2.0 * a32
    s = a32 + c32 * x                                        # the same terms in fp32 (each is > 0: log 4 + log 0.9 at least)
    terms = -torch.log(s - s * s) + torch.log(c32)
    assert (terms > 0).all()
    base = lin.double() if with_logp else torch.zeros(B, dtype=torch.float64)
    _sums_close(lout, base - terms.double().sum(1))


@pytest.mark.parametrize('per', [1, 255, 257, 3071])
def test_normal_logprob_sizes(per):
    """out[b] = sum_i (-0.5 log(2 pi) - z_i^2 / 2) at the same per-sample sizes."""
    lib = _hip.load()
    B = 3
    z = torch.randn(B, per, generator=_gen(10 + per))
    zd = z.to(DEV)
    out = torch.full((B,), float('nan'), device=DEV)
    _poison_lds(zd)
    _hip.check(lib.inf_normal_logprob(_hip.ptr(zd), _hip.ptr(out), B, per, _hip.stream_of(zd)), 'inf_normal_logprob')
    torch.cuda.synchronize()
    logz = -0.5 * torch.log(torch.tensor(2.0 * np.pi, dtype=torch.float32))
    terms = logz - z * z / 2.0                               # fp32 terms, all negative
    _sums_close(out, terms.double().sum(1))
    _sums_close(out, (-0.5 * np.log(2 * np.pi) - z.double() ** 2 / 2).sum(1))


# ---- inf_squeeze2 ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C,H,W', [(1, 2, 2), (3, 6, 10), (5, 8, 4)])
def test_squeeze2_shapes(C, H, W):
    """Space to depth by 2 on the smallest image, on H != W and on odd channel counts: bitwise the reference's
    permute(0, 1, 3, 5, 2, 4)."""
    lib = _hip.load()
    B = 3
    x = torch.randn(B, C, H, W, generator=_gen(C * 100 + H))
    xd = x.to(DEV)
    y = torch.full((B * 4 * C * (H // 2) * (W // 2) + 1,), 7.0, device=DEV)
    _poison_lds(xd)
    _hip.check(lib.inf_squeeze2(_hip.ptr(xd), _hip.ptr(y), B, C, H, W, _hip.stream_of(xd)), 'inf_squeeze2')
    torch.cuda.synchronize()
    ref = x.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(B, 4 * C, H // 2, W // 2)
    assert torch.equal(y[:-1].cpu().view_as(ref), ref)
    assert y[-1].item() == 7.0


# ---- inf_rademacher ----------------------------------------------------------------------------------------------------

def _draw(n, seed, offset=0):
    out = torch.full((n + 1,), 7.0, device=DEV)
    _poison_lds(out)
    _hip.check(_hip.load().inf_rademacher(_hip.ptr(out), n, seed, offset, _hip.stream_of(out)), 'inf_rademacher')
    torch.cuda.synchronize()
    assert out[n].item() == 7.0
    return out[:n].cpu()


@pytest.mark.parametrize('n', [1, 257, 100003])
def test_rademacher_stream(n):
    """Exactly +-1; a draw at offset k is the global draw's slice [k:]; two seeds differ; the mean of 1e5 draws is
    within 0.02 of zero (6 sigma of 1 / sqrt(1e5))."""
    seed = 5
    full = _draw(n + 4096, seed)
    assert ((full == 1.0) | (full == -1.0)).all()
    assert torch.equal(_draw(n, seed), full[:n])
    for k in (1, 255, 4096):
        assert torch.equal(_draw(n, seed, k), full[k:k + n]), k
    if n > 1:
        assert not torch.equal(_draw(n, seed + 1), full[:n])
    if n >= 100000:
        assert abs(full[:100000].double().mean().item()) <= 0.02
