"""Host-side checks for the wide fc training route: the reference fixture the GPU test reads, and the
pair construction inf_logdet_grad(INF_LOGDET_SERIES) uses above d = 16, in fp64 torch, independent of any kernel."""
import os

import numpy as np
import pytest
import torch


def test_tab_d43_train_fixture_loads(golden_dir):
    """tab_d43_train_b16 has what test_gpu_widefc_train.py::test_tab_d43_training_matches_reference reads: the batch,
    the seeds, the loss, four blocks' forward step counts and series lengths, 80 gradients, no backward step counts."""
    g = np.load(os.path.join(golden_dir, 'tab_d43_train_b16.npz'))
    assert g['x'].shape == (16, 43) and g['x'].dtype == np.float32
    assert int(g['nblocks']) == 4 and np.isfinite(float(g['loss']))
    for k in ('seed', 'weight_seed', 'logpx'):
        assert k in g.files
    for i in range(4):
        assert int(g['b%d_nstep' % i]) >= 1
        assert len(g['b%d_n_power_series' % i]) >= 1 and min(g['b%d_n_power_series' % i]) >= 1
    assert len([k for k in g.files if k.startswith('g:') or k.startswith('gs:')]) == 80
    assert not [k for k in g.files if '_bwd_' in k]
    for k in g.files:
        if k.startswith('gs:'):
            assert 'gh:' + k[3:] in g.files


def _jvp(y, x, v):
    """J(x) v with the graph into x and the parameters, by two reverse passes (autograd only)."""
    u = torch.ones_like(y, requires_grad=True)
    vjp = torch.autograd.grad(y, x, u, create_graph=True)[0]
    return torch.autograd.grad(vjp, u, v, create_graph=True)[0]


@pytest.mark.parametrize('n', [1, 2, 5])
def test_series_pairs_reproduce_autograd(n):
    """S_b = sum_{k=1..n} c_k eps^T J^k eps on a 19-24-19 Sin net, B = 4.  The n pairs from the two chains,
    A_m = g sum_{j <= n-1-m} c_{j+m+1} a_j with a_j = (J^T)^j eps and b_m = J^m eps (constants), give
    sum_m A_m^T J b_m, whose gradient into x and every parameter equals autograd's gradient of sum_b g_b S_b; and
    S_b = sum_k c_k eps . b_k.  Shifting the coefficient index by one, or letting j run to n-1, must not."""
    d, B, hid = 19, 4, 24
    gen = torch.Generator().manual_seed(5 + n)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    params = [(rnd(hid, d) * 0.3).requires_grad_(True), (rnd(hid) * 0.1).requires_grad_(True),
              (rnd(d, hid) * 0.3).requires_grad_(True), (rnd(d) * 0.1).requires_grad_(True)]
    f = lambda t: torch.sin(t @ params[0].T + params[1]) @ params[2].T + params[3]
    x = (rnd(B, d) * 0.5).requires_grad_(True)
    eps = torch.sign(rnd(B, d))
    g = rnd(B)
    g[1] = 0.0
    c = [(-1) ** (k + 1) / k * (1.3 if k > 2 else 1.0) for k in range(1, n + 1)]     # c[k-1] = c_k
    leaves = [x] + params
    y = f(x)
    # autograd through the truncated series (basic_logdet_estimator with create_graph)
    v, S = eps, torch.zeros(B, dtype=torch.float64)
    for k in range(1, n + 1):
        v = torch.autograd.grad(y, x, v, create_graph=True)[0]
        S = S + c[k - 1] * (v * eps).sum(1)
    ref = torch.autograd.grad((S * g).sum(), leaves, retain_graph=True, allow_unused=True)
    # the two chains, as constants
    a, b = [eps], [eps]
    for j in range(1, n + 1):
        a.append(torch.autograd.grad(y, x, a[-1], retain_graph=True)[0].detach())
        b.append(_jvp(y, x, b[-1]).detach())
    value = sum(c[k - 1] * (eps * b[k]).sum(1) for k in range(1, n + 1))
    assert torch.allclose(value, S.detach(), rtol=1e-12, atol=1e-14)

    def pair_grads(shift, jmax):
        total = 0.0
        for m in range(n):
            A = g[:, None] * sum(c[j + m + shift] * a[j] for j in range(jmax(m) + 1) if 0 <= j + m + shift < n)
            total = total + (A * _jvp(y, x, b[m])).sum()
        return torch.autograd.grad(total, leaves, retain_graph=True, allow_unused=True)
    got = pair_grads(0, lambda m: n - 1 - m)
    for r, q in zip(ref, got):
        if r is None or q is None:           # (the last bias does not enter J)
            assert r is None and q is None
            continue
        assert torch.allclose(q, r, rtol=1e-9, atol=1e-12 * max(1.0, r.abs().max().item()))
    assert sum(1 for r in ref if r is None) == 1
    # the convention is pinned: another coefficient index or another upper limit of j gives another gradient
    wrong = [pair_grads(1, lambda m: n - 1 - m), pair_grads(0, lambda m: n - 2 - m)] if n > 1 else []
    for w in wrong:
        rx = ref[0]
        assert (w[0] - rx).abs().max().item() > 1e-3 * rx.abs().max().item()


# ---- the fc weight-gradient contraction's inputs (shared with test_gpu_widefc_train.py) ---------------------------------

FC_SHAPES = [(17, 128), (43, 128), (1025, 128)]          # (d, hidden)
FC_COLUMNS = [1, 31, 33, 257, 1030]                      # float4 tails, both sides of a 32-column chunk, many splits
WG_K, WG_T, MAX_SPLIT = 32, 64, 32                       # grad.hip's chunk and tile, engine_grad.hip GRAD_SPLIT
BOUND = 2e-4


def contraction_inputs(d, hidden, B):
    """The d-hidden-hidden-d Sin net (test_gpu_fcgrad._net), x and the upstream gradient of one contraction case."""
    from test_gpu_fcgrad import _net
    from lib import synthetic as syn
    from lib.layers.base import Sin
    net = _net(d, hidden, Sin, seed=7 + d)
    x = syn.tabular_batch(B, d, seed=100 + B) * 0.5
    gout = syn.tabular_batch(B, d, seed=200 + B)
    return net, x, gout


def _split_boundary_column(M, N, B):
    """First column of the middle split of wgrad_fc_kernel's launch (launch_wgrad's rule), or None with one split."""
    tiles = ((M + WG_T - 1) // WG_T) * ((N + WG_T - 1) // WG_T)
    nchunks = (B + WG_K - 1) // WG_K
    nsplit = max(1, min(nchunks, 1024 // tiles, MAX_SPLIT))
    if nsplit < 2:
        return None
    return WG_K * ((nchunks * (nsplit // 2)) // nsplit)


@pytest.mark.parametrize('d,hidden', FC_SHAPES, ids=['d%d' % s[0] for s in FC_SHAPES])
@pytest.mark.parametrize('B', FC_COLUMNS)
def test_contraction_inputs_expose_a_dropped_column(d, hidden, B):
    """On the GPU cases' inputs, in fp64: the last layer's dW_eff = G X^T (G = gout^T (d, B), X the layer's input
    (hidden, B)) moves by at least 10 x the 2e-4 bound of its largest element when one column is dropped -- the last
    column, the last element of the last whole float4 group, the first column of the middle split and the one before
    it.  So a kernel that loses any of them cannot pass the GPU test."""
    from test_gpu_fcgrad import _eval64, _params64
    net, x, gout = contraction_inputs(d, hidden, B)
    with torch.no_grad():
        X = _eval64(net[:-1], x.double(), _params64(net))          # (B, hidden)
    G = gout.double()                                               # (B, d)
    dW = G.T @ X
    scale = dW.abs().max().item()
    cols = {B - 1}
    if B >= 4:
        cols.add(4 * (B // 4) - 1)
    sb = _split_boundary_column(d, hidden, B)
    if sb is not None:
        cols.update({sb, sb - 1})
        assert 0 < sb < B
    assert (B > WG_K) == (sb is not None)
    for c in sorted(cols):
        moved = torch.outer(G[c], X[c]).abs().max().item()
        assert moved >= 10 * BOUND * scale, (c, moved, scale)
