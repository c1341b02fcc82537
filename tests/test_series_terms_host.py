"""Host-side checks of the inputs of tests/test_gpu_series_terms.py, in fp64 on the CPU.  No GPU.

The GPU tests compare n-term sums with fp64 at 2e-5 max(1, |ref|_inf).  A term below that bound could be wrong unnoticed,
so the condition on every strong net and input used there is: the LAST term's reference magnitude |c_n term_n| (max over
the samples) is at least 100 x the absolute tolerance applied to the sum -- then every term weighs in the comparison.  It
is a condition on the inputs, not a measurement of the engine.  The same for the Neumann vector's last term against the
vector's bound, and, for the fc nets up to d = 16, the exact-trace series.
"""
import numpy as np
import pytest
import torch

import test_gpu_series_terms as T

MARGIN = 100.0


def _conv_uses():
    """(net, B) of every conv run on the GPU, the whole-sum runs' series length."""
    uses = set()
    for xname, zname, B, *_ in T.CONV_RUNS.values():
        uses.add((xname, B))
        if zname:
            uses.add((zname, B))
    return sorted(uses)


def _neumann_margin(chain, eps, nco):
    """|ncoeff_n| |v_n|_inf (max over samples) over 2e-5 max(1, |w|_inf)."""
    c = torch.tensor(nco[1:].astype(np.float64)).view(-1, *([1] * (chain.dim() - 1)))
    w = eps.double() + (c * chain).sum(0)
    return abs(float(nco[-1])) * chain[-1].abs().max().item() / (T.FWD_TOL * max(1.0, w.abs().max().item()))


@pytest.mark.parametrize('name,B', _conv_uses())
def test_conv_fixture_last_term_weighs_100_tolerances(name, B):
    seq, x, eps = T.conv_case(name)
    n = T.CONV_NETS[name][4]
    chain, e = T.conv_chain(name)[:n, :B], eps[:B]
    m = T.fixture_margin(chain, e, T.series_coeff(n))
    mn = _neumann_margin(chain, e, T.neumann_coeff(n))
    dots, _ = T.term_dots(chain, e)
    print('%s B=%d n=%d: |c_k term_k| max over samples %s; last term / tolerance: series %.0f, neumann %.0f'
          % (name, B, n, ' '.join('%.2e' % (v / (k + 1)) for k, v in enumerate(dots.abs().max(1)[0])), m, mn))
    assert m >= MARGIN and mn >= MARGIN


@pytest.mark.parametrize('name', sorted(T.FC_NETS))
def test_fc_fixture_last_term_weighs_100_tolerances(name):
    seq, x, eps = T.fc_case(name)
    d, n = x.shape[1], T.FC_NETS[name][6]
    chain = T.fc_chain(name)[:n]
    co = T.series_coeff(n)
    m = T.fixture_margin(chain, eps, co)
    mn = _neumann_margin(chain, eps, T.neumann_coeff(n))
    dots, _ = T.term_dots(chain, eps)
    print('%s B=%d n=%d: |c_k term_k| max over samples %s; last term / tolerance: series %.0f, neumann %.0f'
          % (name, x.shape[0], n, ' '.join('%.2e' % (v / (k + 1)) for k, v in enumerate(dots.abs().max(1)[0])), m, mn))
    assert m >= MARGIN and mn >= MARGIN
    if d <= 16 and name in T.FC_SUM_NETS:
        tr, _ = T._trace_refs(T.ref_jacobian(seq, x), n)
        c = torch.tensor(co.astype(np.float64)).unsqueeze(1)
        S = (c * tr).sum(0)
        mt = (c[-1] * tr[-1]).abs().max().item() / (T.FWD_TOL * max(1.0, S.abs().max().item()))
        print('%s exact trace: last term / tolerance %.0f' % (name, mt))
        assert mt >= MARGIN


def test_strong_layers_sit_at_their_cap_with_converged_singular_pairs():
    """Every layer of a strong net has sigma = u . (W v) above coeff (the Lipschitz rescaling is active), and (u, v) lies
    in the top singular cluster: the d structured singular values are nearly equal (2 plus noise), so the power iteration
    ends on a mixture of them -- sigma is below the 2-norm, by less than the cluster's width (1 %)."""
    seq = T.strong_fc(6, 128, T.Sin, 5)
    for m in seq:
        if hasattr(m, 'compute_weight'):
            sigma = torch.dot(m.u, torch.mv(m.weight, m.v)).item()
            top = torch.linalg.matrix_norm(m.weight.detach().double(), 2).item()
            assert sigma > m.coeff and 0.99 * top <= sigma <= top * (1 + 1e-6), (sigma, top)


def test_builders_are_deterministic():
    a, b = T.strong_conv(C=3, hid=64, H=8, W=8, lead=True), T.strong_conv(C=3, hid=64, H=8, W=8, lead=True)
    for (_, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(p, q)


def test_reference_chain_matches_the_explicit_jacobian():
    """ref_chain's eps^T J^k against powers of ref_jacobian's J on an fc net (two independent fp64 routes)."""
    seq, x, eps = T.fc_case('swish6')
    chain, J = T.fc_chain('swish6'), T.ref_jacobian(seq, x)
    v = eps.double()
    for k in range(chain.shape[0]):
        v = torch.bmm(v.unsqueeze(1), J).squeeze(1)
        assert (v - chain[k]).abs().max().item() <= 1e-12 * max(1.0, v.abs().max().item())
