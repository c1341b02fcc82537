"""Golden vectors for fully connected blocks over more than 32 features, from the reference itself (build container
only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_widefc.py [case ...]

Same harness as make_golden.py (its import shims, capture hooks and run_case), make_golden_train.py's training case and
make_golden_acts.py's stability rule, all reused by import.  The architectures are lib/synthetic.py's FCEND_SMALL
(``ImplicitFlow(fc_end=True)``, the reference's class default: the last scale ends in two imBlock(FCNet, FCNet) with
ActNorm1d, d = 192), FC_IMG_SMALL (``fc=True``: every block fully connected, d = 192) and TAB_D43 / TAB_D63 (the
tabular flows of train_tabular.py at MINIBOONE's and BSDS300's widths).

Every case runs the reference with 1 and with 8 torch threads and is written only if both give every block the same
Broyden nstep / lowest_step and series lengths (make_golden_acts.stable).  All cases below are stable with the first
seeds tried (input seed 3, run seed 7; the inverse case z seed 3, run seed 7).

The training case (``fcend_small_train_b2``: one ``loss.backward()``, every parameter gradient) has its own rule,
stable_train.  Its forward trajectory (nstep and series lengths of every block) is the same with 1 and 8 threads for
every seed tried, but the implicit backward's solve is not: eps_backward = 1e-10 is below what fp32 reaches, so that
solve runs on at its noise floor to the threshold (30 steps, now and then 12 - 29) and its nstep / lowest_step follow
the summation order of the 192-wide linear layers, which torch's thread count changes (none of 36 seed pairs kept them:
(21, 5), (21, 6), (22, 5), (3, 7), (4, 9), (8, 13) and (s, s - 20) for s = 30 .. 59).  The solve's RESULT does not
move, though: so the case is kept if both runs give the same forward trajectory and the same loss to 1e-6, and every
recorded gradient of the 1-thread run lies within a quarter of tests/test_gpu_train.py::_check_grads' bounds of the
8-thread run's.  The backward step counts are not written into the fixture and no test pins them.  Input seed 21, run
seed 5 (cifar_small_train_b2's, the first tried).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims + reference import + hooks)
import make_golden_train as mgt  # noqa: E402  (backward-solve and Neumann hooks)
import make_golden_acts as mga  # noqa: E402  (stable: the 1 / 8 thread rule)

torch = mg.torch
syn = mg.syn
layers = mg.layers
ib = mg.ib


def _conv_model(arch, B):
    """make_golden.conv_model with fc / fc_end / fc_idim taken from the arch."""
    c, h, w = arch['input_size']
    return mg.ImplicitFlow(
        (B, c, h, w), n_blocks=arch['n_blocks'], intermediate_dim=arch['idim'], factor_out=False,
        init_layer=layers.LogitTransform(arch['init_alpha']), actnorm=arch['actnorm'], fc=arch.get('fc', False),
        coeff=arch['coeff'], vnorms='2222', sn_atol=1e-3, sn_rtol=1e-3, n_power_series=None,
        n_dist=arch['n_dist'], n_samples=1, kernels=arch['kernels'], activation_fn=arch['act'],
        fc_end=arch.get('fc_end', False), fc_idim=arch.get('fc_idim', 128), n_exact_terms=arch['n_exact_terms'],
        preact=arch['preact'], neumann_grad=True, grad_in_forward=True)


def stable(name, run):
    """make_golden_acts.stable with the builder above installed in make_golden's namespace for the case."""
    own = mg.conv_model
    mg.conv_model = _conv_model
    try:
        mga.stable(name, run)
    finally:
        mg.conv_model = own


def run_inverse_case(name, arch, B, z_seed, seed, weight_seed=0):
    """``ImplicitFlow.inverse(z, logpz)`` in eval: x, the returned log-density term, and every block's root solve
    (imBlock.inverse, implicit_block.py:236-243) in the order the inverse visits the blocks (last block first)."""
    torch.manual_seed(1234)
    model = _conv_model(arch, B)
    x0 = syn.image_batch(2, arch['input_size'], arch['nvals'], seed=1)
    with torch.no_grad():
        model(x0, restore=True)
    model.load_state_dict(syn.make_state_dict(arch, weight_seed), strict=True)
    model.eval()
    z = torch.randn(B, int(np.prod(arch['input_size'])), generator=torch.Generator().manual_seed(z_seed)) * 0.5
    solves = []
    inner = ib.broyden

    def broyden(*a, **k):
        r = inner(*a, **k)
        solves.append((r['nstep'], r['lowest_step'], int(r['prot_break'])))
        return r
    mg.REC.clear()
    mg.REC.append({})                       # the capture hooks write into the last record; no forward opens one here
    ib.broyden = broyden
    try:
        np.random.seed(seed)
        torch.manual_seed(seed)
        with torch.no_grad():
            x, logpx = model.inverse(z, torch.zeros(B, 1))
    finally:
        ib.broyden = inner
    out = dict(z=z.numpy().astype(np.float32), seed=np.int64(seed), weight_seed=np.int64(weight_seed),
               x=x.detach().reshape(B, -1).numpy().astype(np.float32),
               logpx=logpx.detach().view(-1).numpy().astype(np.float64), nblocks=np.int64(len(solves)),
               loss=np.float64(logpx.mean().item()),
               n_power_series=np.asarray(mg.REC[0].get('n_power_series', [])))
    for i, (ns, ls, pb) in enumerate(solves):
        out['b%d_nstep' % i] = np.int64(ns)
        out['b%d_lowest_step' % i] = np.int64(ls)
        out['b%d_prot_break' % i] = np.int64(pb)
    # (make_golden_acts._trajectory reads b<i>_n_power_series per block: the inverse draws two series per block)
    nps = list(out['n_power_series'])
    for i in range(len(solves)):
        out['b%d_n_power_series' % i] = np.asarray(nps[2 * i:2 * i + 2])
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-26s mean logpx=%.8f solves=%s nps=%s -> %s (%d KB)' % (
        name, logpx.mean().item(), [s[0] for s in solves], nps, os.path.basename(path), os.path.getsize(path) // 1024))


IMG = (3, 8, 8)
GRAD_REL = 2e-3 / 4          # a quarter of _check_grads' rel


def _grads_agree(a, b):
    """_check_grads' comparisons (tests/test_gpu_train.py) between two fixtures, at GRAD_REL; returns the worst ratio of
    a difference to its bound."""
    worst = 0.0
    for k in a.files:
        if k.startswith('g:'):
            ref = b[k].astype(np.float64)
            worst = max(worst, np.abs(a[k] - ref).max() / (GRAD_REL * max(np.abs(ref).max(), 1e-12) + 1e-9))
        elif k.startswith('gs:'):
            sa, sb = a[k], b[k]
            norm = np.sqrt(sb[1])
            n = 1            # (the element count only widens _check_grads' sum / projection bounds: 1 is the strictest)
            worst = max(worst, abs(sa[0] - sb[0]) / (GRAD_REL * norm * np.sqrt(n)),
                        abs(np.sqrt(sa[1]) - norm) / (GRAD_REL * norm), abs(sa[2] - sb[2]) / (GRAD_REL * norm * np.sqrt(n)))
            ha, hb = a['gh:' + k[3:]].astype(np.float64), b['gh:' + k[3:]].astype(np.float64)
            worst = max(worst, np.abs(ha - hb).max() / (GRAD_REL * max(np.abs(hb).max(), 1e-12) + 1e-9))
    return worst


def stable_train(name, run):
    """The training case's rule (module docstring): 1 and 8 threads give the same forward trajectory, the same loss to
    1e-6 and gradients within a quarter of _check_grads' bounds; the backward step counts are dropped from the file."""
    path = os.path.join(HERE, name + '.npz')
    own = mg.conv_model
    mg.conv_model = _conv_model
    got = []
    try:
        for nt in (1, 8):
            torch.set_num_threads(nt)
            run()
            g = np.load(path)
            got.append({k: g[k] for k in g.files})
    finally:
        mg.conv_model = own

    class _G(dict):
        files = property(lambda self: list(self))
    a, b = _G(got[0]), _G(got[1])
    fwd = lambda g: [(int(g['b%d_nstep' % i]), np.asarray(g['b%d_n_power_series' % i]).tolist())
                     for i in range(int(g['nblocks']))]
    worst = _grads_agree(a, b)
    dl = abs(float(a['loss']) - float(b['loss']))
    if fwd(a) != fwd(b) or dl > 1e-6 or worst > 1.0:
        os.remove(path)
        raise SystemExit('%s: not stable: forward %s, |d loss| %.2e, worst gradient ratio %.2f'
                         % (name, 'same' if fwd(a) == fwd(b) else 'DIFFERS', dl, worst))
    keep = {k: v for k, v in b.items() if '_bwd_' not in k}
    np.savez_compressed(path, **keep)
    print('   %s: forward trajectory the same over 1 / 8 threads, |d loss| %.2e, gradients within %.2f of a quarter of '
          'the bounds (backward steps %s against %s: not kept)' % (
              name, dl, worst, [int(a['b%d_bwd_nstep' % i]) for i in range(int(a['nblocks']))],
              [int(b['b%d_bwd_nstep' % i]) for i in range(int(b['nblocks']))]))


CASES = {
    'fcend_small_b4': lambda: stable('fcend_small_b4', lambda: mg.run_case(
        'fcend_small_b4', syn.FCEND_SMALL, syn.image_batch(4, IMG, seed=3), seed=7)),
    'fc_img_small_b4': lambda: stable('fc_img_small_b4', lambda: mg.run_case(
        'fc_img_small_b4', syn.FC_IMG_SMALL, syn.image_batch(4, IMG, seed=3), seed=7)),
    'tab_d43_b64': lambda: stable('tab_d43_b64', lambda: mg.run_case(
        'tab_d43_b64', syn.TAB_D43, syn.tabular_batch(64, 43, seed=3), seed=7)),
    'tab_d63_b64': lambda: stable('tab_d63_b64', lambda: mg.run_case(
        'tab_d63_b64', syn.TAB_D63, syn.tabular_batch(64, 63, seed=3), seed=7)),
    'fcend_small_train_b2': lambda: stable_train('fcend_small_train_b2', lambda: mgt.run_train_case(
        'fcend_small_train_b2', syn.FCEND_SMALL, syn.image_batch(2, IMG, seed=21), seed=5)),
    'fcend_small_inverse_b4': lambda: stable('fcend_small_inverse_b4', lambda: run_inverse_case(
        'fcend_small_inverse_b4', syn.FCEND_SMALL, 4, z_seed=3, seed=7)),
}

if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        CASES[n]()
