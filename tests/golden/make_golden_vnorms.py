"""Golden vectors for mixed induced norms (--vnorms such as '13f1'), from the reference itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vnorms.py [case ...]

Same harness as make_golden.py (its import shims and capture hooks, reused by import) and, for the training case,
make_golden_train.py's.  Three kinds of case:

* ``vnorms_power_iter``: one reference ``compute_weight(update=True)`` per entry of lib/synthetic.py VNORM_LAYERS
  and norm pair, 5 fixed iterations, plus one tolerance-mode run (atol = rtol = 1e-3) per shape.  W, u0 and v0 come
  from ``syn.vnorm_layer_inputs(name, seed)`` and are not stored; stored are the seed, the module's u, v and scale
  after the update (the 1x1 conv's stale buffers as the reference leaves them) and the iteration count.  Vectors
  longer than VNORM_SAMPLE are stored as a seeded sample (``syn.vnorm_sample_index``) plus ``syn.vec_summary``; a
  one-hot vector as its index.
* ``vnorms_construct``: state dicts of reference ``InducedNormLinear(5, 7, domain, codomain)`` built on the CPU under
  ``torch.manual_seed`` (the random restarts included).
* the flows ``vnorms_cifar_small_b4`` ('13f1'), ``vnorms_fc_b16`` and ``vnorms_fc_train_b16`` ('2332') on the
  configs of lib/synthetic.py, captured like make_golden.py / make_golden_train.py capture theirs.  The reference's
  factories build InducedNorm layers for these norm pairs; for its class default '122f' they build LopConv2d
  (closed-form column / row norms, no u / v), which this project does not provide, so no fixture is made of it.

Every case runs the reference with 1 and with 8 torch threads and is written only if the two runs agree.  A
power-iteration case is also written only if
  - the same layer in fp64 (``.double()``) moves u, v and scale by at most a quarter of the tests' tolerance
    2e-5 max(1, |ref|_inf), so fp32 roundoff alone cannot fail the test;
  - at every one-hot normalisation the largest and second largest |entry| differ by more than 1e-3 relative;
  - in tolerance mode neither err / tol ratio lies in [0.8, 1.25] at the final or the preceding iteration.
A flow case needs at least one layer with sigma > coeff.  Seeds are the first that pass; the ones skipped are printed
and noted below.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims + reference import + hooks)
import make_golden_train as mgt  # noqa: E402
import lib.layers.base.mixed_lipschitz as ml  # noqa: E402  (the reference's)

torch = mg.torch
syn = mg.syn
layers = mg.layers
base_layers = mg.base_layers
INF = float('inf')
TOL = 2e-5          # the tests' bound, x max(1, |ref|_inf)
GAP = 1e-3          # one-hot: relative distance of the two largest |entries|
MARGIN = (0.8, 1.25)

# Every case tries seeds 0, 1, ... and takes the first that passes.  Seeds skipped in the run that made the committed
# fixtures (all others took seed 0):
#   conv3_96/1_2 (n5 and tol): seed 0 (1 and 8 threads differ) -> 1
#   conv3_96/3_3/n5:           seeds 0 .. 15 (1 and 8 threads differ: two long fp32 sums per normalisation) -> 16
#   vnorms_construct 3_3:      seed 0 (a restart's scale within 1e-4 of the first start's) -> 1


# ---- instrumented normalisations ------------------------------------------------------------------------------
GAPS = []
_orig_projmax = ml.projmax_


def _projmax(v):
    a = torch.sort(torch.abs(v.detach().double().view(-1)), descending=True)[0]
    GAPS.append(float((a[0] - a[1]) / a[0]) if a.numel() > 1 else 1.0)
    return _orig_projmax(v)


ml.projmax_ = _projmax


def _layer(kind, cin, cout, k, hw, dom, cod, W, u0, v0, n_iterations, dtype=torch.float32):
    """A reference layer holding (W, u0, v0), ready for compute_weight(update=True)."""
    tol = dict(n_iterations=n_iterations, atol=1e-3, rtol=1e-3)
    if kind == 'linear':
        m = ml.InducedNormLinear(cin, cout, domain=dom, codomain=cod, **tol)
    else:
        m = ml.InducedNormConv2d(cin, cout, k, 1, k // 2, domain=dom, codomain=cod, **tol)
        m.initialized.fill_(1)
        m.spatial_dims.copy_(torch.tensor([float(hw[0]), float(hw[1])]))
    m = m.to(dtype)
    with torch.no_grad():
        m.weight.copy_(W.to(dtype))
    m.u = u0.to(dtype).clone()
    m.v = v0.to(dtype).clone()
    return m


def _simulate(m, kind, k, hw, dom, cod, n_iterations):
    """The update's loop restated with the reference's own normalize_u / normalize_v: the iteration count and, per
    iteration, err / tol of u and v.  Returns (iters, ratios, u, v)."""
    W = m.weight.detach()
    u, v = m.u.detach().clone().view(-1), m.v.detach().clone().view(-1)
    if kind == 'linear' or k == 1:
        Wm = W.view(W.shape[0], W.shape[1])
        fwd, bwd = (lambda t: torch.mv(Wm, t)), (lambda t: torch.mv(Wm.t(), t))
    else:
        c, o = W.shape[1], W.shape[0]
        fwd = lambda t: torch.nn.functional.conv2d(t.view(1, c, *hw), W, padding=k // 2).reshape(-1)
        bwd = lambda t: torch.nn.functional.conv_transpose2d(t.view(1, o, *hw), W, padding=k // 2).reshape(-1)
    ratios, iters = [], 0
    for _ in range(200 if n_iterations is None else n_iterations):
        ou, ov = u.clone(), v.clone()
        u = ml.normalize_u(fwd(v), cod)
        v = ml.normalize_v(bwd(u), dom)
        iters += 1
        eu = torch.norm(u - ou) / (u.nelement() ** 0.5)
        ev = torch.norm(v - ov) / (v.nelement() ** 0.5)
        tu, tv = 1e-3 + 1e-3 * torch.max(u), 1e-3 + 1e-3 * torch.max(v)
        ratios.append((float(eu / tu), float(ev / tv)))
        if n_iterations is None and eu < tu and ev < tv:
            break
    return iters, ratios, u, v


def _power_case(name, kind, cin, cout, k, hw, dom, cod, n_iterations, seed):
    """One case at one seed: the fixture entries, or a string saying which check failed."""
    W, u0, v0 = syn.vnorm_layer_inputs(name, seed)
    runs = []
    for nt in (1, 8):
        torch.set_num_threads(nt)
        m = _layer(kind, cin, cout, k, hw, dom, cod, W, u0, v0, n_iterations)
        GAPS.clear()
        with torch.no_grad():
            m.compute_weight(update=True)
        runs.append((m.u.detach().clone(), m.v.detach().clone(), m.scale.detach().clone(), list(GAPS)))
    if not all(torch.equal(a, b) for a, b in zip(runs[0][:3], runs[1][:3])):
        return '1 and 8 threads differ'
    u, v, scale, gaps = runs[1]
    if gaps and min(gaps) <= GAP:
        return 'one-hot gap %.2e' % min(gaps)
    m = _layer(kind, cin, cout, k, hw, dom, cod, W, u0, v0, n_iterations)
    iters, ratios, ui, vi = _simulate(m, kind, k, hw, dom, cod, n_iterations)
    sigma_i = float(torch.dot(ui, (torch.mv(m.weight.view(cout, cin), vi) if (kind == 'linear' or k == 1) else
                                   torch.nn.functional.conv2d(vi.view(1, cin, *hw), m.weight, padding=k // 2).view(-1))))
    if abs(sigma_i - float(scale)) > 1e-6 * max(1.0, abs(sigma_i)):
        return 'the restated loop gives sigma %.8f, the module %.8f' % (sigma_i, float(scale))
    if n_iterations is None:
        if iters >= 200:
            return 'no convergence in 200 iterations'
        for r in ratios[-2:]:
            if any(MARGIN[0] <= q <= MARGIN[1] for q in r):
                return 'marginal stop: err/tol %s' % (ratios[-2:],)
    # fp64 rerun
    m64 = _layer(kind, cin, cout, k, hw, dom, cod, W, u0, v0, iters, dtype=torch.float64)
    with torch.no_grad():
        m64.compute_weight(update=True)
    for a, b, what in ((u, m64.u, 'u'), (v, m64.v, 'v'), (scale, m64.scale, 'scale')):
        d = float((a.double() - b.double()).abs().max())
        bound = 0.25 * TOL * max(1.0, float(a.abs().max()))
        if d > bound:
            return 'fp64 moves %s by %.2e > %.2e' % (what, d, bound)
    out = dict(seed=np.int64(seed), iters=np.int64(iters), scale=np.float32(scale.item()),
               n_iterations=np.int64(-1 if n_iterations is None else n_iterations),
               domain=np.float32(dom), codomain=np.float32(cod))
    stale_u = kind == 'conv' and k == 1 and cod == INF
    stale_v = kind == 'conv' and k == 1 and dom == 1
    for key, t, t0, hot, stale in (('u', u, u0, cod == INF, stale_u), ('v', v, v0, dom == 1, stale_v)):
        t = t.view(-1).numpy()
        if stale:
            assert np.array_equal(t, t0.numpy()), 'the reference did not leave %s stale' % key
            out[key + '_stale'] = np.int64(1)
        elif hot:
            assert (t != 0).sum() == 1 and t.max() == 1.0
            out[key + '_hot'] = np.int64(int(np.argmax(t)))
        elif t.size > syn.VNORM_SAMPLE:
            out[key + '_sample'] = t[syn.vnorm_sample_index(name + '.' + key, t.size)].astype(np.float32)
            s, _ = syn.vec_summary(t, 'vnorm.' + name + '.' + key)
            out[key + '_summary'] = s
            out[key + '_absmax'] = np.float32(np.abs(t).max())
        else:
            out[key] = t.astype(np.float32)
    return out


def case_id(name, dom, cod, tol_mode):
    f = lambda p: 'inf' if p == INF else '%g' % p
    return '%s/%s_%s/%s' % (name, f(dom), f(cod), 'tol' if tol_mode else 'n5')


def power_iter_cases():
    out, skipped = {}, {}
    for name, kind, cin, cout, k, hw, pairs in syn.VNORM_LAYERS:
        todo = [(dom, cod, 5) for dom, cod in pairs] + [(pairs[0][0], pairs[0][1], None)]
        for dom, cod, n_it in todo:
            cid = case_id(name, dom, cod, n_it is None)
            for seed in range(20):
                r = _power_case(name, kind, cin, cout, k, hw, dom, cod, n_it, seed)
                if isinstance(r, dict):
                    break
                skipped.setdefault(cid, []).append((seed, r))
            else:
                raise SystemExit('%s: no seed in 0..19 passes: %s' % (cid, skipped[cid]))
            print('%-28s seed %d iters %3d scale %+.6f' % (cid, seed, int(r['iters']), float(r['scale'])))
            for key, val in r.items():
                out['%s:%s' % (cid, key)] = val
    out['cases'] = np.array(sorted({k.split(':')[0] for k in out}))
    path = os.path.join(HERE, 'vnorms_power_iter.npz')
    np.savez_compressed(path, **out)
    print('-> %s (%d KB); skipped seeds: %s' % (os.path.basename(path), os.path.getsize(path) // 1024, skipped or 'none'))


# ---- construction ---------------------------------------------------------------------------------------------
def construct_cases():
    out = {}
    for tag, dom, cod in (('1_inf', 1, INF), ('3_3', 3, 3)):
        for seed in range(20):
            sds, scales = [], []
            for nt in (1, 8):
                torch.set_num_threads(nt)
                torch.manual_seed(seed)
                log = []
                orig = ml.InducedNormLinear.compute_weight

                def spy(self, *a, **k):
                    r = orig(self, *a, **k)
                    log.append(float(self.scale))
                    return r
                ml.InducedNormLinear.compute_weight = spy
                try:
                    GAPS.clear()
                    m = ml.InducedNormLinear(5, 7, domain=dom, codomain=cod)
                finally:
                    ml.InducedNormLinear.compute_weight = orig
                sds.append({k: v.detach().clone() for k, v in m.state_dict().items()})
                scales.append((log, list(GAPS)))
            same = all(torch.equal(sds[0][k], sds[1][k]) for k in sds[0])
            log, gaps = scales[1]
            # the restart rule compares each restart's scale with the first run's: no comparison may be marginal
            # (the same bits, as when two starts reach the same one-hot pair, are not)
            clear = all(s == log[0] or abs(s - log[0]) > 1e-4 * max(abs(log[0]), 1e-3) for s in log[1:])
            if same and clear and (not gaps or min(gaps) > GAP):
                break
            print('construct %s: seed %d skipped (same %s, clear %s, gap %s)' % (tag, seed, same, clear,
                                                                                 min(gaps) if gaps else None))
        else:
            raise SystemExit('construct %s: no seed passes' % tag)
        print('construct %-6s seed %d scales %s' % (tag, seed, ['%.4f' % s for s in log]))
        out[tag + ':seed'] = np.int64(seed)
        out[tag + ':domain'], out[tag + ':codomain'] = np.float32(dom), np.float32(cod)
        for k, v in sds[1].items():
            out['%s:sd:%s' % (tag, k)] = v.numpy().copy()
    np.savez_compressed(os.path.join(HERE, 'vnorms_construct.npz'), **out)


# ---- flows ----------------------------------------------------------------------------------------------------
def _conv_model(arch, B):
    """make_golden.conv_model with the arch's vnorms."""
    c, h, w = arch['input_size']
    return mg.ImplicitFlow(
        (B, c, h, w), n_blocks=arch['n_blocks'], intermediate_dim=arch['idim'], factor_out=False,
        init_layer=layers.LogitTransform(arch['init_alpha']), actnorm=arch['actnorm'], fc=False,
        coeff=arch['coeff'], vnorms=arch['vnorms'], sn_atol=1e-3, sn_rtol=1e-3, n_power_series=None,
        n_dist=arch['n_dist'], n_samples=1, kernels=arch['kernels'], activation_fn=arch['act'],
        fc_end=False, n_exact_terms=arch['n_exact_terms'], preact=arch['preact'], neumann_grad=True,
        grad_in_forward=True)


def _fc_model(arch):
    """make_golden.fc_model with per-layer norms (train_tabular.py:283-307)."""
    d = arch['d']
    dims = [d] + list(arch['dims']) + [d]
    norms = syn.layer_norms(arch)
    act = {'sin': base_layers.Sin, 'swish': base_layers.Swish}[arch['act']]

    def build_nnet():
        nnet = []
        for i, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
            if i > 0:
                nnet.append(act())
            nnet.append(base_layers.get_linear(a, b, coeff=arch['coeff'], n_iterations=None, atol=1e-3, rtol=1e-3,
                                               domain=norms[i][0], codomain=norms[i][1], zero_init=(b == d)))
        return torch.nn.Sequential(*nnet)

    blocks = [layers.imBlock(build_nnet(), build_nnet(), n_dist=arch['n_dist'], n_power_series=None,
                             exact_trace=arch.get('exact_trace', False), brute_force=arch['brute_force'], n_samples=1,
                             n_exact_terms=arch['n_exact_terms'], neumann_grad=False, grad_in_forward=False,
                             eps_forward=arch['eps_forward'])
              for _ in range(arch['n_blocks'])]
    return layers.SequentialFlow(blocks)


def _placeholder_u_v(self):
    """Stands in for InducedNormConv2d._initialize_u_v while a flow case builds its model: u / v of the right sizes
    without the ten random restarts of 200 iterations each (minutes for a conv flow).  run_case loads the state dict
    right after the materialising forward, which overwrites u, v and scale."""
    with torch.no_grad():
        if self.kernel_size == (1, 1):
            nu, nv = self.out_channels, self.in_channels
        else:
            c, h, w = self.in_channels, int(self.spatial_dims[0].item()), int(self.spatial_dims[1].item())
            nv = c * h * w
            nu = torch.nn.functional.conv2d(torch.zeros(1, c, h, w), self.weight, stride=self.stride,
                                            padding=self.padding).numel()
        self.u.resize_(nu).zero_()
        self.v.resize_(nv).zero_()
        self.u[0] = 1
        self.v[0] = 1
        self.initialized.fill_(1)


def _trajectory(path):
    g = np.load(path)
    keys = sorted(k for k in g.files if k.endswith(('_nstep', '_lowest_step', '_n_power_series')))
    return [(k, np.asarray(g[k]).tolist()) for k in keys], float(g['loss'])


def flow_case(name, arch, run):
    """run() writes tests/golden/<name>.npz; kept only if 1 and 8 threads give the same trajectory and some layer of
    the arch has sigma > coeff."""
    sd = syn.make_state_dict(arch, 0)
    over = [k for k, v in sd.items() if k.endswith('.scale') and '_copy.' not in k and float(v) > arch['coeff']]
    if not over:
        raise SystemExit('%s: no layer with sigma > coeff: the scale path would be idle' % name)
    path = os.path.join(HERE, name + '.npz')
    own = mg.conv_model, mg.fc_model, ml.InducedNormConv2d._initialize_u_v
    mg.conv_model, mg.fc_model, ml.InducedNormConv2d._initialize_u_v = _conv_model, _fc_model, _placeholder_u_v
    got = []
    try:
        for nt in (1, 8):
            torch.set_num_threads(nt)
            run()
            got.append(_trajectory(path))
    finally:
        mg.conv_model, mg.fc_model, ml.InducedNormConv2d._initialize_u_v = own
    if got[0][0] != got[1][0]:
        os.remove(path)
        raise SystemExit('%s: 1 and 8 threads give different trajectories (choose another seed)' % name)
    print('   %s: stable over 1 / 8 threads, |d loss| %.2e; %d layers with sigma > coeff' % (
        name, abs(got[0][1] - got[1][1]), len(over)))


SMALL, FC = syn.CONFIGS['cifar10_small_13f1'], syn.CONFIGS['fc_2332']
CASES = {
    'vnorms_power_iter': power_iter_cases,
    'vnorms_construct': construct_cases,
    'vnorms_cifar_small_b4': lambda: flow_case('vnorms_cifar_small_b4', SMALL, lambda: mg.run_case(
        'vnorms_cifar_small_b4', SMALL, syn.image_batch(4, seed=3), seed=7)),
    'vnorms_fc_b16': lambda: flow_case('vnorms_fc_b16', FC, lambda: mg.run_case(
        'vnorms_fc_b16', FC, syn.tabular_batch(16, 6, seed=3), seed=7)),
    'vnorms_fc_train_b16': lambda: flow_case('vnorms_fc_train_b16', FC, lambda: mgt.run_train_case(
        'vnorms_fc_train_b16', FC, syn.tabular_batch(16, 6, seed=8), seed=13)),
}

if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        CASES[n]()
