"""Lipschitz-capped conv / linear layers (reference: lib/layers/base/mixed_lipschitz.py,
factories lib/layers/base/lipschitz.py:510-531).

Each layer keeps the reference's parameters and buffers (``weight, bias, scale, u, v`` and for
convs ``initialized, spatial_dims``) so state dicts and checkpoints are interchangeable.  The
effective weight is ``W / max(1, u.(W v) / coeff)``.  On the hot path the MI355X engine computes
that scale and repacks the weights itself (``inf_net_refresh``); the methods here maintain u/v
(power iteration, ``update=True``) and give the plain-tensor forward for direct calls.

The layer is bounded in the induced norm l_domain -> l_codomain (``--vnorms``): any numbers >= 1, ``float('inf')``
included; 2 -> 2 is the spectral norm that every run_*.sh config selects.  Only what produces u and v depends on the
norms: ``normalize_u`` / ``normalize_v`` here (host, construction time) and in csrc/power.hip (device).  A learnable
order (the reference's ``learn_p``: a tensor-valued domain) is out of scope and raises.

Kept from the reference for checkpoint and oracle parity: the one-hot normalisation puts +1 at the
arg-max whatever the sign; a 1x1 conv's stored v (domain 1) / u (codomain inf) is not written back by an update; the
random restarts at construction keep the LAST pair whose scale exceeds the FIRST pair's.
"""
import ctypes
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.nn.init as init

__all__ = ['InducedNormConv2d', 'InducedNormLinear', 'get_conv2d', 'get_linear', 'batch_power_update', 'normalize_u',
           'normalize_v']


def _unit(t):
    return F.normalize(t, p=2, dim=0)


def _one_hot(t):
    """+1 at the first index of max |t|, 0 elsewhere; the sign is dropped (the reference's projmax_)."""
    out = torch.zeros_like(t)
    out[torch.argmax(torch.abs(t))] = 1
    return out


def _power_form(t, e, p):
    """sign(t) a^e / |a^e|_p with a = |t| / max |t| and sign(0) = +1.  e = 0 with p = inf (the limits domain = inf,
    codomain = 1) gives the sign vector: 0^0 = 1 and n^(1/inf) = 1."""
    a = torch.abs(t)
    sign = torch.where(t < 0, -torch.ones_like(t), torch.ones_like(t))
    a = (a / torch.max(a)) ** e
    return sign * a / torch.sum(a ** p) ** (1 / p)


def normalize_v(v, domain):
    """v for the domain's norm (mixed_lipschitz.py:414-426)."""
    if domain == 2:
        return _unit(v)
    if domain == 1:
        return _one_hot(v)
    return _power_form(v, 1 / (domain - 1), domain)


def normalize_u(u, codomain):
    """u for the codomain's norm (mixed_lipschitz.py:429-444)."""
    if codomain == 2:
        return _unit(u)
    if codomain == float('inf'):
        return _one_hot(u)
    return _power_form(u, codomain - 1, float('inf') if codomain == 1 else codomain / (codomain - 1))


def _check_norms(domain, codomain):
    if torch.is_tensor(domain) or torch.is_tensor(codomain):
        raise NotImplementedError('a tensor-valued domain / codomain (the reference\'s learn_p, a learnable order of '
                                  'the induced norm) is out of scope; pass numbers >= 1')
    for p in (domain, codomain):
        if isinstance(p, bool) or not (isinstance(p, (int, float)) and p >= 1):
            raise ValueError('domain / codomain must be numbers >= 1 (float(\'inf\') included), got %r' % (p,))


RESTARTS, RESTART_ITERATIONS = 10, 200      # mixed_lipschitz.py:49-52,225-232


def _power_iterate(apply_w, apply_wt, u, v, max_itrs, atol, rtol, domain=2, codomain=2):
    """u <- normalize_u(W v), v <- normalize_v(W^T u) until both move less than atol + rtol*max
    (mixed_lipschitz.py:295-310,348-368)."""
    used = 0
    for _ in range(max_itrs):
        u_prev, v_prev = u, v
        u = normalize_u(apply_w(v), codomain)
        v = normalize_v(apply_wt(u), domain)
        used += 1
        if atol is not None and rtol is not None:
            du = torch.norm(u - u_prev) / (u.nelement() ** 0.5)
            dv = torch.norm(v - v_prev) / (v.nelement() ** 0.5)
            if du < atol + rtol * torch.max(u) and dv < atol + rtol * torch.max(v):
                break
    _power_iterate.last_used = used
    return u, v


def _native_power_iteration(kind, cin, cout, ksize, hw, W, u, v, scale, itrs, atol, rtol, use_tol, domain=2,
                            codomain=2):
    """inf_power_iteration: the whole loop on the engine, u / v / scale updated in place (a 1x1 conv's v for domain 1
    and u for codomain inf stay as they are, include/inflow.h).  Returns the iteration count.  The version counters
    are bumped so the engine's packed weights refresh."""
    from ... import _hip
    lib = _hip.load()
    d = _hip.PowerIterDesc(kind=kind, cin=cin, cout=cout, ksize=ksize, height=hw[0], width=hw[1],
                           weight=W.data_ptr(), u=u.data_ptr(), v=v.data_ptr(), scale=scale.data_ptr(),
                           domain=float(domain), codomain=float(codomain))
    ws = _hip.workspace(W.device, lib.inf_power_iteration_workspace_bytes(ctypes.byref(d)))
    used = ctypes.c_int(0)
    _hip.check(lib.inf_power_iteration(ctypes.byref(d), int(itrs), int(bool(use_tol)), float(atol or 0.),
                                       float(rtol or 0.), ctypes.byref(used), _hip.ptr(ws), ws.numel(),
                                       _hip.stream_of(W)), 'inf_power_iteration')
    for t in (u, v, scale):
        torch.autograd.graph.increment_version(t)
    return used.value


def _native_one_iter(kind, cin, cout, ksize, hw, W, u, v, domain, codomain):
    """sigma after one iteration from (u, v), on copies: the stored buffers are left alone (compute_one_iter)."""
    scale = W.new_zeros(())
    _native_power_iteration(kind, cin, cout, ksize, hw, W, u.clone(), v.clone(), scale, 1, None, None, False, domain,
                            codomain)
    return scale


def batch_power_update(modules):
    """compute_weight(update=True) for many InducedNorm layers on one device: one engine call
    (inf_power_iteration_batch) per tolerance setting, so the host reads the convergence flags once per
    speculative chunk for all layers.  Each layer's norms travel in its descriptor.  Same per-layer iterations, stopping rule and results as calling
    compute_weight(update=True) on each; layers not yet initialised take that per-layer path."""
    from ... import _hip
    groups, rest = {}, []
    for m in modules:
        if not m.weight.is_cuda:
            rest.append(m)
            continue
        if isinstance(m, InducedNormConv2d):
            if not m._initialized_host():
                rest.append(m)
                continue
            k = m.kernel_size[0]
            if m.kernel_size != (k, k) or m.stride != (1, 1) or m.padding != (k // 2, k // 2):
                rest.append(m)
                continue
            hw = (1, 1) if m.is_1x1 else m._hw()
            d = (1, m.in_channels, m.out_channels, k, hw)
        else:
            d = (2, m.in_features, m.out_features, 1, (1, 1))
        n_iterations, atol, rtol = m.n_iterations, m.atol, m.rtol   # compute_weight's defaults
        itrs = _iteration_budget(n_iterations, atol, rtol)
        key = (m.weight.device, itrs, n_iterations is None, atol, rtol)
        groups.setdefault(key, []).append((m, d))
    for m in rest:
        m.compute_weight(update=True)
    lib = _hip.load() if groups else None
    for (dev, itrs, use_tol, atol, rtol), items in groups.items():
        descs = (_hip.PowerIterDesc * len(items))()
        for j, (m, (kind, cin, cout, ks, hw)) in enumerate(items):
            descs[j] = _hip.PowerIterDesc(kind=kind, cin=cin, cout=cout, ksize=ks, height=hw[0], width=hw[1],
                                          weight=m.weight.data_ptr(), u=m.u.data_ptr(), v=m.v.data_ptr(),
                                          scale=m.scale.data_ptr(), domain=float(m.domain),
                                          codomain=float(m.codomain))
        used = (ctypes.c_int * len(items))()
        ws = _hip.workspace(dev, lib.inf_power_iteration_batch_workspace_bytes(descs, len(items)))
        _hip.check(lib.inf_power_iteration_batch(descs, len(items), int(itrs), int(bool(use_tol)), float(atol or 0.),
                                                 float(rtol or 0.), used, _hip.ptr(ws), ws.numel(),
                                                 _hip.stream_of(m.weight)), 'inf_power_iteration_batch')
        for j, (m, _) in enumerate(items):
            m.last_power_iters = used[j]
            for t in (m.u, m.v, m.scale):
                torch.autograd.graph.increment_version(t)


def _iteration_budget(n_iterations, atol, rtol):
    if n_iterations is None and (atol is None or rtol is None):
        raise ValueError('Need one of n_iteration or (atol, rtol).')
    return n_iterations if n_iterations is not None else 200


class InducedNormLinear(nn.Module):

    def __init__(self, in_features, out_features, bias=True, coeff=0.97, domain=2, codomain=2, n_iterations=None,
                 atol=None, rtol=None, zero_init=False, **unused_kwargs):
        super().__init__()
        _check_norms(domain, codomain)
        self.in_features, self.out_features = in_features, out_features
        self.coeff, self.n_iterations, self.atol, self.rtol = coeff, n_iterations, atol, rtol
        self.domain, self.codomain = domain, codomain
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter('bias', None)
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if zero_init:
            self.weight.data.div_(1000)
        if self.bias is not None:
            bound = 1 / math.sqrt(in_features)
            init.uniform_(self.bias, -bound, bound)
        self.register_buffer('scale', torch.tensor(0.))
        self.register_buffer('u', normalize_u(self.weight.new_empty(out_features).normal_(0, 1), codomain))
        self.register_buffer('v', normalize_v(self.weight.new_empty(in_features).normal_(0, 1), domain))
        with torch.no_grad():
            self.compute_weight(True, n_iterations=200, atol=None, rtol=None)
            # Other norms: the iteration can stop at a local maximum, so the reference tries more random starts.  Its
            # best_scale is never updated: the LAST start that beats the FIRST one is kept, and `scale` is left at
            # the last start's value (mixed_lipschitz.py:43-56).
            first_scale = self.scale.clone()
            best_u, best_v = self.u.clone(), self.v.clone()
            if not (domain == 2 and codomain == 2):
                for _ in range(RESTARTS):
                    self.u.copy_(normalize_u(self.weight.new_empty(out_features).normal_(0, 1), codomain))
                    self.v.copy_(normalize_v(self.weight.new_empty(in_features).normal_(0, 1), domain))
                    self.compute_weight(True, n_iterations=RESTART_ITERATIONS)
                    if self.scale > first_scale:
                        best_u, best_v = self.u.clone(), self.v.clone()
            self.u.copy_(best_u)
            self.v.copy_(best_v)

    def compute_weight(self, update=True, n_iterations=None, atol=None, rtol=None):
        W = self.weight
        if update:
            n_iterations = self.n_iterations if n_iterations is None else n_iterations
            atol = self.atol if atol is None else atol
            rtol = self.rtol if rtol is None else atol          # the reference reads atol here too
            itrs = _iteration_budget(n_iterations, atol, rtol)
            with torch.no_grad():
                tol = (atol, rtol) if n_iterations is None else (None, None)
                if W.is_cuda:
                    self.last_power_iters = _native_power_iteration(
                        2, self.in_features, self.out_features, 1, (1, 1), W.detach(), self.u, self.v, self.scale,
                        itrs, atol, rtol, n_iterations is None, self.domain, self.codomain)
                    if not torch.is_grad_enabled():
                        return W / torch.clamp(self.scale / self.coeff, min=1.)
                else:       # construction-time init on the host (the module is built on CPU, then moved)
                    u, v = _power_iterate(lambda t: torch.mv(W, t), lambda t: torch.mv(W.t(), t), self.u, self.v,
                                          itrs, *tol, self.domain, self.codomain)
                    self.u.copy_(u)
                    self.v.copy_(v)
                    self.last_power_iters = _power_iterate.last_used
        sigma = torch.dot(self.u, torch.mv(W, self.v))
        with torch.no_grad():
            self.scale.copy_(sigma)
        return W / torch.max(torch.ones(1, device=W.device), sigma / self.coeff)

    def compute_domain_codomain(self):
        """(domain, codomain) of the induced norm (mixed_lipschitz.py:68-74): the constructor's numbers (a learnable
        order is not provided)."""
        return self.domain, self.codomain

    def compute_one_iter(self):
        W = self.weight.detach()
        if W.is_cuda:
            return _native_one_iter(2, self.in_features, self.out_features, 1, (1, 1), W, self.u, self.v,
                                    self.domain, self.codomain)
        u = normalize_u(torch.mv(W, self.v), self.codomain)
        v = normalize_v(torch.mv(W.t(), u), self.domain)
        return torch.dot(u, torch.mv(W, v))

    def forward(self, x):
        return F.linear(x, self.compute_weight(update=False), self.bias)

    def extra_repr(self):
        return ('in_features={}, out_features={}, bias={}, coeff={}, domain={:.2f}, codomain={:.2f}, n_iters={}, '
                'atol={}, rtol={}').format(self.in_features, self.out_features, self.bias is not None, self.coeff,
                                           self.domain, self.codomain, self.n_iterations, self.atol, self.rtol)


class InducedNormConv2d(nn.Module):

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, bias=True, coeff=0.97, domain=2,
                 codomain=2, n_iterations=None, atol=None, rtol=None, **unused_kwargs):
        super().__init__()
        _check_norms(domain, codomain)
        pair = lambda a: tuple(a) if isinstance(a, (tuple, list)) else (a, a)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding = pair(kernel_size), pair(stride), pair(padding)
        self.coeff, self.n_iterations, self.atol, self.rtol = coeff, n_iterations, atol, rtol
        self.domain, self.codomain = domain, codomain
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(in_channels * self.kernel_size[0] * self.kernel_size[1])
            init.uniform_(self.bias, -bound, bound)
        self.register_buffer('initialized', torch.tensor(0))
        self.register_buffer('spatial_dims', torch.tensor([1., 1.]))
        self.register_buffer('scale', torch.tensor(0.))
        self.register_buffer('u', self.weight.new_empty(out_channels))
        self.register_buffer('v', self.weight.new_empty(in_channels))

    # u/v are sized by the first input's spatial dims; accept checkpoints whatever the current size
    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for name in ('u', 'v'):
            key = prefix + name
            if key in state_dict and state_dict[key].shape != getattr(self, name).shape:
                setattr(self, name, getattr(self, name).new_empty(state_dict[key].shape))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @property
    def is_1x1(self):
        return self.kernel_size == (1, 1)

    def _hw(self):
        """spatial_dims as ints; read from the device only when the buffer changed (no sync per call)."""
        t = self.spatial_dims
        key = (t.data_ptr(), t._version)
        c = self.__dict__.get('_hw_cache')
        if c is None or c[0] != key:
            h, w = t.tolist()
            c = self.__dict__['_hw_cache'] = (key, (int(h), int(w)))
        return c[1]

    def _initialized_host(self):
        """bool(self.initialized) without a device sync once it is known to be set."""
        t = self.initialized
        key = (t.data_ptr(), t._version)
        c = self.__dict__.get('_init_cache')
        if c is None or c[0] != key:
            c = self.__dict__['_init_cache'] = (key, bool(t.item()))
        return c[1]

    def _conv_ops(self, W):
        c = self.in_channels
        h, w = self._hw()
        fwd = lambda t: F.conv2d(t.view(1, c, h, w), W, stride=self.stride, padding=self.padding).reshape(-1)
        shape = F.conv2d(torch.zeros(1, c, h, w, device=W.device, dtype=W.dtype), W, stride=self.stride,
                         padding=self.padding).shape
        bwd = lambda t: F.conv_transpose2d(t.view(shape), W, stride=self.stride, padding=self.padding).reshape(-1)
        return fwd, bwd, shape

    def _initialize_u_v(self):
        """mixed_lipschitz.py:195-239: random normalised u/v, then power iteration; for norms other than 2 -> 2, ten
        more random starts under the reference's rule (see InducedNormLinear.__init__) and in its order of draws."""
        domain, codomain = self.domain, self.codomain
        new = lambda n: self.weight.new_empty(n).normal_(0, 1)
        with torch.no_grad():
            if self.is_1x1:
                nu, nv = self.out_channels, self.in_channels
                self.u = normalize_u(new(nu), codomain)
                self.v = normalize_v(new(nv), domain)
            else:
                h, w = self._hw()
                nv = self.in_channels * h * w
                self.v = normalize_v(new(nv), domain)
                _, _, shape = self._conv_ops(self.weight)
                nu = int(torch.Size(shape).numel())
                self.u = normalize_u(new(nu), codomain)
                new = lambda n: torch.randn(n).to(self.weight)      # the k x k restarts draw on the host
            self.initialized.fill_(1)
            self.compute_weight(True)
            first_scale = self.scale.clone()
            best_u, best_v = self.u.clone(), self.v.clone()
            if not (domain == 2 and codomain == 2):
                for _ in range(RESTARTS):
                    self.u.copy_(normalize_u(new(nu), codomain))
                    self.v.copy_(normalize_v(new(nv), domain))
                    self.compute_weight(True, n_iterations=RESTART_ITERATIONS)
                    if self.scale > first_scale:
                        best_u, best_v = self.u.clone(), self.v.clone()
            self.u.copy_(best_u)
            self.v.copy_(best_v)

    def compute_weight(self, update=True, n_iterations=None, atol=None, rtol=None):
        if not self._initialized_host():
            self._initialize_u_v()
        n_iterations = self.n_iterations if n_iterations is None else n_iterations
        atol = self.atol if atol is None else atol
        rtol = self.rtol if rtol is None else atol              # the reference reads atol here too
        itrs = _iteration_budget(n_iterations, atol, rtol)
        W = self.weight
        if self.is_1x1:
            Wm = W.view(self.out_channels, self.in_channels)
            fwd, bwd = (lambda t: torch.mv(Wm, t)), (lambda t: torch.mv(Wm.t(), t))
        else:
            fwd, bwd, _ = self._conv_ops(W)
        u, v = self.u.view(-1), self.v.view(-1)
        if update:
            # The reference's 1x1 path normalises a temporary where the result is one-hot and copies back only the
            # other forms (mixed_lipschitz.py:311-315): the stored v (domain 1) / u (codomain inf) stays as it was,
            # while sigma below comes from the iterated vectors.
            stale_u = self.is_1x1 and self.codomain == float('inf')
            stale_v = self.is_1x1 and self.domain == 1
            with torch.no_grad():
                tol = (atol, rtol) if n_iterations is None else (None, None)
                if W.is_cuda:
                    k = self.kernel_size[0]
                    if self.kernel_size != (k, k) or self.stride != (1, 1) or self.padding != (k // 2, k // 2):
                        raise NotImplementedError('engine power iteration: square kernels, stride 1, padding k//2')
                    hw = (1, 1) if self.is_1x1 else self._hw()
                    args = (self.in_channels, self.out_channels, self.kernel_size[0], hw, W.detach())
                    tail = (self.scale, itrs, atol, rtol, n_iterations is None, self.domain, self.codomain)
                    if torch.is_grad_enabled() and (stale_u or stale_v):
                        # sigma below needs the iterated vectors: the same iteration as a linear layer (which
                        # writes both back) on copies, then store what the reference stores
                        u, v = self.u.clone(), self.v.clone()
                        self.last_power_iters = _native_power_iteration(2, *args, u, v, *tail)
                        if not stale_u:
                            self.u.copy_(u)
                        if not stale_v:
                            self.v.copy_(v)
                    else:
                        self.last_power_iters = _native_power_iteration(1, *args, self.u, self.v, *tail)
                    if not torch.is_grad_enabled():
                        return W / torch.clamp(self.scale / self.coeff, min=1.)
                else:       # construction-time init on the host (the module is built on CPU, then moved)
                    u, v = _power_iterate(fwd, bwd, u, v, itrs, *tol, self.domain, self.codomain)
                    if not stale_u:
                        self.u.copy_(u.view_as(self.u))
                    if not stale_v:
                        self.v.copy_(v.view_as(self.v))
                    self.last_power_iters = _power_iterate.last_used
        sigma = torch.dot(u, fwd(v))
        with torch.no_grad():
            self.scale.copy_(sigma)
        return W / torch.max(torch.ones(1, device=W.device), sigma / self.coeff)

    def compute_domain_codomain(self):
        """(domain, codomain) of the induced norm (mixed_lipschitz.py:180-186): the constructor's numbers."""
        return self.domain, self.codomain

    def compute_one_iter(self):
        if not self.initialized:
            raise ValueError('Layer needs to be initialized first.')
        W = self.weight.detach()
        if self.is_1x1:
            Wm = W.view(self.out_channels, self.in_channels)
            fwd, bwd = (lambda t: torch.mv(Wm, t)), (lambda t: torch.mv(Wm.t(), t))
        else:
            fwd, bwd, _ = self._conv_ops(W)
        if W.is_cuda:
            # a 1x1 conv is the linear layer of its (cout, cin) matrix; that kind returns both vectors
            return _native_one_iter(2 if self.is_1x1 else 1, self.in_channels, self.out_channels,
                                    self.kernel_size[0], (1, 1) if self.is_1x1 else self._hw(), W, self.u, self.v,
                                    self.domain, self.codomain)
        u = normalize_u(fwd(self.v.view(-1)), self.codomain)
        v = normalize_v(bwd(u), self.domain)
        return torch.dot(u, fwd(v))

    def forward(self, x):
        if not self._initialized_host():
            self.spatial_dims.copy_(torch.tensor(x.shape[2:4]).to(self.spatial_dims))
        return F.conv2d(x, self.compute_weight(update=False), self.bias, self.stride, self.padding, 1, 1)

    def extra_repr(self):
        return ('{}, {}, kernel_size={}, stride={}, padding={}, coeff={}, domain={:.2f}, codomain={:.2f}, n_iters={}, '
                'atol={}, rtol={}').format(self.in_channels, self.out_channels, self.kernel_size, self.stride,
                                           self.padding, self.coeff, self.domain, self.codomain, self.n_iterations,
                                           self.atol, self.rtol)


def _closed_form(domain, codomain):
    """The norm pairs for which the reference's factories build LopLinear / LopConv2d (the closed-form operator norms
    max column / row norm with a per-column / per-row scale, lipschitz.py:274-366,510-531) instead of an InducedNorm
    layer.  Those layers are not provided: an InducedNorm layer in their place would compute another function (one
    scalar scale) and could not load their checkpoints (no u / v), so the factories refuse the pair."""
    inf = float('inf')
    return (domain == 1 and codomain in (1, 2, inf)) or (codomain == inf and domain in (2, inf))


def _refuse_closed_form(domain, codomain):
    if not torch.is_tensor(domain) and not torch.is_tensor(codomain) and _closed_form(domain, codomain):
        raise NotImplementedError('the reference bounds a %s -> %s layer with its closed-form LopLinear / LopConv2d, '
                                  'which is not provided (InducedNormLinear / InducedNormConv2d take the pair when '
                                  'built directly)' % (domain, codomain))


def get_linear(in_features, out_features, bias=True, coeff=0.97, domain=None, codomain=None, **kwargs):
    """lipschitz.py:510-518: InducedNormLinear bounded in the l_domain -> l_codomain induced norm (numbers >= 1,
    float('inf') included; None stands for 2).  Pairs the reference gives to LopLinear raise (_closed_form)."""
    _refuse_closed_form(2 if domain is None else domain, 2 if codomain is None else codomain)
    return InducedNormLinear(in_features, out_features, bias, coeff, 2 if domain is None else domain,
                             2 if codomain is None else codomain, **kwargs)


def get_conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=True, coeff=0.97, domain=None,
               codomain=None, **kwargs):
    """lipschitz.py:521-531: InducedNormConv2d bounded in the l_domain -> l_codomain induced norm (numbers >= 1,
    float('inf') included; None stands for 2).  Pairs the reference gives to LopConv2d raise (_closed_form)."""
    _refuse_closed_form(2 if domain is None else domain, 2 if codomain is None else codomain)
    return InducedNormConv2d(in_channels, out_channels, kernel_size, stride, padding, bias, coeff,
                             2 if domain is None else domain, 2 if codomain is None else codomain, **kwargs)
