"""Per-launch event times of the per-layer GEMMs of d-128-128-d Sin nets under both values of INF_OPT_FC_SKINNY."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'implicit-normalizing-flows_amd'))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
from lib import _hip, synthetic as syn
from lib.layers import base as bl
from lib.layers.base import Sin
DEV = 'cuda:0'
for d, B in ((3072, 64), (43, 1000), (1025, 64)):
    torch.manual_seed(0)
    lin = lambda a, b: bl.get_linear(a, b, coeff=0.97, n_iterations=None, atol=1e-3, rtol=1e-3, domain=2, codomain=2)
    net = torch.nn.Sequential(lin(d, 128), Sin(), lin(128, 128), Sin(), lin(128, d))
    net(torch.zeros(1, d))
    net = net.to(DEV)
    n = _hip.native_net(net, (d,), torch.device(DEV))
    x = syn.tabular_batch(B, d, seed=1).to(DEV)
    v = syn.tabular_batch(B, d, seed=2).to(DEV)
    stream = _hip.stream_of(x)
    n.refresh_if_needed(stream)
    ws = torch.empty(n.ws_bytes(B), dtype=torch.uint8, device=DEV)
    y = torch.empty_like(x)
    for opt in (0, 1):
        n.set_option(_hip.INF_OPT_FC_SKINNY, opt)
        for rep in range(2):
            _hip.profile_begin(10000)
            for _ in range(20):
                _hip.check(n.lib.inf_net_forward(n.handle, _hip.ptr(x), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream), 'f')
                _hip.check(n.lib.inf_net_vjp(n.handle, _hip.ptr(x), _hip.ptr(v), _hip.ptr(y), B, _hip.ptr(ws), ws.numel(), stream), 'v')
            torch.cuda.synchronize()
            st = _hip.profile_end()
        print('d %d B %d option %d: ' % (d, B, opt) + '; '.join('%s x%d %.1f us' % (_hip.tag_name(s['tag']), s['launches'], 1000 * s['total_ms'] / s['launches']) for s in sorted(st, key=lambda s: s['tag'])), flush=True)
