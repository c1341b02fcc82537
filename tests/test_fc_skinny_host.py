"""Host side of the skinny GEMM family of wide fc nets: the option constant against the header, the
option call on a null net, and the launch-profile names of tags 960-962.  No GPU."""
import os
import re

from lib import _hip

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'inflow.h')


def test_option_constant_equals_the_header():
    text = open(HEADER).read()
    m = re.search(r'\bINF_OPT_FC_SKINNY\s*=\s*(\d+)', text)
    assert m and int(m.group(1)) == _hip.INF_OPT_FC_SKINNY == 9
    assert re.search(r'\*\s+INF_OPT_FC_SKINNY\s', text)                 # documented with its neighbours


def test_option_on_a_null_net_is_invalid():
    lib = _hip.load()
    assert lib.inf_net_set_option(None, _hip.INF_OPT_FC_SKINNY, 0) == -1
    assert lib.inf_net_get_option(None, _hip.INF_OPT_FC_SKINNY) < 0


def test_tag_names():
    names = [_hip.tag_name(t) for t in (960, 961, 962)]
    assert names == ['gemm_skinny_kernel<split-K partial>', 'gemm_skinny_reduce_kernel',
                     'gemm_skinny_kernel<small tile>']
    assert _hip.tag_name(950).startswith('fc_out_wide_kernel') and _hip.tag_name(2222061).startswith('gemm_f32_kernel')
