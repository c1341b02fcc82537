"""Golden TRAINING vector for a tabular flow wider than 16 features, from the reference itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_widetrain.py [case ...]

``tab_d43_train_b16``: one ``loss.backward()`` of lib/synthetic.py's TAB_D43 (train_tabular.py's flow at MINIBOONE's
width: four imBlocks over 43-128-128-43 Sin nets, neumann_grad=False, grad_in_forward=False -- the basic power series
with create_graph=True) on ``tabular_batch(16, 43)``, by make_golden_train.run_train_case.

Kept under make_golden_widefc.stable_train's rule: the reference runs with 1 and with 8 torch threads, and the case is
written only if both give every block the same forward nstep and series lengths, the same loss to 1e-6, and every
recorded gradient within a quarter of tests/test_gpu_train.py::_check_grads' bounds.  The implicit backward's step
counts are not stored: eps_backward = 1e-10 is below what fp32 reaches, so they follow the summation order
(make_golden_widefc.py's docstring).  Input seed 3, run seed 7 (make_golden_widefc.py's, the first tried).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_train as mgt  # noqa: E402  (run_train_case)
import make_golden_widefc as mgw  # noqa: E402  (stable_train)

syn = mgt.syn

CASES = {
    'tab_d43_train_b16': lambda: mgw.stable_train('tab_d43_train_b16', lambda: mgt.run_train_case(
        'tab_d43_train_b16', syn.TAB_D43, syn.tabular_batch(16, 43, seed=3), seed=7)),
}

if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        CASES[n]()
