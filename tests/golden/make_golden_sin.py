"""Golden vectors for Sin image flows (the reference image driver's default activation, train_img.py --act), with the
leading activation of preact, from the reference itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sin.py [case ...]

Same harness as make_golden_acts.py (make_golden.py's import shims, model builders and capture hooks,
make_golden_train.py's backward hooks, and make_golden_acts.stable): every case runs the reference with 1 and with 8
torch threads and is written only if both runs give every block the same Broyden ``nstep`` / ``lowest_step`` and series
lengths.  Sin is smooth, so there is no perturbed-input check (make_golden_acts.py's, for the kinked activations).
The architectures are lib/synthetic.py ``CONFIGS['cifar10_small_sin']`` and ``CONFIGS['cifar10_sin']`` (preact=True, the
image architectures' own setting: every net but the first block's leads with a Sin) and, for the fc_end blocks,
``CONFIGS['fcend_small_sin']`` on 3 x 8 x 8 (make_golden_widefc.py's builder: the FCNets over d = 192 lead with a Sin too).
Seeds are make_golden_acts.py's.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_acts as mga  # noqa: E402  (stable(); imports make_golden / make_golden_train)
import make_golden_widefc as mgw  # noqa: E402  (stable() with the fc_end / fc model builder)

mg, mgt, syn = mga.mg, mga.mgt, mga.syn

CASES = {
    'sin_small_b2': lambda: mga.stable('sin_small_b2', lambda: mg.run_case(
        'sin_small_b2', syn.CONFIGS['cifar10_small_sin'], syn.image_batch(2, seed=3), seed=7)),
    'sin_full_b2': lambda: mga.stable('sin_full_b2', lambda: mg.run_case(
        'sin_full_b2', syn.CONFIGS['cifar10_sin'], syn.image_batch(2, seed=3), seed=7)),
    'sin_fcend_small_b2': lambda: mgw.stable('sin_fcend_small_b2', lambda: mg.run_case(
        'sin_fcend_small_b2', syn.CONFIGS['fcend_small_sin'], syn.image_batch(2, mgw.IMG, seed=3), seed=7)),
    'sin_small_train_b2': lambda: mga.stable('sin_small_train_b2', lambda: mgt.run_train_case(
        'sin_small_train_b2', syn.CONFIGS['cifar10_small_sin'], syn.image_batch(2, seed=21), seed=5)),
}

if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        CASES[n]()
