"""Golden vectors for images that do not cut into whole 32- or 64-pixel tiles, from the reference itself (build
container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ragged.py [case ...]

Same harness as make_golden.py (its import shims, model builders and capture hooks, reused by import) and
make_golden_acts.py's ``stable``: every case runs the reference with 1 and with 8 torch threads and is written only if
the two runs agree in every block's Broyden ``nstep`` / ``lowest_step`` and series lengths.

``mnist_b2``: the reference's ``--data mnist`` shape (train_img.py:256-258: one channel, ``LogitTransform(1e-6)``) at
``--imagesize 28``, lib/synthetic.py ``MNIST_SMALL``: ``ImplicitFlow`` eval on (2, 1, 28, 28) with n_blocks [1, 1, 1],
idim 256, swish, vnorms '2222' (make_golden.conv_model's).  Its scales are 28x28, 14x14 and 7x7: 784, 196 and 49
pixels, none a multiple of 32, which the fused 3-1-3 kernels run as ragged whole-row tiles.  The
weights are ``syn.make_state_dict(MNIST_SMALL, 0)`` and are not stored; the fixture holds the input, the flow's
outputs, and per block z, log-det, Broyden ``nstep`` / ``lowest_step`` and the series lengths.
"""
import sys

import make_golden_acts as mga  # noqa: E402  (make_golden's shims + reference import + hooks, and stable())

mg = mga.mg
syn = mg.syn

ARCH = syn.CONFIGS['mnist_small']


def _mnist_b2():
    x = syn.image_batch(2, input_size=ARCH['input_size'], nvals=ARCH['nvals'], seed=3)
    mga.stable('mnist_b2', lambda: mg.run_case('mnist_b2', ARCH, x, seed=7))


CASES = {'mnist_b2': _mnist_b2}

if __name__ == '__main__':
    for n in sys.argv[1:] or list(CASES):
        CASES[n]()
