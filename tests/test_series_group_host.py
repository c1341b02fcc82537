"""The rule that picks the sample groups of a fused conv series (inf_series_group: a pure function, no device).

The rule, in bytes and tiles (include/inflow.h): the derivative planes live between two terms are
concurrent x nnets x group x H W x hidden x 4 B x 2 (d1 and d2); where the whole batch's exceed the 256 MiB budget, the
group is the largest whose planes do not and whose launches -- the short last group's too -- run on the kernel family of
the whole batch's VJP launch (inf_net313_kernel_family); the batch itself (one group) otherwise.
"""
import itertools

from lib import _hip

HID = 512
BUDGET = 256 << 20
MODE_VJP = 2
FAM_K128 = 3


def _family(lib, C, H, W, B, nnets, pol, h3):
    return lib.inf_net313_kernel_family(HID, C, H, W, B, nnets, nnets, pol, MODE_VJP, h3)


def _group(lib, C, H, W, B, nnets, concurrent, pol=1, h3=1):
    return lib.inf_series_group(HID, C, H, W, B, nnets, concurrent, pol, h3)


def _plane_bytes(H, W, samples, nnets, concurrent):
    return concurrent * nnets * samples * H * W * HID * 4 * 2


def test_rule_table():
    lib = _hip.load()
    # the 32x32 scale at B = 64, x- and z-branch chains side by side: 32 samples, 128 MiB per chain
    assert _group(lib, 3, 32, 32, 64, 1, 2) == 32
    assert _plane_bytes(32, 32, 32, 1, 2) == BUDGET
    # ... as one pair chain (INF_OPT_EVAL_OVERLAP = 0): the same 32; one net alone holds 256 MiB: one group
    assert _group(lib, 3, 32, 32, 64, 2, 1) == 32
    assert _group(lib, 3, 32, 32, 64, 1, 1) == 64
    # the 16x16 scale at B = 64, pair: 128 MiB, within the budget
    assert _plane_bytes(16, 16, 64, 2, 1) == BUDGET // 2
    assert _group(lib, 12, 16, 16, 64, 2, 1) == 64
    # B = 256 (the per-GPU batch of the C4 configuration): the pair's 16x16 planes are 512 MiB; 128 samples keep the
    # 128-pixel kernel (2 nets x 128 x 2 tiles = 512 workgroups)
    assert _group(lib, 12, 16, 16, 256, 2, 1) == 128
    assert _family(lib, 12, 16, 16, 128, 2, 1, 1) == FAM_K128 == _family(lib, 12, 16, 16, 256, 2, 1, 1)
    assert _group(lib, 3, 32, 32, 256, 1, 2) == 32
    # B = 63 at 32x32, two chains: 32 + 31 would put the last group under the 128-pixel kernel's 256 tiles (31 x 8), and
    # no smaller group reaches them either: one group
    assert _group(lib, 3, 32, 32, 63, 1, 2) == 63
    # ... with that kernel forced wherever it fits (policy 2) or off (policy 0) the grid no longer decides it between
    # 16 and 63 samples of 16 64-pixel tiles, and 32 + 31 is taken
    assert _group(lib, 3, 32, 32, 63, 1, 2, pol=2) == 32
    assert _group(lib, 3, 32, 32, 63, 1, 2, pol=0) == 32
    # the 8x8 scale has no 128-pixel tile: a batch large enough to exceed the budget is cut by bytes (512 KiB per
    # sample of a pair), on the same kernel before and after
    assert _group(lib, 48, 8, 8, 4096, 2, 1) == 512
    assert _family(lib, 48, 8, 8, 512, 2, 1, 1) == _family(lib, 48, 8, 8, 4096, 2, 1, 1)
    # invalid arguments and shapes without a fused kernel
    assert _group(lib, 3, 32, 32, 0, 1, 1) < 0 and _group(lib, 3, 32, 32, 64, 3, 1) < 0
    assert _group(lib, 3, 32, 32, 64, 1, 0) < 0
    assert lib.inf_series_group(384, 3, 32, 32, 64, 1, 1, 1, 1) < 0


def test_group_is_the_largest_that_keeps_bytes_and_family():
    """Over the CIFAR-10 and CelebA-HQ 256 scales, batches around the thresholds, every policy and both operand kinds:
    a group smaller than the batch is within the budget and on the batch's family, its short last group too, and no
    larger one is; the batch is returned only when it fits the budget or no smaller group qualifies."""
    lib = _hip.load()
    shapes = [(3, 32, 32), (12, 16, 16), (48, 8, 8), (3, 256, 256), (12, 128, 128), (48, 64, 64)]
    batches = [1, 4, 31, 32, 33, 63, 64, 65, 100, 128, 256, 300]
    for (C, H, W), B, nnets, conc, pol, h3 in itertools.product(shapes, batches, (1, 2), (1, 2), (0, 1, 2, 3), (0, 1)):
        fam = _family(lib, C, H, W, B, nnets, pol, h3)
        assert fam >= 0
        g = _group(lib, C, H, W, B, nnets, conc, pol, h3)
        case = (C, H, W, B, nnets, conc, pol, h3, g)

        def admissible(k):
            return (_plane_bytes(H, W, k, nnets, conc) <= BUDGET and _family(lib, C, H, W, k, nnets, pol, h3) == fam and
                    (B % k == 0 or _family(lib, C, H, W, B % k, nnets, pol, h3) == fam))
        assert 1 <= g <= B, case
        if _plane_bytes(H, W, B, nnets, conc) <= BUDGET:
            assert g == B, case
            continue
        best = next((k for k in range(B - 1, 0, -1) if admissible(k)), B)
        assert g == best, case + (best,)
