"""Selection of the two-pass staging variant of the stage-2 3x3 fp32 conv (ConvArgs::twopass,
csrc/hip/cnn_conv_fast.hip): only launches that set the field get it, only on the 8-row tile, with the grid and
block of the default kernel and half its LDS. No GPU needed."""

import pytest

from test_conv_dispatch_table import CONV_SEL, conv_args, select
from test_hip_fp32 import K

LDS_LIMIT = 53 * 1024
S2 = (3, 56, 56, 16, 16, 1)                 # k, cinp, coutp, H, W, prec
BIG = ((25, 32), (80, 32), (5, 32))         # launches on the 8-row tile (>= 300 workgroups)
SMALL = ((1, 32), (2, 32), (4, 32), (2, 8))   # launches the small-launch rule moves to 4- / 2-row tiles


def _args(Km, ng, B, epi, two, shape=S2, cr=50):
    a = conv_args(Km, shape + (ng, B, cr, epi))
    a.twopass = two
    return a


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("ng,B", BIG)
def test_twopass_selected_on_the_8_row_tile(ng, B, epi):
    Km = K()
    L = Km.lib()
    off = select(L, "gt_conv_fast_select", _args(Km, ng, B, epi, 0), CONV_SEL)
    on = select(L, "gt_conv_fast_select", _args(Km, ng, B, epi, 1), CONV_SEL)
    assert off[4] == 8 and L.gt_conv_fast_twopass(_args(Km, ng, B, epi, 0)) == 0
    assert L.gt_conv_fast_twopass(_args(Km, ng, B, epi, 1)) == 1
    assert on[:13] == off[:13]                       # the same tile shape ...
    assert on[15:19] == off[15:19]                   # ... grid and block
    assert on[19] <= LDS_LIMIT < off[19] and on[19] in (on[13], on[14])
    assert 3 * (on[19] + 256) <= 160 * 1024          # three workgroups (+ the static offset table) per CU


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("ng,B", SMALL)
def test_small_launch_tiles_ignore_the_field(ng, B, epi):
    Km = K()
    L = Km.lib()
    off = select(L, "gt_conv_fast_select", _args(Km, ng, B, epi, 0), CONV_SEL)
    assert off[4] in (2, 4)
    assert select(L, "gt_conv_fast_select", _args(Km, ng, B, epi, 1), CONV_SEL) == off
    assert L.gt_conv_fast_twopass(_args(Km, ng, B, epi, 1)) == 0


def test_other_shapes_ignore_the_field():
    """Every other fp32 / bf16 geometry of the search spaces selects the same kernel with the field set."""
    Km = K()
    L = Km.lib()
    for shape in [(5, 24, 56, 16, 16, 1), (5, 56, 24, 16, 16, 1), (3, 24, 24, 32, 32, 1), (3, 56, 56, 16, 16, 0),
                  (3, 104, 104, 8, 8, 1), (3, 128, 128, 16, 16, 1), (3, 64, 64, 16, 16, 1), (3, 56, 56, 12, 16, 1)]:
        for ng, B in BIG + SMALL:
            off = select(L, "gt_conv_fast_select", _args(Km, ng, B, 1, 0, shape, 0), CONV_SEL)
            assert select(L, "gt_conv_fast_select", _args(Km, ng, B, 1, 1, shape, 0), CONV_SEL) == off, (shape, ng, B)
            assert L.gt_conv_fast_twopass(_args(Km, ng, B, 1, 1, shape, 0)) == (-1 if off is None else 0)
