"""Host decisions of the U-Net C entry points (red-diffeq_amd/csrc/unet.hip): the workspace and ticket sizes
they report and the calls they reject.  CPU only: the size functions compute on the host, and every rejected
call returns RDQ_E_INVALID before any HIP call, so nothing here needs (or touches) a GPU.

The values were recorded from the library as it was before its host paths were consolidated (one argument
builder per conv family, one GroupNorm launcher), so they pin what that consolidation must keep."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from red_diffeq import _hip

# (B, cin1, cin2, H = W, cout, k, pad, in_mode) -> (rdq_conv2d_ws_bytes, rdq_conv2d_tickets, rdq_conv2d_gn_ws_bytes,
# rdq_conv2d_gn_sc_ws_bytes, rdq_conv2d_gn_sc_tickets, rdq_conv2d_bf16_wpack_bytes, rdq_conv2d_bf16_ws_bytes,
# rdq_conv2d_bf16_gn_ws_bytes) at G = 8, cout_s = cout and default options
SIZES = {
    # the dim-64 U-Net's convs at 72 / 36 / 18 / 9 pixels (stem, blocks, to_qkv / to_out, unshuffle downsamples,
    # concat blocks and their 1x1 shortcuts, upsample convs, final conv), B = 1
    (1, 1, 0, 72, 64, 7, 3, 0): (0, 162, 0, 0, 324, 200704, 13271040, 0),
    (1, 64, 0, 72, 64, 3, 1, 0): (0, 162, 1368576, 1368576, 324, 73728, 5308416, 0),
    (1, 64, 0, 72, 384, 1, 0, 0): (0, 972, 0, 0, 1944, 49152, 0, 0),
    (1, 128, 0, 72, 64, 1, 0, 0): (0, 162, 1368576, 0, 324, 16384, 0, 0),
    (1, 256, 0, 36, 64, 1, 0, 2): (0, 41, 342272, 0, 82, 32768, 663552, 0),
    (1, 64, 64, 72, 64, 3, 1, 0): (2654208, 162, 4022784, 4022784, 324, 147456, 11943936, 0),
    (1, 64, 64, 72, 64, 1, 0, 0): (0, 162, 1368576, 0, 324, 16384, 0, 0),
    (1, 128, 0, 72, 64, 3, 1, 1): (2654208, 162, 4022784, 0, 324, 147456, 11943936, 0),
    (1, 64, 0, 72, 1, 1, 0, 0): (0, 162, 0, 0, 324, 128, 0, 0),
    (1, 64, 0, 36, 64, 3, 1, 0): (671744, 41, 1014016, 1014016, 82, 73728, 1327104, 0),
    (1, 64, 0, 36, 384, 1, 0, 0): (0, 246, 0, 0, 492, 49152, 0, 0),
    (1, 256, 0, 18, 128, 1, 0, 2): (0, 22, 168704, 0, 44, 65536, 331776, 0),
    (1, 128, 64, 36, 128, 3, 1, 0): (2015232, 82, 2689280, 2689280, 164, 442368, 7299072, 0),
    (1, 128, 64, 36, 128, 1, 0, 0): (0, 82, 674048, 0, 164, 49152, 0, 0),
    (1, 256, 0, 36, 128, 3, 1, 1): (2015232, 82, 2689280, 0, 164, 589824, 11943936, 0),
    (1, 128, 0, 18, 128, 3, 1, 0): (720896, 22, 889600, 889600, 44, 294912, 1492992, 0),
    (1, 128, 0, 18, 384, 1, 0, 0): (0, 66, 0, 0, 132, 98304, 0, 0),
    (1, 512, 0, 9, 256, 1, 0, 2): (196608, 12, 280320, 0, 24, 262144, 331776, 0),
    (1, 256, 128, 18, 256, 3, 1, 0): (1802240, 44, 2136832, 2857728, 88, 1769472, 8957952, 0),
    (1, 256, 128, 18, 256, 1, 0, 0): (720896, 44, 1055488, 0, 88, 196608, 995328, 0),
    (1, 512, 0, 18, 256, 3, 1, 1): (1802240, 44, 2136832, 0, 88, 2359296, 11943936, 0),
    (1, 256, 0, 9, 256, 3, 1, 0): (786432, 12, 870144, 870144, 24, 1179648, 1492992, 0),
    (1, 256, 0, 9, 384, 1, 0, 0): (0, 18, 0, 0, 36, 196608, 248832, 0),
    (1, 256, 0, 9, 512, 3, 1, 0): (1572864, 24, 1739520, 1739520, 48, 2359296, 2985984, 0),
    (1, 512, 0, 9, 512, 3, 1, 0): (1966080, 24, 2132736, 2525952, 48, 4718592, 5971968, 0),
    (1, 512, 0, 9, 384, 1, 0, 0): (294912, 18, 0, 0, 36, 393216, 497664, 0),
    (1, 128, 0, 9, 512, 1, 0, 0): (0, 24, 166656, 0, 48, 131072, 0, 0),
    (1, 512, 256, 9, 512, 3, 1, 0): (1966080, 24, 2132736, 2919168, 48, 7077888, 8957952, 0),
    (1, 512, 256, 9, 512, 1, 0, 0): (786432, 24, 953088, 0, 48, 786432, 995328, 0),
    # ... B = 8
    (8, 1, 0, 72, 64, 7, 3, 0): (0, 1296, 0, 0, 2592, 200704, 21233664, 0),
    (8, 64, 0, 72, 64, 3, 1, 0): (0, 1296, 10948608, 10948608, 2592, 73728, 21233664, 10658304),
    (8, 64, 0, 72, 384, 1, 0, 0): (0, 7776, 0, 0, 15552, 49152, 0, 0),
    (8, 128, 0, 72, 64, 1, 0, 0): (0, 1296, 10948608, 0, 2592, 16384, 0, 0),
    (8, 256, 0, 36, 64, 1, 0, 2): (0, 324, 2737152, 0, 648, 32768, 5308416, 0),
    (8, 64, 64, 72, 64, 3, 1, 0): (0, 1296, 10948608, 10948608, 2592, 147456, 21233664, 10658304),
    (8, 64, 64, 72, 64, 1, 0, 0): (0, 1296, 10948608, 0, 2592, 16384, 0, 0),
    (8, 128, 0, 72, 64, 3, 1, 1): (0, 1296, 10948608, 0, 2592, 147456, 21233664, 10658304),
    (8, 64, 0, 72, 1, 1, 0, 0): (0, 1296, 0, 0, 2592, 128, 0, 0),
    (8, 64, 0, 36, 64, 3, 1, 0): (0, 324, 2737152, 2737152, 648, 73728, 10616832, 0),
    (8, 64, 0, 36, 384, 1, 0, 0): (0, 1944, 0, 0, 3888, 49152, 0, 0),
    (8, 256, 0, 18, 128, 1, 0, 2): (0, 162, 1347840, 0, 324, 65536, 2654208, 0),
    (8, 128, 64, 36, 128, 3, 1, 0): (0, 648, 5391360, 5391360, 1296, 442368, 37158912, 5318912),
    (8, 128, 64, 36, 128, 1, 0, 0): (0, 648, 5391360, 0, 1296, 49152, 0, 0),
    (8, 256, 0, 36, 128, 3, 1, 1): (0, 648, 5391360, 0, 1296, 589824, 37158912, 5318912),
    (8, 128, 0, 18, 128, 3, 1, 0): (2654208, 162, 4002048, 4002048, 324, 294912, 11943936, 0),
    (8, 128, 0, 18, 384, 1, 0, 0): (0, 486, 0, 0, 972, 98304, 0, 0),
    (8, 512, 0, 9, 256, 1, 0, 2): (1376256, 84, 2045184, 0, 168, 262144, 2654208, 0),
    (8, 256, 128, 18, 256, 3, 1, 0): (0, 324, 2674944, 2674944, 648, 1769472, 31850496, 0),
    (8, 256, 128, 18, 256, 1, 0, 0): (0, 324, 2674944, 0, 648, 196608, 7962624, 0),
    (8, 512, 0, 18, 256, 3, 1, 1): (0, 324, 2674944, 0, 648, 2359296, 31850496, 0),
    (8, 256, 0, 9, 256, 3, 1, 0): (2064384, 84, 2733312, 2733312, 168, 1179648, 11943936, 0),
    (8, 256, 0, 9, 384, 1, 0, 0): (0, 126, 0, 0, 252, 196608, 1990656, 0),
    (8, 256, 0, 9, 512, 3, 1, 0): (2752512, 168, 4084992, 4084992, 336, 2359296, 23887872, 0),
    (8, 512, 0, 9, 512, 3, 1, 0): (2752512, 168, 4084992, 4084992, 336, 4718592, 27869184, 0),
    (8, 512, 0, 9, 384, 1, 0, 0): (2064384, 126, 0, 0, 252, 393216, 3981312, 0),
    (8, 128, 0, 9, 512, 1, 0, 0): (0, 168, 1332480, 0, 336, 131072, 0, 0),
    (8, 512, 256, 9, 512, 3, 1, 0): (2752512, 168, 4084992, 6837504, 336, 7077888, 29196288, 0),
    (8, 512, 256, 9, 512, 1, 0, 0): (2752512, 168, 4084992, 0, 336, 786432, 7962624, 0),
    # ... B = 25
    (25, 1, 0, 72, 64, 7, 3, 0): (0, 4050, 0, 0, 8100, 200704, 0, 0),
    (25, 64, 0, 72, 64, 3, 1, 0): (0, 4050, 34214400, 34214400, 8100, 73728, 0, 33307392),
    (25, 64, 0, 72, 384, 1, 0, 0): (0, 24300, 0, 0, 48600, 49152, 0, 0),
    (25, 128, 0, 72, 64, 1, 0, 0): (0, 4050, 34214400, 0, 8100, 16384, 0, 0),
    (25, 256, 0, 36, 64, 1, 0, 2): (0, 1013, 8553728, 0, 2026, 32768, 16588800, 0),
    (25, 64, 64, 72, 64, 3, 1, 0): (0, 4050, 34214400, 34214400, 8100, 147456, 0, 33307392),
    (25, 64, 64, 72, 64, 1, 0, 0): (0, 4050, 34214400, 0, 8100, 16384, 0, 0),
    (25, 128, 0, 72, 64, 3, 1, 1): (0, 4050, 34214400, 0, 8100, 147456, 0, 33307392),
    (25, 64, 0, 72, 1, 1, 0, 0): (0, 4050, 0, 0, 8100, 128, 0, 0),
    (25, 64, 0, 36, 64, 3, 1, 0): (0, 1013, 8553728, 8553728, 2026, 73728, 24883200, 8326912),
    (25, 64, 0, 36, 384, 1, 0, 0): (0, 6078, 0, 0, 12156, 49152, 0, 0),
    (25, 256, 0, 18, 128, 1, 0, 2): (0, 508, 4212224, 0, 1016, 65536, 8294400, 0),
    (25, 128, 64, 36, 128, 3, 1, 0): (0, 2026, 16848128, 16848128, 4052, 442368, 49766400, 16621312),
    (25, 128, 64, 36, 128, 1, 0, 0): (0, 2026, 16848128, 0, 4052, 49152, 0, 0),
    (25, 256, 0, 36, 128, 3, 1, 1): (0, 2026, 16848128, 0, 4052, 589824, 49766400, 16621312),
    (25, 128, 0, 18, 128, 3, 1, 0): (0, 508, 4212224, 4212224, 1016, 294912, 33177600, 4155392),
    (25, 128, 0, 18, 384, 1, 0, 0): (0, 1524, 0, 0, 3048, 98304, 0, 0),
    (25, 512, 0, 9, 256, 1, 0, 2): (0, 256, 2089984, 0, 512, 262144, 8294400, 0),
    (25, 256, 128, 18, 256, 3, 1, 0): (0, 1016, 8359424, 8359424, 2032, 1769472, 33177600, 8302592),
    (25, 256, 128, 18, 256, 1, 0, 0): (0, 1016, 8359424, 0, 2032, 196608, 24883200, 0),
    (25, 512, 0, 18, 256, 3, 1, 1): (0, 1016, 8359424, 0, 2032, 2359296, 33177600, 8302592),
    (25, 256, 0, 9, 256, 3, 1, 0): (0, 256, 2089984, 2089984, 512, 1179648, 31104000, 0),
    (25, 256, 0, 9, 384, 1, 0, 0): (0, 384, 0, 0, 768, 196608, 6220800, 0),
    (25, 256, 0, 9, 512, 3, 1, 0): (0, 512, 4163584, 4163584, 1024, 2359296, 33177600, 0),
    (25, 512, 0, 9, 512, 3, 1, 0): (0, 512, 4163584, 4163584, 1024, 4718592, 33177600, 0),
    (25, 512, 0, 9, 384, 1, 0, 0): (0, 384, 0, 0, 768, 393216, 12441600, 0),
    (25, 128, 0, 9, 512, 1, 0, 0): (0, 512, 4163584, 0, 1024, 131072, 0, 0),
    (25, 512, 256, 9, 512, 3, 1, 0): (0, 512, 4163584, 4163584, 1024, 7077888, 33177600, 0),
    (25, 512, 256, 9, 512, 1, 0, 0): (0, 512, 4163584, 0, 1024, 786432, 24883200, 0),
    # an upsample conv at another shape; shapes outside the channel-chunk form (k_conv_ig): 48 -> 40, 5x5
    (2, 256, 0, 18, 256, 3, 1, 1): (2064384, 84, 2733312, 0, 168, 1179648, 11943936, 0),
    (1, 48, 0, 9, 40, 3, 1, 0): (49152, 3, 0, 0, 6, 46080, 51840, 0),
    (2, 3, 0, 17, 5, 5, 2, 0): (0, 19, 0, 0, 38, 8000, 57800, 0),
    # 63 | 64 tiles of the halo-staged kernel (CONV3_MIN_TILES), 191 | 192 (CONV3F_MIN_TILES)
    (63, 64, 0, 16, 64, 3, 1, 0): (0, 504, 4257792, 4257792, 1008, 73728, 16515072, 0),
    (64, 64, 0, 16, 64, 3, 1, 0): (0, 512, 4325376, 4325376, 1024, 73728, 16777216, 4210688),
    (191, 64, 0, 16, 64, 3, 1, 0): (0, 1528, 12908544, 12908544, 3056, 73728, 25034752, 12566272),
    (192, 64, 0, 16, 64, 3, 1, 0): (0, 1536, 12976128, 12976128, 3072, 73728, 25165824, 12632064),
    # 162 tiles with 11 | 12 K stages (CC_SPLIT2_STAGES): 3x3 stages of 8 channels, 1x1 stages of 64
    (1, 88, 0, 72, 64, 3, 1, 0): (0, 162, 1368576, 0, 324, 110592, 7962624, 0),
    (1, 96, 0, 72, 64, 3, 1, 0): (2654208, 162, 4022784, 0, 324, 110592, 7962624, 0),
    (1, 704, 0, 72, 64, 1, 0, 0): (0, 162, 1368576, 0, 324, 90112, 6635520, 0),
    (1, 768, 0, 72, 64, 1, 0, 0): (2654208, 162, 4022784, 0, 324, 98304, 7962624, 0),
}

# (option, value) of rdq_unet_set_option -> the OPTION_ROWS whose sizes differ from SIZES under it
OPTION_ROWS = [(1, 88, 0, 72, 64, 3, 1, 0), (1, 96, 0, 72, 64, 3, 1, 0), (1, 768, 0, 72, 64, 1, 0, 0),
               (1, 512, 256, 9, 512, 3, 1, 0), (64, 64, 0, 16, 64, 3, 1, 0), (192, 64, 0, 16, 64, 3, 1, 0)]
OPTION_SIZES = {
    (7, 11): {   # CC_SPLIT2_STAGES
        (1, 88, 0, 72, 64, 3, 1, 0): (2654208, 162, 4022784, 0, 324, 110592, 7962624, 0),
    },
    (7, 13): {   # CC_SPLIT2_STAGES
        (1, 96, 0, 72, 64, 3, 1, 0): (0, 162, 1368576, 0, 324, 110592, 7962624, 0),
        (1, 768, 0, 72, 64, 1, 0, 0): (0, 162, 1368576, 0, 324, 98304, 7962624, 0),
    },
    (6, 5): {   # CC_MIN_STAGES
        (1, 512, 256, 9, 512, 3, 1, 0): (1966080, 24, 2132736, 2525952, 48, 7077888, 8957952, 0),
    },
    (2, 65): {   # CONV3_MIN_TILES
        (64, 64, 0, 16, 64, 3, 1, 0): (0, 512, 4325376, 4325376, 1024, 73728, 16777216, 0),
    },
    (4, 0): {},   # CONV3F_MIN_TILES: chooses a kernel, no size
    (1, 1): {},   # BF16_PER_TAP: the same
    (3, 0): {},   # BF16_RAW: the same
}

# rdq_group_norm_ws_bytes(B, C, HW, G)
GN_WS = {
    (1, 64, 5184, 8): 1472, (1, 128, 1296, 8): 832, (1, 256, 324, 8): 448, (1, 512, 81, 8): 320,
    (8, 64, 5184, 8): 11776, (8, 128, 1296, 8): 6656, (8, 256, 324, 8): 3584, (8, 512, 81, 8): 2560,
    (25, 64, 5184, 8): 36800, (25, 128, 1296, 8): 20800, (25, 256, 324, 8): 11200, (25, 512, 81, 8): 8000,
    (2, 64, 5184, 8): 2944,
}
# rdq_linear_attention_ws_bytes(B, heads, dh, n, nmem)
LA_WS = {
    (1, 4, 32, 5184, 4): 381952, (1, 4, 32, 1296, 4): 120832, (1, 4, 32, 324, 4): 51200, (1, 4, 32, 81, 4): 33792,
    (8, 4, 32, 5184, 4): 3055616, (8, 4, 32, 1296, 4): 966656, (8, 4, 32, 324, 4): 409600,
    (8, 4, 32, 81, 4): 270336, (25, 4, 32, 5184, 4): 9548800, (25, 4, 32, 1296, 4): 3020800,
    (25, 4, 32, 324, 4): 1280000, (25, 4, 32, 81, 4): 844800, (2, 4, 32, 5184, 4): 763904,
}
# (B, dim, n) -> (rdq_linear_attention_bf16_ws_bytes, rdq_linear_attention_f32_ws_bytes)
LAB_WS = {
    (1, 64, 5184): (713728, 1410048), (1, 64, 1296): (191488, 365568), (1, 128, 324): (52224, 104448),
    (1, 128, 5184): (713728, 1410048), (8, 64, 5184): (5709824, 11280384), (8, 64, 1296): (1531904, 2924544),
    (8, 128, 324): (417792, 835584), (8, 128, 5184): (5709824, 11280384), (25, 64, 5184): (17843200, 17843200),
    (25, 64, 1296): (4787200, 9139200), (25, 128, 324): (1305600, 2611200), (25, 128, 5184): (17843200, 17843200),
    (3, 64, 5184): (2141184, 4230144), (344, 64, 5184): (35930112, 35930112),
}


def _desc(t):
    B, cin1, cin2, H, cout, k, pad, mode = t
    return _hip.ConvDesc(B, cin1, cin2, H, H, cout, k, k, pad, mode)


def _sizes(lib, t, G=8):
    p = ctypes.byref(_desc(t))
    cout = t[4]
    return (lib.rdq_conv2d_ws_bytes(p), lib.rdq_conv2d_tickets(p), lib.rdq_conv2d_gn_ws_bytes(p, G),
            lib.rdq_conv2d_gn_sc_ws_bytes(p, G, cout), lib.rdq_conv2d_gn_sc_tickets(p, cout),
            lib.rdq_conv2d_bf16_wpack_bytes(p), lib.rdq_conv2d_bf16_ws_bytes(p),
            lib.rdq_conv2d_bf16_gn_ws_bytes(p, G))


@pytest.mark.parametrize("t", list(SIZES), ids=lambda t: "-".join(map(str, t)))
def test_conv_size_functions(t):
    """Every conv size function on one descriptor, options at default: the exact values of the library
    before the host paths were consolidated.  Host-only: no GPU call."""
    assert _sizes(_hip.load_library(), t) == SIZES[t]


@pytest.mark.parametrize("option,value", list(OPTION_SIZES), ids=lambda v: str(v))
def test_conv_size_functions_follow_the_options(option, value):
    """One option changed through rdq_unet_set_option: the sizes that depend on it move, the others do not,
    and the default values are back once it is restored."""
    lib = _hip.load_library()
    old = lib.rdq_unet_set_option(option, value)
    try:
        assert old >= 0
        for t in OPTION_ROWS:
            assert _sizes(lib, t) == OPTION_SIZES[(option, value)].get(t, SIZES[t]), t
    finally:
        assert lib.rdq_unet_set_option(option, old) == value
    for t in OPTION_ROWS:
        assert _sizes(lib, t) == SIZES[t], t


def test_size_functions_of_bad_descriptors_are_zero():
    lib = _hip.load_library()
    assert _sizes(lib, (0, 64, 0, 72, 64, 3, 1, 0)) == (0,) * 8
    assert _sizes(lib, (1, 64, 0, 72, 0, 3, 1, 0)) == (0,) * 8
    assert lib.rdq_conv2d_ws_bytes(None) == 0 and lib.rdq_conv2d_tickets(None) == 0
    assert lib.rdq_conv2d_gn_ws_bytes(None, 8) == 0 and lib.rdq_conv2d_gn_sc_ws_bytes(None, 8, 64) == 0
    assert lib.rdq_conv2d_bf16_wpack_bytes(None) == 0 and lib.rdq_conv2d_bf16_ws_bytes(None) == 0
    assert lib.rdq_conv2d_bf16_gn_ws_bytes(None, 8) == 0
    d = ctypes.byref(_desc((1, 64, 0, 72, 64, 3, 1, 0)))
    assert lib.rdq_conv2d_gn_ws_bytes(d, 7) == 0            # G does not divide cout
    assert lib.rdq_conv2d_gn_ws_bytes(d, 16) == 0           # 4 channels per group
    assert lib.rdq_conv2d_gn_sc_ws_bytes(d, 8, 0) == 0
    assert lib.rdq_conv2d_gn_sc_ws_bytes(d, 8, 48) == 1368576      # the 1x1 shortcut only needs cin % 64
    d = ctypes.byref(_desc((1, 64, 0, 5, 64, 3, 1, 0)))     # 25 pixels < one 32-pixel tile
    assert lib.rdq_conv2d_gn_ws_bytes(d, 8) == 0
    d = ctypes.byref(_desc((25, 64, 0, 15, 64, 3, 1, 0)))   # 225 pixels < one 256-pixel tile
    assert lib.rdq_conv2d_bf16_gn_ws_bytes(d, 8) == 0


def test_norm_and_attention_size_functions():
    lib = _hip.load_library()
    for args, want in GN_WS.items():
        assert lib.rdq_group_norm_ws_bytes(*args) == want, args
    for args, want in LA_WS.items():
        assert lib.rdq_linear_attention_ws_bytes(*args) == want, args
    for args, (bf16, f32) in LAB_WS.items():
        assert lib.rdq_linear_attention_bf16_ws_bytes(*args) == bf16, args
        assert lib.rdq_linear_attention_f32_ws_bytes(*args) == f32, args
    assert lib.rdq_group_norm_ws_bytes(0, 64, 5184, 8) == 0 and lib.rdq_group_norm_ws_bytes(1, 64, 5184, 0) == 0
    assert lib.rdq_linear_attention_ws_bytes(1, 4, 32, 0, 4) == 0
    assert lib.rdq_linear_attention_ws_bytes(1, 4, 32, 81, -1) == 0
    for dim in (32, 96, 256):
        assert lib.rdq_linear_attention_bf16_ws_bytes(1, dim, 5184) == 0
        assert lib.rdq_linear_attention_f32_ws_bytes(1, dim, 5184) == 0


# ---------------------------------------------------------------------------------------- rejections
# Every call below has exactly one thing wrong and must return RDQ_E_INVALID before anything is launched.
# The pointers are dummy non-null values that are never dereferenced.  NEVER add a call that would be
# accepted: an accepted call launches a kernel.
P = ctypes.c_void_p(16)
Q = ctypes.c_void_p(4096)
NULL = None
INVALID = -10001

CAT = (1, 128, 64, 36, 128, 3, 1, 0)       # an up-path block1: 3x3 on a concat, splits K
C72 = (1, 64, 0, 72, 64, 3, 1, 0)
QKV = (1, 128, 0, 18, 384, 1, 0, 0)
STEM = (1, 1, 0, 72, 64, 7, 3, 0)
B25 = (25, 64, 0, 72, 64, 3, 1, 0)         # on the bf16 halo-staged kernel
WIDE = (1, 64, 0, 72, 1024, 3, 1, 0)       # G = 128 divides it into groups of 8 channels
WIDE25 = (25, 64, 0, 72, 1024, 3, 1, 0)

_ptrs3 = (ctypes.c_void_p * 3)
_LW = _ptrs3(16, 16, 16)
_LY = _ptrs3(16, 16, 16)
_LW_HOLE = _ptrs3(16, 0, 16)
_LOUT = (ctypes.c_int32 * 3)(128, 256, 512)          # lout[0] = 2 cout of C72
_LOUT_ZERO = (ctypes.c_int32 * 3)(128, 0, 512)


def _gn_ws(a):
    return _hip.load_library().rdq_conv2d_gn_ws_bytes(ctypes.byref(a["d"]), a["G"])


def _sc_ws(a):
    return _hip.load_library().rdq_conv2d_gn_sc_ws_bytes(ctypes.byref(a["d"]), a["G"], a["cout_s"])


def _bf16_gn_ws(a):
    return _hip.load_library().rdq_conv2d_bf16_gn_ws_bytes(ctypes.byref(a["d"]), a["G"])


def _conv_ws(a):
    return _hip.load_library().rdq_conv2d_ws_bytes(ctypes.byref(a["d"]))


def _lab_ws(fn):
    return lambda a: getattr(_hip.load_library(), fn)(a["B"], a["dim"], a["n"])


# entry point -> its arguments in order, each with a valid value; "d" is a descriptor tuple, a callable is
# evaluated on the final arguments (the workspace size of the call's own descriptor)
_GN = dict(x=P, x2=P, w=P, bias=P, G=8, eps=1e-5, gamma=P, beta=P)
_LSM = dict(cin=256, temb=P, n=3, lw=_LW, lb=NULL, lout=_LOUT, ly=_LY, ss_index=0)
_TM = dict(t=P, w1=P, b1=P, hid=256, w2=P, b2=P, out=256)
_LAB = dict(B=3, dim=64, n=5184, nmem=4, scale=0.25, x=P, g_in=P, wqkv=P, mem_kv=P, wout=P, b_out=P, g_out=P, y=Q, ws=P)
VALID = {
    "rdq_conv2d": dict(d=CAT, x=P, x2=P, w=P, bias=P, residual=P, y=P, ws=P, ws_bytes=_conv_ws, tickets=P, st=NULL),
    "rdq_conv2d_rms": dict(d=QKV, x=P, g=P, w=P, bias=P, residual=P, y=P, ws=P, ws_bytes=_conv_ws, tickets=P, st=NULL),
    "rdq_conv2d_gn_silu": dict(d=CAT, **_GN, scale_shift=P, post_residual=P, y=P, ws=P, ws_bytes=_gn_ws, tickets=P,
                               st=NULL),
    "rdq_conv2d_gn_silu_sc": dict(d=CAT, **_GN, scale_shift=P, y=P, cout_s=128, w_s=P, b_s=P, y_s=P, ws=P,
                                  ws_bytes=_sc_ws, tickets=P, st=NULL),
    "rdq_conv2d_gn_silu_lsm": dict(d=C72, **_GN, post_residual=P, y=P, ws=P, ws_bytes=_gn_ws, tickets=P, **_LSM,
                                   st=NULL),
    "rdq_conv2d_gn_silu_out": dict(d=C72, **_GN, scale_shift=P, post_residual=P, nf=1, wf=P, bf=P, yf=P, ws=P,
                                   ws_bytes=_gn_ws, tickets=P, st=NULL),
    "rdq_unet_head": dict(d=STEM, x=P, w=P, bias=P, y=P, dim=64, theta=10000.0, **_TM, temb=P, st=NULL),
    "rdq_conv2d_stem": dict(d=STEM, x=P, w=P, bias=P, y=P, st=NULL),
    "rdq_conv2d_bf16_pack": dict(d=CAT, w=P, wp=P, st=NULL),
    "rdq_conv2d_bf16": dict(d=CAT, x=P, x2=P, wp=P, bias=P, residual=P, y=P, ws=P,
                            ws_bytes=lambda a: _hip.load_library().rdq_conv2d_bf16_ws_bytes(ctypes.byref(a["d"])),
                            st=NULL),
    "rdq_conv2d_bf16_gn_silu": dict(d=B25, x=P, x2=P, wp=P, bias=P, G=8, eps=1e-5, gamma=P, beta=P, scale_shift=P,
                                    post_residual=P, y=P, ws=P, ws_bytes=_bf16_gn_ws, st=NULL),
    "rdq_conv2d_bf16_gn_silu8": dict(d=B25, x=P, x2=P, wp=P, bias=P, G=8, eps=1e-5, gamma=P, beta=P, scale_shift=P,
                                     y8=P, ws=P, ws_bytes=_bf16_gn_ws, st=NULL),
    "rdq_conv2d_bf16_gn_silu_x8": dict(d=B25, x8=P, wp=P, bias=P, G=8, eps=1e-5, gamma=P, beta=P, scale_shift=P,
                                       post_residual=P, y=P, ws=P, ws_bytes=_bf16_gn_ws, st=NULL),
    "rdq_conv2d_bf16_gn_silu_out": dict(d=B25, x=P, x2=P, wp=P, bias=P, G=8, eps=1e-5, gamma=P, beta=P,
                                        scale_shift=P, post_residual=P, nf=1, wf=P, bf=P, yf=P, ws=P,
                                        ws_bytes=_bf16_gn_ws, st=NULL),
    "rdq_group_norm_silu": dict(B=2, C=64, HW=5184, G=8, eps=1e-5, x=P, gamma=P, beta=P, ss=P, y=P, ws=P, st=NULL),
    "rdq_rmsnorm": dict(B=2, C=64, HW=5184, x=P, g=P, res=P, y=P, st=NULL),
    "rdq_linear": dict(B=2, cin=64, out=256, x=P, w=P, bias=P, act_in=1, act_out=0, y=P, st=NULL),
    "rdq_sinusoidal_emb": dict(B=2, dim=64, theta=10000.0, t=P, y=P, st=NULL),
    "rdq_time_mlp": dict(B=2, dim=64, theta=10000.0, **_TM, y=P, st=NULL),
    "rdq_linear_silu_multi": dict(B=2, cin=256, x=P, n=3, w=_LW, b=NULL, out=_LOUT, y=_LY, st=NULL),
    "rdq_linear_attention": dict(B=2, heads=4, dh=32, n=5184, nmem=4, scale=0.25, qkv=P, mem_kv=P, out=P, ws=P,
                                 st=NULL),
    "rdq_linear_attention_block": dict(B=2, heads=4, dh=32, n=5184, nmem=4, scale=0.25, qkv=P, mem_kv=P, dim=64,
                                       w_out=P, b_out=P, g_out=P, res=P, y=P, ws=P, st=NULL),
    "rdq_linear_attention_bf16": dict(**_LAB, ws_bytes=_lab_ws("rdq_linear_attention_bf16_ws_bytes"), st=NULL),
    "rdq_linear_attention_f32": dict(**_LAB, ws_bytes=_lab_ws("rdq_linear_attention_f32_ws_bytes"), st=NULL),
    "rdq_full_attention": dict(B=2, heads=4, dh=32, n=81, nmem=4, qkv=P, mem_kv=P, out=P, st=NULL),
    "rdq_red_q_sample": dict(B=2, n=5184, sa=P, s1a=P, t=P, x0=P, eps=P, xt=P, st=NULL),
    "rdq_red_q_sample_t": dict(B=2, n=5184, sa=P, s1a=P, t=P, x0=P, eps=P, xt=P, t_out=P, st=NULL),
    "rdq_red_epilogue": dict(B=2, n=5184, sr=P, srm1=P, t=P, xt=P, eh=P, eps=P, g=P, st=NULL),
}


def _short(a):
    """ws_bytes one byte short of what the call's own size function asks for"""
    return VALID[a["_fn"]]["ws_bytes"](a) - 1


def _nulls(fn, *names):
    return [(fn, f"{n}=null", {n: NULL}) for n in names]


_FUSED_CC = ("rdq_conv2d_gn_silu", "rdq_conv2d_gn_silu_sc", "rdq_conv2d_gn_silu_lsm", "rdq_conv2d_gn_silu_out")
_FUSED_BF = ("rdq_conv2d_bf16_gn_silu", "rdq_conv2d_bf16_gn_silu8", "rdq_conv2d_bf16_gn_silu_out")
_FUSED_LAB = ("rdq_linear_attention_bf16", "rdq_linear_attention_f32")

REJECTED = []
# the descriptor and input checks that every conv entry point with the three input modes shares
for fn in ("rdq_conv2d", "rdq_conv2d_gn_silu", "rdq_conv2d_bf16", "rdq_conv2d_bf16_gn_silu", "rdq_conv2d_bf16_gn_silu8",
           "rdq_conv2d_bf16_gn_silu_out"):
    big = fn.startswith("rdq_conv2d_bf16_gn")       # these need the halo-staged kernel's >= 64 tiles
    B = 25 if big else 1
    REJECTED += [
        (fn, "concat-without-x2", {"d": (B, 128, 64, 36, 128, 3, 1, 0), "x2": NULL}),
        (fn, "upsample-odd-H", {"d": (B, 128, 0, 35, 128, 3, 1, 1)}),
        (fn, "upsample-with-cin2", {"d": (B, 128, 64, 36, 128, 3, 1, 1)}),
        (fn, "unshuffle-with-cin2", {"d": (B, 256, 64, 18, 128, 1, 0, 2)}),
        (fn, "unshuffle-cin1-not-x4", {"d": (B, 130, 0, 18, 128, 1, 0, 2)}),
        (fn, "B=0", {"d": (0, 128, 64, 36, 128, 3, 1, 0)}),
    ]
    if fn != "rdq_conv2d_bf16_gn_silu8":            # it reads d->cout before anything checks d
        REJECTED += [(fn, "d=null", {"d": None})]
for fn in _FUSED_CC[1:]:
    REJECTED += [(fn, "concat-without-x2", {"d": (1, 128, 64, 36, 128, 3, 1, 0), "x2": NULL,
                                            **({"lout": (ctypes.c_int32 * 3)(256, 256, 512)} if "lsm" in fn else {})})]
for fn in _FUSED_CC + _FUSED_BF + ("rdq_conv2d_bf16_gn_silu_x8",) + _FUSED_LAB:
    REJECTED += [(fn, "ws-one-byte-short", {"ws_bytes": _short}), (fn, "ws=null", {"ws": NULL}),
                 (fn, "ws_bytes=0", {"ws_bytes": 0})]
for fn in _FUSED_CC + _FUSED_BF + ("rdq_conv2d_bf16_gn_silu_x8",):
    REJECTED += [(fn, "G-does-not-divide-cout", {"G": 7}), (fn, "G=0", {"G": 0}),
                 (fn, "4-channels-per-group", {"G": VALID[fn]["d"][4] // 4}),
                 (fn, "7x7", {"d": (25, 64, 0, 72, 64, 7, 3, 0)})]
    REJECTED += _nulls(fn, "gamma", "beta")
REJECTED += _nulls("rdq_conv2d", "x", "w", "y")
REJECTED += [("rdq_conv2d", "pad<0", {"d": (1, 128, 64, 36, 128, 3, -1, 0)}),
             ("rdq_conv2d", "cout=0", {"d": (1, 128, 64, 36, 0, 3, 1, 0)})]
REJECTED += _nulls("rdq_conv2d_rms", "d", "x", "g", "w", "y")
REJECTED += [
    ("rdq_conv2d_rms", "3x3", {"d": (1, 128, 0, 18, 384, 3, 1, 0)}),
    ("rdq_conv2d_rms", "cin1>2048", {"d": (1, 2112, 0, 18, 384, 1, 0, 0)}),
    ("rdq_conv2d_rms", "unshuffle", {"d": (1, 128, 0, 18, 384, 1, 0, 2)}),
    ("rdq_conv2d_rms", "cin2", {"d": (1, 128, 64, 18, 384, 1, 0, 0)}),
    ("rdq_conv2d_rms", "cin1-not-x64", {"d": (1, 96, 0, 18, 384, 1, 0, 0)}),
]
REJECTED += _nulls("rdq_conv2d_gn_silu", "x", "w", "y")
REJECTED += [("rdq_conv2d_gn_silu", "not-chunk-form", {"d": (1, 48, 0, 9, 40, 3, 1, 0), "ws_bytes": 1 << 30})]
REJECTED += _nulls("rdq_conv2d_gn_silu_sc", "d", "x", "w", "y", "w_s", "y_s")
REJECTED += [
    ("rdq_conv2d_gn_silu_sc", "upsample", {"d": (1, 128, 0, 36, 128, 3, 1, 1), "ws_bytes": 1 << 30}),
    ("rdq_conv2d_gn_silu_sc", "1x1", {"d": (1, 128, 64, 36, 128, 1, 0, 0), "ws_bytes": 1 << 30}),
    ("rdq_conv2d_gn_silu_sc", "cout_s=0", {"cout_s": 0, "ws_bytes": 1 << 30}),
    ("rdq_conv2d_gn_silu_sc", "shortcut-not-chunk-form", {"d": (1, 72, 0, 36, 128, 3, 1, 0), "ws_bytes": 1 << 30}),
]
REJECTED += _nulls("rdq_conv2d_gn_silu_lsm", "x", "w", "y", "temb", "lw", "lout", "ly")
REJECTED += [
    ("rdq_conv2d_gn_silu_lsm", "n>32", {"n": 33}),
    ("rdq_conv2d_gn_silu_lsm", "n=0", {"n": 0}),
    ("rdq_conv2d_gn_silu_lsm", "in=0", {"cin": 0}),
    ("rdq_conv2d_gn_silu_lsm", "ss_index=n", {"ss_index": 3}),
    ("rdq_conv2d_gn_silu_lsm", "lout[ss]-not-2cout", {"ss_index": 1}),
    ("rdq_conv2d_gn_silu_lsm", "lw[1]=null", {"lw": _LW_HOLE}),
    ("rdq_conv2d_gn_silu_lsm", "lout[1]=0", {"lout": _LOUT_ZERO}),
    ("rdq_conv2d_gn_silu_lsm", "upsample", {"d": (1, 64, 0, 72, 64, 3, 1, 1)}),
    ("rdq_conv2d_gn_silu_lsm", "unshuffle", {"d": (1, 64, 0, 72, 64, 1, 0, 2)}),
]
REJECTED += _nulls("rdq_conv2d_gn_silu_out", "x", "w", "yf", "wf")
REJECTED += [
    ("rdq_conv2d_gn_silu_out", "nf>4", {"nf": 5}),
    ("rdq_conv2d_gn_silu_out", "nf=0", {"nf": 0}),
    ("rdq_conv2d_gn_silu_out", "cout-not-x4", {"d": (1, 64, 0, 72, 66, 3, 1, 0), "G": 6}),
    ("rdq_conv2d_gn_silu_out", "G>64", {"d": WIDE, "G": 128}),
]
REJECTED += _nulls("rdq_unet_head", "d", "x", "w", "y", "t", "w1", "b1", "w2", "b2", "temb")
REJECTED += [
    ("rdq_unet_head", "chunk-form", {"d": C72}),
    ("rdq_unet_head", "cout>64", {"d": (1, 1, 0, 72, 128, 7, 3, 0)}),
    ("rdq_unet_head", "conv2d-would-split-K", {"d": (1, 60, 0, 9, 64, 3, 1, 0)}),
    ("rdq_unet_head", "cin2", {"d": (1, 1, 1, 72, 64, 7, 3, 0)}),
    ("rdq_unet_head", "upsample", {"d": (1, 1, 0, 72, 64, 7, 3, 1)}),
    ("rdq_unet_head", "5x5", {"d": (1, 1, 0, 72, 64, 5, 2, 0)}),
    ("rdq_unet_head", "pad<0", {"d": (1, 1, 0, 72, 64, 7, -1, 0)}),
    ("rdq_unet_head", "B=0", {"d": (0, 1, 0, 72, 64, 7, 3, 0)}),
    ("rdq_unet_head", "dim-odd", {"dim": 63}),
    ("rdq_unet_head", "dim<4", {"dim": 2}),
    ("rdq_unet_head", "hid=0", {"hid": 0}),
    ("rdq_unet_head", "out=0", {"out": 0}),
    ("rdq_unet_head", "dim+hid-past-the-staging-image", {"hid": 1 << 20}),
]
REJECTED += _nulls("rdq_conv2d_stem", "d", "x", "w", "y")
REJECTED += [
    ("rdq_conv2d_stem", "cin1=2", {"d": (1, 2, 0, 72, 64, 7, 3, 0)}),
    ("rdq_conv2d_stem", "cin2=1", {"d": (1, 1, 1, 72, 64, 7, 3, 0)}),
    ("rdq_conv2d_stem", "5x5", {"d": (1, 1, 0, 72, 64, 5, 3, 0)}),
    ("rdq_conv2d_stem", "kw=5", {"d": _hip.ConvDesc(1, 1, 0, 72, 72, 64, 7, 5, 3, 0)}),
    ("rdq_conv2d_stem", "pad=2", {"d": (1, 1, 0, 72, 64, 7, 2, 0)}),
    ("rdq_conv2d_stem", "cout=32", {"d": (1, 1, 0, 72, 32, 7, 3, 0)}),
    ("rdq_conv2d_stem", "upsample", {"d": (1, 1, 0, 72, 64, 7, 3, 1)}),
    ("rdq_conv2d_stem", "W=63", {"d": _hip.ConvDesc(1, 1, 0, 72, 63, 64, 7, 7, 3, 0)}),
    ("rdq_conv2d_stem", "W=73", {"d": _hip.ConvDesc(1, 1, 0, 72, 73, 64, 7, 7, 3, 0)}),
    ("rdq_conv2d_stem", "B=0", {"d": (0, 1, 0, 72, 64, 7, 3, 0)}),
    ("rdq_conv2d_stem", "output-past-2^31", {"d": (6473, 1, 0, 72, 64, 7, 3, 0)}),
]
REJECTED += _nulls("rdq_conv2d_bf16_pack", "d", "w", "wp")
REJECTED += [("rdq_conv2d_bf16_pack", "B=0", {"d": (0, 128, 64, 36, 128, 3, 1, 0)})]
REJECTED += _nulls("rdq_conv2d_bf16", "x", "wp", "y")
for fn in _FUSED_BF:
    REJECTED += _nulls(fn, "x", "wp")
    REJECTED += [(fn, "below-conv3-min-tiles", {"d": (1, 64, 0, 72, 64, 3, 1, 0), "ws_bytes": 1 << 30}),
                 (fn, "unshuffle", {"d": (25, 64, 0, 72, 64, 3, 1, 2), "ws_bytes": 1 << 30})]
REJECTED += _nulls("rdq_conv2d_bf16_gn_silu", "y")
REJECTED += _nulls("rdq_conv2d_bf16_gn_silu8", "y8")
REJECTED += [("rdq_conv2d_bf16_gn_silu8", "cout-not-x8", {"d": (25, 64, 0, 72, 68, 3, 1, 0), "G": 17, "ws_bytes": 1 << 30})]
REJECTED += _nulls("rdq_conv2d_bf16_gn_silu_x8", "x8", "wp", "y")
REJECTED += [
    ("rdq_conv2d_bf16_gn_silu_x8", "cin1-not-x32", {"d": (25, 72, 0, 72, 64, 3, 1, 0)}),
    ("rdq_conv2d_bf16_gn_silu_x8", "cin2", {"d": (25, 64, 64, 72, 64, 3, 1, 0)}),
    ("rdq_conv2d_bf16_gn_silu_x8", "upsample", {"d": (25, 64, 0, 72, 64, 3, 1, 1)}),
]
REJECTED += _nulls("rdq_conv2d_bf16_gn_silu_out", "yf", "wf")
REJECTED += [
    ("rdq_conv2d_bf16_gn_silu_out", "nf>4", {"nf": 5}),
    ("rdq_conv2d_bf16_gn_silu_out", "nf=0", {"nf": 0}),
    ("rdq_conv2d_bf16_gn_silu_out", "G>64", {"d": WIDE25, "G": 128}),
]
REJECTED += _nulls("rdq_group_norm_silu", "x", "gamma", "beta", "y", "ws")
REJECTED += [("rdq_group_norm_silu", "G-does-not-divide-C", {"G": 7}), ("rdq_group_norm_silu", "B=0", {"B": 0}),
             ("rdq_group_norm_silu", "HW=0", {"HW": 0}), ("rdq_group_norm_silu", "G=0", {"G": 0})]
REJECTED += _nulls("rdq_rmsnorm", "x", "g", "y") + [("rdq_rmsnorm", "C=0", {"C": 0})]
REJECTED += _nulls("rdq_linear", "x", "w", "y") + [("rdq_linear", "out=0", {"out": 0})]
REJECTED += _nulls("rdq_sinusoidal_emb", "t", "y")
REJECTED += [("rdq_sinusoidal_emb", "dim-odd", {"dim": 63}), ("rdq_sinusoidal_emb", "dim<4", {"dim": 2}),
             ("rdq_sinusoidal_emb", "dim>2048", {"dim": 2050})]
REJECTED += _nulls("rdq_time_mlp", "t", "w1", "b1", "w2", "b2", "y")
REJECTED += [("rdq_time_mlp", "past-64KB", {"hid": 2048 - 64 + 1}), ("rdq_time_mlp", "dim-odd", {"dim": 63}),
             ("rdq_time_mlp", "B=0", {"B": 0})]
REJECTED += _nulls("rdq_linear_silu_multi", "x", "w", "out", "y")
REJECTED += [("rdq_linear_silu_multi", "n>32", {"n": 33}), ("rdq_linear_silu_multi", "n=0", {"n": 0}),
             ("rdq_linear_silu_multi", "w[1]=null", {"w": _LW_HOLE}),
             ("rdq_linear_silu_multi", "out[1]=0", {"out": _LOUT_ZERO})]
REJECTED += _nulls("rdq_linear_attention", "qkv", "mem_kv", "out", "ws")
REJECTED += [("rdq_linear_attention", "dh>32", {"dh": 33}), ("rdq_linear_attention", "nmem<0", {"nmem": -1})]
REJECTED += _nulls("rdq_linear_attention_block", "qkv", "mem_kv", "w_out", "g_out", "y", "ws")
REJECTED += [("rdq_linear_attention_block", "heads=3", {"heads": 3}), ("rdq_linear_attention_block", "dh=16", {"dh": 16}),
             ("rdq_linear_attention_block", "dim=96", {"dim": 96}), ("rdq_linear_attention_block", "dim=512", {"dim": 512})]
for fn in _FUSED_LAB:
    REJECTED += _nulls(fn, "x", "g_in", "wqkv", "mem_kv", "wout", "g_out", "y")
    REJECTED += [(fn, "dim=96", {"dim": 96}), (fn, "dim=256", {"dim": 256}), (fn, "dim=32", {"dim": 32}),
                 (fn, "y==x", {"y": P}), (fn, "B=0", {"B": 0}), (fn, "nmem<0", {"nmem": -1}),
                 (fn, "tensor-past-2^31", {"B": 6473, "ws_bytes": 1 << 40})]
REJECTED += _nulls("rdq_full_attention", "qkv", "mem_kv", "out")
REJECTED += [("rdq_full_attention", "past-160KB-of-LDS", {"n": 481}), ("rdq_full_attention", "dh=16", {"dh": 16}),
             ("rdq_full_attention", "heads=0", {"heads": 0})]
REJECTED += _nulls("rdq_red_q_sample", "sa", "s1a", "t", "x0", "eps", "xt") + [("rdq_red_q_sample", "n=0", {"n": 0})]
REJECTED += _nulls("rdq_red_q_sample_t", "sa", "s1a", "t", "x0", "eps", "xt", "t_out")
REJECTED += [("rdq_red_q_sample_t", "B=0", {"B": 0})]
REJECTED += _nulls("rdq_red_epilogue", "sr", "srm1", "t", "xt", "eh", "eps", "g") + [("rdq_red_epilogue", "n=0", {"n": 0})]


def _arguments(fn, changes):
    a = dict(VALID[fn], _fn=fn)
    a.update(changes)
    if isinstance(a.get("d"), tuple):
        a["d"] = _desc(a["d"])
    for k, v in a.items():
        if callable(v):
            a[k] = v(a) if a.get("d", 0) is not None else 1 << 30
    del a["_fn"]
    return [ctypes.byref(v) if isinstance(v, _hip.ConvDesc) else v for v in a.values()]


@pytest.mark.parametrize("fn,what,changes", REJECTED, ids=[f"{fn}-{what}" for fn, what, _ in REJECTED])
def test_entry_point_rejects(fn, what, changes):
    """One invalid argument, everything else valid: RDQ_E_INVALID, before any HIP call."""
    lib = _hip.load_library()
    assert getattr(lib, fn)(*_arguments(fn, changes)) == INVALID


def test_every_unet_entry_point_with_arguments_has_rejections():
    """The table covers every launching entry point of include/red_diffeq_unet.h."""
    header = open(os.path.join(ROOT, "include", "red_diffeq_unet.h")).read()
    launching = set(re.findall(r"^int (rdq_\w+)\(", header, re.M)) - {"rdq_unet_set_option", "rdq_unet_options_generation",
                                                                      "rdq_conv2d_route", "rdq_time_mlp_route",
                                                                      "rdq_linear_silu_multi_route"}   # host queries: no launch
    assert launching == set(VALID) == {fn for fn, _, _ in REJECTED}
    for fn, args in VALID.items():
        assert len(args) == len(_hip.SIGNATURES[fn][1]), fn
    for fn in ("rdq_time_mlp_route", "rdq_linear_silu_multi_route"):
        assert fn in _hip.SIGNATURES and re.search(rf"^int {fn}\(", header, re.M), fn


# RDQ_LINEAR_ROUTE_* (include/red_diffeq_unet.h)
LIN_INVALID, PER_SAMPLE, BATCHED, WDOT = 0, 1, 2, 3
# B -> rdq_time_mlp_route
TIME_MLP_ROUTES = {0: LIN_INVALID, -3: LIN_INVALID, 1: PER_SAMPLE, 2: PER_SAMPLE, 16: PER_SAMPLE, 17: BATCHED,
                   25: BATCHED, 344: BATCHED}
# (B, in) -> rdq_linear_silu_multi_route
LSM_ROUTES = {(0, 256): LIN_INVALID, (2, 0): LIN_INVALID, (1, 256): PER_SAMPLE, (16, 256): PER_SAMPLE,
              (16, 64): PER_SAMPLE, (17, 1): BATCHED, (17, 64): BATCHED, (17, 255): BATCHED, (344, 100): BATCHED,
              (17, 256): WDOT, (65, 256): WDOT, (344, 256): WDOT, (17, 257): PER_SAMPLE, (20, 600): PER_SAMPLE,
              (344, 1024): PER_SAMPLE}


def test_linear_route_queries():
    """The routing of rdq_time_mlp and rdq_linear_silu_multi as the header states it: the batched kernels from 17
    samples, the sample-per-lane kernel at in = 256 only, the per-sample kernel for in > 256 at any B."""
    lib = _hip.load_library()
    header = open(os.path.join(ROOT, "include", "red_diffeq_unet.h")).read()
    for name, v in (("INVALID", LIN_INVALID), ("PER_SAMPLE", PER_SAMPLE), ("BATCHED", BATCHED), ("WDOT", WDOT)):
        assert re.search(rf"RDQ_LINEAR_ROUTE_{name} = {v}\b", header), name
    for B, want in TIME_MLP_ROUTES.items():
        assert lib.rdq_time_mlp_route(B) == want, B
    for (B, cin), want in LSM_ROUTES.items():
        assert lib.rdq_linear_silu_multi_route(B, cin) == want, (B, cin)
