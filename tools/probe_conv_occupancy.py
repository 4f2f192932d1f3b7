"""Resident workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor) and launch geometry of the
stage-2 3x3 fp32 conv at a population launch size, default tile vs two-pass staging (ConvArgs::twopass).

usage: python tools/probe_conv_occupancy.py [groups] [batch]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gentun_amd.ops import cnn_kernels as K

G = int(sys.argv[1]) if len(sys.argv) > 1 else 25
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
torch.zeros(1, device="cuda")                   # the occupancy query needs an initialised device
L = K.lib()
for fwd in (1, 0):
    for two in (0, 1):
        a = K.ConvArgs()
        a.KH, a.KW, a.Cinp, a.Coutp, a.H, a.W = 3, 3, 56, 56, 16, 16
        a.G = a.ngroups = G
        a.B, a.prec, a.cout_real, a.epi_bf16, a.twopass = B, 1, 50, fwd, two
        a.TH = K.conv_tile_rows(16, 16)
        s = K.ConvSel()
        assert L.gt_conv_fast_select(C.byref(a), C.byref(s))
        print(json.dumps({"launch": "fwd" if fwd else "dgrad", "groups": G, "batch": B, "twopass_asked": two,
                          "twopass_kernel": L.gt_conv_fast_twopass(a), "tile_rows": s.TH, "grid": [s.gx, s.gy],
                          "block": s.block, "dynamic_lds": s.lds, "workgroups_per_cu": L.gt_conv_fast_occupancy(a)}))
