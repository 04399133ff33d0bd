"""Kernel experiment (timing build only): where an item of the Winograd kernel's persistent walk spends its life.

    python -m hvpr_amd.build --timing
    HVPR_AMD_LIB=hvpr_amd/libhvpr_amd_timing.so python tools/wino_item_timeline.py [--shared]

Per backbone level: cycle stamps of the first three items of a few workgroups (the second and third are reported where a
workgroup walks that many, else the first; item entry, exit of the first chunk's barrier,
end of the K loop, end of the item), stand-alone or (--shared) with a second stream that keeps another level-0 layer in flight (on
the direct kernel, which does not write these stamps).
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hvpr_amd import _lib, kernels

L = ctypes.CDLL(_lib.LIB_PATH)
L.hvpr_exp_wino_dbg.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
dev = "cuda:0"
shared = "--shared" in sys.argv
use_table = "--no-table" not in sys.argv
side = torch.cuda.Stream()
for (H, W, C) in [(248, 296, 128), (124, 148, 256), (62, 74, 512)]:
    x = torch.randn(1, H, W, C, device=dev)
    pc = kernels.pack_conv_wino(torch.randn(C, C, 3, 3, device=dev) / (3 * C ** 0.5), torch.ones(C, device=dev), torch.zeros(C, device=dev))
    x0 = torch.randn(1, 248, 296, 128, device=dev)
    pc0 = kernels.pack_conv(torch.randn(128, 128, 3, 3, device=dev) / 34.0, torch.ones(128, device=dev), torch.zeros(128, device=dev), tile_cfg=1)
    rows = []
    for rep in range(6):
        L.hvpr_exp_wino_dbg(None, 0, 1)
        if shared:
            with torch.cuda.stream(side):
                for _ in range(3):
                    kernels.conv2d_nhwc(x0, pc0, use_table=use_table)
        kernels.conv2d_wino_nhwc(x, pc, use_table=use_table)
        torch.cuda.synchronize()
        buf = np.zeros(8 * 3 * 4, np.int64)
        L.hvpr_exp_wino_dbg(buf.ctypes.data, buf.size, 0)
        if rep:                                  # the first launch warms caches and clocks
            rows.append(buf.reshape(8, 3, 4))
    r = np.stack(rows)                           # [launch][slot][item][4]
    later = r[:, :, 1:].reshape(-1, 4)
    later = later[later[:, 0] != 0]
    which = "second and third" if len(later) else "first"
    s = later if len(later) else r[:, :, 0].reshape(-1, 4)
    s = s[s[:, 0] != 0]
    if not len(s):
        print(json.dumps({"level": f"{H}x{W}x{C}", "items": 0}))
        continue
    pro, k, epi = s[:, 1] - s[:, 0], s[:, 2] - s[:, 1], s[:, 3] - s[:, 2]
    life = s[:, 3] - s[:, 0]
    print(json.dumps({"level": f"{H}x{W}x{C}", "shared": shared, "table": use_table, "items": int(len(s)), "which": which,
                      "median_cycles": {"entry_to_first_barrier": float(np.median(pro)), "k_loop": float(np.median(k)),
                                        "epilogue": float(np.median(epi)), "item": float(np.median(life))},
                      "share_outside_k_loop": round(float(np.median((pro + epi) / life)), 4)}), flush=True)
