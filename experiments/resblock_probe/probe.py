"""Times qpg_resblock_f32 alone at B = 256, T = 60 (240 workgroups: one per CU) and T = 120 (480): the product row of
README.md's table.  (The rows with parts of the stage compiled out needed the -DQPG_RES_PROBE hooks: see README.md.)
    python experiments/resblock_probe/probe.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import qpgesture_amd._lib as L  # noqa: E402
import torch  # noqa: E402

dev = torch.device("cuda:0")
pack = torch.randn((128 * 8192,), device=dev) * 0.03
b1 = torch.randn((512,), device=dev) * 0.05
b2 = torch.randn((512,), device=dev) * 0.05
for T in (60, 120):
    x = torch.randn((256, T, 512), device=dev)
    y = torch.empty_like(x)
    for _ in range(3):
        L.call("qpg_resblock_f32", dev, x, 256, T, 3, pack, b1, b2, y, None)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    for e0, e1 in ev:
        e0.record()
        L.call("qpg_resblock_f32", dev, x, 256, T, 3, pack, b1, b2, y, None)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    med = ms[len(ms) // 2]
    print("T=%3d: median %.1f us  min %.1f us  (%.1f TFLOP/s-equivalent)"
          % (T, med * 1e3, ms[0] * 1e3, 2.0 * 256 * T * 512 * 2048 / med / 1e9))
