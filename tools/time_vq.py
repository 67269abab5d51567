"""VQ search kernels at the benchmark shape: time per call of the three CRK_VQ_LC routes.  (That the routes agree on
every index is tests/test_gpu_ops.py::test_vq_every_search_path_agrees_on_near_ties_and_edges.)
    python tools/time_vq.py"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch
from crank_amd import _lib, ops

g = torch.Generator().manual_seed(0)
x = torch.randn(64, 500, 64, generator=g).cuda()
w = (torch.randn(512, 64, generator=g) * 0.7).cuda()
try:
    for lc in (0, 1, 2):
        _lib.check(_lib.lib().crk_debug_vq_set_lc(lc), "set")
        for _ in range(3):
            ops.vq_apply(x, w)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(50):
            ops.vq_apply(x, w)
        ev[1].record()
        torch.cuda.synchronize()
        print(f"CRK_VQ_LC={lc}: {ev[0].elapsed_time(ev[1]) / 50 * 1e3:.1f} us per call (events, incl. launch)")
finally:
    _lib.lib().crk_debug_vq_set_lc(int(os.environ.get("CRK_VQ_LC", "2")))
