"""Do the forward / data-gradient chain launches of the speaker-adversarial net and the speaker classifier gain anything
when they run side by side?  At the benchmark shape (64 x 500 frames, the recipe's two nets) each pair of launches is
captured twice - one after the other on one stream, and as two parallel branches of the graph - and the replays are timed
with device events:
    python tools/speaker_chains_side_by_side.py [replays]
Prints microseconds per replay of each form (profiles/speaker_chains_side_by_side.txt)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from crank_amd import _lib, ops  # noqa: E402
from crank_amd._lib import ptr, stream_ptr  # noqa: E402
from crank_amd.bin.train import get_model  # noqa: E402
from crank_amd.utils import load_yaml  # noqa: E402

NO_PARAM_GRAD = 2
ops.set_precision("bf16")
replays = int(sys.argv[1]) if len(sys.argv) > 1 else 300
B, T = 64, 500
torch.manual_seed(0)
models = get_model(load_yaml(None, batch_size=B, batch_len=T), 14, "cuda")
L = _lib.lib()
jobs = []
for name in ("SPKRADV", "C"):
    m = models[name]
    (net, base), = m._nets
    assert L.crk_net_reserve(net.handle, B, T) == 0
    x = torch.randn(B * T, net.in_ch, device="cuda")
    dy = torch.randn(B * T, net.out_ch, device="cuda")
    y = torch.empty(B * T, net.out_ch, device="cuda")
    saved = torch.empty(L.crk_net_saved_bytes(net.handle, B, T) // 4 + 1, device="cuda")
    jobs.append(dict(name=name, net=net, params=m.flat.data_ptr() + 4 * base, x=x, dy=dy, y=y, saved=saved))


def fwd(j):
    n = j["net"]
    assert L.crk_net_forward(n.handle, j["params"], 1, ptr(j["x"]), n.in_ch, None, 0, ptr(j["y"]), n.out_ch, ptr(j["saved"]), B, T, 0, 0,
                             stream_ptr()) == 0


def bwd(j):  # the chain alone, stopped at the first conv's output gradient as in the nets' own updates (no dx, no weight gradient)
    n = j["net"]
    assert L.crk_net_backward(n.handle, j["params"], 1, None, ptr(j["x"]), n.in_ch, None, 0, ptr(j["dy"]), n.out_ch, None, 0, 1.0, None,
                              0, ptr(j["saved"]), B, T, NO_PARAM_GRAD, 0, stream_ptr()) == 0


def capture(fn, side):
    g = torch.cuda.CUDAGraph()
    s2 = torch.cuda.Stream()
    with torch.cuda.graph(g):
        if side:
            cur = torch.cuda.current_stream()
            s2.wait_stream(cur)
            fn(jobs[0])
            with torch.cuda.stream(s2):
                fn(jobs[1])
            cur.wait_stream(s2)
        else:
            fn(jobs[0])
            fn(jobs[1])
    return g


def timed(g):
    for _ in range(20):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / replays


for j in jobs:  # weights prepared and planes written outside the captures
    fwd(j)
    bwd(j)
torch.cuda.synchronize()
for what, fn in (("forward chains", fwd), ("data-gradient chains", bwd)):
    graphs = {"one stream": capture(fn, False), "two branches": capture(fn, True)}
    for rep in range(3):  # alternating
        print(what, " ".join(f"| {k}: {timed(g):7.2f} us" for k, g in graphs.items()), flush=True)
print("(a replay of an empty graph costs its launch: the difference between the two forms is what counts)")
