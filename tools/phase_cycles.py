"""Per-wave phase cycles of one stack kernel from an instrumented build (the shared timer of csrc/stack_common.h):
    python tools/phase_cycles.py <kernel> build             cross-compiles crank_amd/libcrank_hip_prof_<kernel>.so
    python tools/phase_cycles.py <kernel> [--rev TEXT]      the tables at the benchmark shape (B = 64, T = 500)
    python tools/phase_cycles.py <kernel> --check           B = 2, T = 150, smallest net: asserts what the timer wrote
<kernel> is a key of KERNELS.  `build` needs the product objects (make -C crank_amd/csrc) and goes through
tools/build_variant.sh, which reads the source list from the Makefile."""
import ctypes
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# the timer's one buffer shape (stack_common.h: SK_PROF_WGS, SK_PROF_WAVES, SK_PROF_SLOTS)
WGS, WAVES, SLOTS = 1024, 8, 16

# (tag, in, out, k, layers, stacks, aux) of the generator's gated stacks, smallest last; the plain nets of the model, smallest last
GATED = (("enc0", 80, 64, 5, 8, 4, 0), ("dec0", 128, 80, 5, 8, 4, 34), ("enc1", 64, 64, 3, 6, 3, 0))
PLAIN = ("C", "SPKRADV")

# src / flag: the one source built with the timer on (a source holds one timed kernel) and the flag that turns it on.  slots: the names of the
# kernel's slots in its own numbering (the comment above the kernel), total: the slot of the wave's whole life.  waves: how many
# waves of a workgroup the report shows.  env: the CRK_* switches (csrc/switches.h) that make the route choose the kernel.
# work: what runs (below).  per_block: slots also printed divided by the stack's block count.
KERNELS = {
    "s2": dict(src="stack2_kernels.hip", flag="-DSK_PROF=1", kernel="stack2_fwd_kernel", work="gated_fwd", waves=8, total=7, env={},
               slots=["taps", "gate", "wait A", "1x1+upd", "operand", "wait B", "prologue barrier", "TOTAL", "pro: first conv / state",
                      "pro: tables", "pro: cond tile", "pro: operand put", "pro: bias req", "pro: other req", "pro: x -> LDS",
                      "pro: x barrier"],
               per_block=(0, 1, 2, 3, 4, 5)),
    "s2b": dict(src="stack2b_kernels.hip", flag="-DSK_PROF=1", kernel="stack2_bwd_kernel", work="gated_bwd", waves=4, total=7, env={},
                slots=["prologue", "P1 1x1+gate", "wait A", "taps(rest)", "dX epi", "wait B", "first conv", "TOTAL", "step0", "steps1-8",
                       "steps9-16"],
                per_block=(1, 2, 8, 9, 10, 3, 4, 5)),
    "skb": dict(src="stack_kernels.hip", flag="-DSK_PROF=1", kernel="stack_bwd_kernel", work="gated_bwd", waves=8, total=7,
                env={"CRK_SKB_V": "1"},
                slots=["prologue", "barrier", "1x1 mfma", "gate bwd", "taps", "dX epi", "commit", "TOTAL", "1x1 issue loads", "1x1 convert"],
                per_block=(1, 8, 9, 2, 3, 4, 5, 6)),
    "ps": dict(src="pstack_kernels.hip", flag="-DSK_PROF=1", kernel="pstack_kernel", work="plain", waves=8, total=5,
               env={"CRK_PS_V": "1"}, slots=["prologue", "taps", "chunk barrier", "commit", "epilogue", "TOTAL"], per_block=()),
    "ps2": dict(src="pstack2_kernels.hip", flag="-DSK_PROF=1", kernel="pstack2_kernel", work="plain", waves=8, total=5, env={},
                slots=["pro: operand -> LDS + barrier", "fragment wait + MFMAs", "next fragments + epilogue", "barrier", "pro: requests",
                       "TOTAL", "pro: table, guards", "pro: biases"],
                per_block=()),
    "pw": dict(src="pstack_wgrad_kernels.hip", flag="-DSK_PROF=1", kernel="pstack_wgrad_body", work="plain_wgrad", waves=4, total=5, env={},
               slots=["set-up", "barrier + tiles -> LDS + barrier", "next requests", "fragments + MFMAs", "partial sums out", "TOTAL"],
               per_block=()),
}


def lib_path(key):
    return os.path.join(REPO, "crank_amd", f"libcrank_hip_prof_{key}.so")


def build(key):
    k = KERNELS[key]
    subprocess.run(["bash", os.path.join(REPO, "tools", "build_variant.sh"), "prof_" + key, k["src"], k["flag"]], check=True)


def read_prof(L):
    """(cycles [WGS, WAVES, SLOTS], res [WGS, 4], workgroups and waves per workgroup of the last timed launch) written since
    the previous call; the call clears the device buffers."""
    import numpy as np

    L.crk_debug_sk_prof.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.crk_debug_sk_prof.restype = ctypes.c_int
    cyc = np.zeros(WGS * WAVES * SLOTS, dtype=np.uint64)
    res = np.zeros((WGS + 1) * 4, dtype=np.uint64)
    assert L.crk_debug_sk_prof(cyc.ctypes.data, res.ctypes.data) == 0
    res = res.reshape(WGS + 1, 4)
    return cyc.reshape(WGS, WAVES, SLOTS), res[:WGS], int(res[WGS, 0]), int(res[WGS, 1])


def report(L, key, tag, layers, check):
    import numpy as np

    k = KERNELS[key]
    names, total = k["slots"], k["total"]
    cyc, res, grid, lwaves = read_prof(L)
    if grid == 0 or lwaves == 0:
        sys.exit(f"{tag}: {k['kernel']} did not run (no launch wrote the timer's buffers): wrong library or route")
    nw = min(lwaves, k["waves"], WAVES)
    live = res[res[:, 1] > 0]
    v = cyc[: len(live), :nw, : len(names)].astype(np.float64)
    if check:
        assert len(live) == min(grid, WGS) and (res[: len(live), 1] > 0).all(), (tag, "workgroups recorded", len(live), "launched", grid)
        assert (v[:, :, total] > 0).all(), (tag, "a recorded wave has no TOTAL")
        assert (v <= v[:, :, total:total + 1]).all(), (tag, "a slot is larger than its wave's TOTAL")
        assert (live[:, 1] >= live[:, 0]).all(), (tag, "a workgroup ends before it starts")
    # residency from HW_ID: (XCC, SE, SA, CU) -> the workgroups that overlapped there
    ev = {}
    for a_, b_, hw, xcc in live:
        cu = (int(xcc) & 0xf, (int(hw) >> 13) & 7, (int(hw) >> 12) & 1, (int(hw) >> 8) & 0xf)
        ev.setdefault(cu, []).extend([(int(a_), 1), (int(b_), -1)])
    mx = 0
    for lst in ev.values():
        c = 0
        for _, d in sorted(lst):
            c += d
            mx = max(mx, c)
    t0 = live[:, 0].min()
    life = (live[:, 1] - live[:, 0]).astype(np.float64) / 100.0
    print(f"{tag}: {grid} workgroups of {lwaves} waves, {len(live)} recorded on {len(ev)} CUs, max co-resident per CU {mx}, workgroup life "
          f"{life.mean():.1f} us (min {life.min():.1f} max {life.max():.1f}), kernel span {(live[:, 1].max() - t0) / 100.0:.1f} us, "
          f"last start at {(live[:, 0].max() - t0) / 100.0:.1f} us")
    for w in range(nw):
        print(f"  wave {w}: " + "  ".join(f"{n} {v[:, w, i].mean():8.0f}" for i, n in enumerate(names)))
    mean = v.mean(axis=(0, 1))
    print("  all   : " + "  ".join(f"{n} {mean[i]:8.0f}" for i, n in enumerate(names)) +
          (" | per block: " + " ".join(f"{names[i]} {mean[i] / layers:.0f}" for i in k["per_block"]) if k["per_block"] and layers else ""))
    if check:
        print(f"  check ok: {len(live)} = min({grid}, {WGS}) workgroups, every wave TOTAL > 0, every slot <= TOTAL, every end >= start")


def run_gated(L, key, B, T, check):
    import torch
    from crank_amd.net.module.flat import FlatModel
    from crank_amd.net.module.pwg import KIND_GENERATOR, HipStack

    for tag, cin, cout, k, layers, stacks, aux in (GATED[-1:] if check else GATED):
        class M(FlatModel):
            def __init__(self):
                super().__init__()
                self.stack = HipStack(KIND_GENERATOR, cin, cout, k, layers, stacks=stacks, aux_channels=aux, bias=True)
                self._alloc(self.stack.entries("", 0), self.stack.n_params, "cuda")
                self.stack.bind(self, 0)
                self.stack.init_parameters()
        m = M()
        what = f"{tag} ({layers} blocks, k{k}, aux {aux})"
        if KERNELS[key]["work"] == "gated_fwd":
            x = torch.randn(B, T, cin, device="cuda")
            a = torch.randn(B, T, aux, device="cuda") if aux else None
            for grad in (False, True):
                with torch.set_grad_enabled(grad):
                    xi = x.clone().requires_grad_(grad)
                    m.stack(xi, c=a)
                    read_prof(L)
                    m.stack(xi, c=a)
                report(L, key, f"{what} forward, {'saving' if grad else 'no-grad'}", layers, check)
        else:
            x = torch.randn(B, T, cin, device="cuda", requires_grad=True)
            a = torch.randn(B, T, aux, device="cuda", requires_grad=True) if aux else None
            for it in range(2):
                y = m.stack(x, c=a)
                read_prof(L)
                y.backward(torch.ones_like(y))
            report(L, key, f"{what} data gradient", layers, check)


def run_plain(L, key, B, T, check):
    import torch
    from crank_amd.bin.train import get_model
    from crank_amd.utils import load_yaml

    m = get_model(load_yaml(None, batch_size=B, batch_len=T), 14, "cuda")
    x = torch.randn(B, T, 80, device="cuda", requires_grad=True)
    e = torch.randn(B, T, 128, device="cuda", requires_grad=True)
    fwd = {"C": lambda: m["C"](x.transpose(1, 2)), "SPKRADV": lambda: m["SPKRADV"]([e[..., :64], e[..., 64:]])}
    wgrad = KERNELS[key]["work"] == "plain_wgrad"
    for net in (PLAIN[-1:] if check else PLAIN):
        for it in range(2):
            read_prof(L)
            y = fwd[net]()
            if it == 1 and not wgrad:
                report(L, key, f"{net} forward", 0, check)
            y.sum().backward()
        report(L, key, f"{net} weight gradient" if wgrad else f"{net} data gradient", 0, check)


def main(argv):
    if not argv or argv[0] not in KERNELS:
        sys.exit(__doc__ + "\nkernels: " + " ".join(KERNELS))
    key, rest = argv[0], argv[1:]
    if rest[:1] == ["build"]:
        return build(key)
    check = "--check" in rest
    rev = rest[rest.index("--rev") + 1] if "--rev" in rest else "unknown revision"
    os.environ["CRANK_AMD_LIB"] = lib_path(key)
    os.environ.update(KERNELS[key]["env"])
    from crank_amd import _lib, ops

    ops.set_precision("bf16")
    L = _lib.lib()
    if not hasattr(L, "crk_debug_sk_prof"):
        sys.exit(f"{lib_path(key)} has no phase timer: python tools/phase_cycles.py {key} build")
    B, T = (2, 150) if check else (64, 500)
    k = KERNELS[key]
    print(f"# phase cycles of {k['kernel']} ({k['src']} {k['flag']}{''.join(' ' + a + '=' + b for a, b in k['env'].items())}) at {rev}, "
          f"B = {B}, T = {T}: shader cycles per wave, mean over the recorded workgroups")
    (run_plain if k["work"].startswith("plain") else run_gated)(L, key, B, T, check)


if __name__ == "__main__":
    main(sys.argv[1:])
