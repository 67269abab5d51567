"""The batch layout of a conv net, restated from the library's host code (no GPU, no library): what
crk_debug_net_layout reports for a reserved shape, computed here from the rules the comments in net.hip and
stack2b_kernels.hip state.  GPU tests assert library == restatement == the edge a case is named after before they compare
values, so a plan that changes later fails a precondition instead of silently testing another layout.

A net is a dict: kind "generator" | "discriminator" | "plain", kernel_size, layers (gated blocks, or convs of a plain chain),
stacks, aux_channels.  Default process switches only (CRK_WG_GROUPS 32, CRK_WG_FILL 1, CRK_WG_CPG unset)."""

CHUNK = 64          # frames per weight-gradient chunk
CUS = 256           # compute units the planners fill
KEYS = ("Gs", "cpg_s", "Gg", "cpg", "nseg", "ft")  # crk_debug_net_layout out[0..5]; out[6] (forward rows) is not restated


def ceil_div(a, b):
    return -(-a // b)


def chunks_per_utt(T):
    return ceil_div(T, CHUNK)


def stack_cpg(net, B, T, groups=32):
    """net.hip::stack_cpg: chunks per weight-gradient group of the gated blocks' region.  Groups of whole utterances, `groups`
    of them; a gated stack of few blocks gets as many groups as fill the compute units with (group, block) workgroups."""
    ncpu = chunks_per_utt(T)
    cpg = ceil_div(B, groups) * ncpu
    L = net["layers"]
    if net["kind"] != "plain" and L > 0 and CUS // L > groups:
        c = ceil_div(B * ncpu, CUS // L)
        if 1 <= c < cpg:
            cpg = c
    return max(cpg, 1)


def stack_groups(net, B, T):
    return ceil_div(B * chunks_per_utt(T), stack_cpg(net, B, T))


def usum_nseg(net, B, T):
    """Per-utterance sum segments a group needs: a group of cpg chunks that starts at the last chunk of an utterance."""
    ncpu = chunks_per_utt(T)
    return (stack_cpg(net, B, T) + 2 * ncpu - 2) // ncpu


def generic_groups(net, B, T):
    """shape_need's generic region (a plain chain's convs; a gated net's first conv and head): (Gg, cpg).  At most 32 groups,
    64 for a plain chain of at most 4 convs."""
    total = B * chunks_per_utt(T)
    groups = 64 if net["kind"] == "plain" and net["layers"] <= 4 else 32
    cpg = ceil_div(total, groups)
    return ceil_div(total, cpg), cpg


def stack_halo(net):
    """hl + hr of a gated stack: (kernel_size - 1) x the sum of its blocks' dilations 2^(l mod layers per stack)."""
    lps = net["layers"] // max(net["stacks"], 1)
    return (net["kernel_size"] - 1) * sum(2 ** (l % lps) for l in range(net["layers"]))


def stack2_bwd_plan(net, B, T):
    """stack2b_kernels.hip::stack2_bwd_plan: (ft, frames per window, windows per utterance) of the channel-split
    data-gradient chain; ft = 0: no plan.  Cost = rounds of 256 workgroups x 64-frame tiles per window, ties to the larger."""
    if net["kind"] == "plain" or net["kernel_size"] not in (3, 5) or net["aux_channels"] > 64 or net["layers"] > 16:
        return 0, 0, 0
    halo = stack_halo(net)
    best, best_cost = 0, 0
    for ft in (2, 3):
        tmo = 64 * ft - halo
        if tmo < 16:
            continue
        cost = ceil_div(B * ceil_div(T, tmo), CUS) * ft
        if not best or cost < best_cost or (cost == best_cost and ft > best):
            best, best_cost = ft, cost
    if not best:
        return 0, 0, 0
    tiles = ceil_div(T, 64 * best - halo)
    return best, ceil_div(T, tiles), tiles


def layout(net, B, T):
    """{key: value} as crk_debug_net_layout reports out[0..5] for a net whose plain-bf16 route runs channel-split."""
    gated = net["kind"] != "plain"
    Gg, cpg = generic_groups(net, B, T)
    return {
        "Gs": stack_groups(net, B, T) if gated else 0,
        "cpg_s": stack_cpg(net, B, T) if gated else 0,
        "Gg": Gg, "cpg": cpg,
        "nseg": usum_nseg(net, B, T) if gated and net["aux_channels"] > 0 else 0,
        "ft": stack2_bwd_plan(net, B, T)[0],
    }


def group_runs(B, T, cpg):
    """The groups of a region as (first chunk, one past the last chunk) over the B * chunks_per_utt(T) chunks of the batch."""
    total = B * chunks_per_utt(T)
    return [(c, min(c + cpg, total)) for c in range(0, total, cpg)]


def utterances_of(run, T):
    """Utterances a group's chunks belong to."""
    ncpu = chunks_per_utt(T)
    return sorted({c // ncpu for c in range(run[0], run[1])})


def last_chunk_frames(T):
    return T - (chunks_per_utt(T) - 1) * CHUNK


# The six nets of a training step (crank_amd/conf/default.yml), by the names the tests use.
NETS = {
    "enc0": dict(kind="generator", in_channels=80, out_channels=64, kernel_size=5, layers=8, stacks=4, aux_channels=0),
    "enc1": dict(kind="generator", in_channels=64, out_channels=64, kernel_size=3, layers=6, stacks=3, aux_channels=0),
    "dec0": dict(kind="generator", in_channels=128, out_channels=80, kernel_size=5, layers=8, stacks=4, aux_channels=34),
    "D": dict(kind="discriminator", in_channels=113, out_channels=1, kernel_size=5, layers=8, stacks=4, aux_channels=0),
    "C": dict(kind="plain", in_channels=80, out_channels=14, kernel_size=5, layers=8, stacks=1, aux_channels=0),
    "SPKRADV": dict(kind="plain", in_channels=128, out_channels=14, kernel_size=3, layers=3, stacks=1, aux_channels=0),
}

# (net, B, T, layout): the oracle cases of tests/test_gpu_batch_layout.py; test_net_layout_cpu.py names each one's edge
ORACLE_CASES = [
    ("C", 13, 130, dict(Gs=0, cpg_s=0, Gg=20, cpg=2, nseg=0, ft=0)),
    ("C", 33, 193, dict(Gs=0, cpg_s=0, Gg=27, cpg=5, nseg=0, ft=0)),
    ("SPKRADV", 33, 193, dict(Gs=0, cpg_s=0, Gg=44, cpg=3, nseg=0, ft=0)),
    ("D", 33, 130, dict(Gs=17, cpg_s=6, Gg=25, cpg=4, nseg=0, ft=2)),
    ("enc0", 129, 100, dict(Gs=26, cpg_s=10, Gg=29, cpg=9, nseg=0, ft=3)),
    ("dec0", 129, 100, dict(Gs=26, cpg_s=10, Gg=29, cpg=9, nseg=6, ft=3)),
    ("enc1", 129, 120, dict(Gs=37, cpg_s=7, Gg=29, cpg=9, nseg=0, ft=3)),
    ("enc1", 26, 257, dict(Gs=33, cpg_s=4, Gg=26, cpg=5, nseg=0, ft=2)),
    ("D", 129, 100, dict(Gs=26, cpg_s=10, Gg=29, cpg=9, nseg=0, ft=3)),
]
