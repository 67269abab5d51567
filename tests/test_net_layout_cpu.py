"""tests/net_layout.py (the host restatement of the library's batch layout) pinned on the figures the comments in net.hip
state and on the edges tests/test_gpu_batch_layout.py names its cases after.  No GPU, no library."""
import pytest

from tests import net_layout as nl
from tests.net_layout import NETS, ORACLE_CASES

ENC1_8 = dict(NETS["enc1"], layers=8, stacks=4)  # a k = 3 stack of 8 blocks


def test_benchmark_shape_figures_of_net_hip():
    B, T = 64, 500
    assert nl.chunks_per_utt(T) == 8
    # "6 x 40 are 240 [workgroups] of 13 [chunks]"
    assert (nl.stack_groups(NETS["enc1"], B, T), nl.stack_cpg(NETS["enc1"], B, T)) == (40, 13)
    # "A stack of 8 blocks keeps its 32 groups of two utterances"
    for net in (NETS["enc0"], NETS["dec0"], NETS["D"], ENC1_8):
        assert (nl.stack_groups(net, B, T), nl.stack_cpg(net, B, T)) == (32, 16)
        assert all(nl.utterances_of(r, T) == [2 * g, 2 * g + 1] for g, r in enumerate(nl.group_runs(B, T, 16)))
    # generic region: "32 groups (16 each)"; "a chain of few convs (the speaker-adversarial net: 3) keeps 64 groups"
    assert nl.generic_groups(NETS["C"], B, T) == (32, 16)
    assert nl.generic_groups(NETS["enc0"], B, T) == (32, 16)
    assert nl.generic_groups(NETS["SPKRADV"], B, T) == (64, 8)
    assert nl.generic_groups(dict(NETS["SPKRADV"], layers=5), B, T) == (32, 16)
    # the classifier walks 16 chunks per group, the speaker-adversarial net 8, a 6-block stack 13
    assert nl.layout(NETS["C"], B, T) == dict(Gs=0, cpg_s=0, Gg=32, cpg=16, nseg=0, ft=0)
    assert nl.layout(NETS["dec0"], B, T) == dict(Gs=32, cpg_s=16, Gg=32, cpg=16, nseg=3, ft=3)
    assert nl.layout(NETS["enc1"], 128, T)["cpg_s"] == 25 and nl.layout(NETS["enc0"], 128, T)["cpg_s"] == 32


def test_small_batches_give_every_chunk_its_own_group():
    """B <= 4 at T = 500: cpg = 1 in the generic region of every net - what the oracle tests before this file covered."""
    for name, net in NETS.items():
        for B in (1, 2, 3, 4):
            assert nl.generic_groups(net, B, 500)[1] == 1, (name, B)
    # sub-batches of one and two: no stack group holds more than one utterance
    for net in (NETS["enc0"], NETS["enc1"], NETS["dec0"], NETS["D"]):
        for B in (1, 2):
            for T in (449, 500):
                cpg = nl.stack_cpg(net, B, T)
                assert cpg <= nl.chunks_per_utt(T)
                assert all(len(nl.utterances_of(r, T)) == 1 for r in nl.group_runs(B, T, cpg)), (net, B, T)


def test_halo_and_window_choice_of_the_data_gradient_chain():
    assert nl.stack_halo(NETS["enc0"]) == 48 and nl.stack_halo(NETS["enc1"]) == 18
    # every shape the value tests ran before: ft = 2
    for net, B, T in ((NETS["dec0"], 2, 500), (NETS["enc0"], 2, 500), (NETS["enc1"], 2, 333), (NETS["enc1"], 9, 300),
                      (NETS["D"], 2, 200), (NETS["D"], 3, 300), (NETS["dec0"], 3, 500), (NETS["enc1"], 3, 500)):
        assert nl.stack2_bwd_plan(net, B, T)[0] == 2, (net, B, T)
    # the benchmark's shapes: ft = 3 (192 rows)
    for net in (NETS["enc0"], NETS["enc1"], NETS["dec0"], NETS["D"]):
        for B in (64, 128):
            assert nl.stack2_bwd_plan(net, B, 500)[0] == 3
    assert nl.stack2_bwd_plan(NETS["enc0"], 64, 500) == (3, 125, 4)
    assert nl.stack2_bwd_plan(NETS["enc1"], 64, 500) == (3, 167, 3)
    # a halo that leaves ft = 2 no room (k = 5, 8 blocks in 2 stacks: dilations 1 .. 8, 120 frames)
    assert nl.stack2_bwd_plan(dict(NETS["enc0"], stacks=2), 2, 200)[0] == 3
    assert nl.stack2_bwd_plan(NETS["C"], 64, 500) == (0, 0, 0)
    # the shapes test_gpu_properties.py adds to its bitwise family comparison
    assert nl.stack2_bwd_plan(NETS["enc0"], 37, 500)[0] == 3   # 259 workgroups at ft = 2
    assert nl.stack2_bwd_plan(NETS["enc1"], 52, 500)[0] == 3   # 260
    assert nl.stack2_bwd_plan(NETS["D"], 37, 500)[0] == 3
    assert nl.generic_groups(NETS["C"], 33, 193) == (27, 5)


@pytest.mark.parametrize("name,B,T,want", ORACLE_CASES)
def test_oracle_case_layouts(name, B, T, want):
    assert nl.layout(NETS[name], B, T) == want


def test_oracle_case_edges():
    """What each case is named after, from the group runs."""
    # C 13 x 130: cpg 2 against 3 chunks per utterance; every second group crosses an utterance end; last chunk 2 frames;
    # last group 1 chunk
    runs = nl.group_runs(13, 130, 2)
    assert nl.chunks_per_utt(130) == 3 and nl.last_chunk_frames(130) == 2
    assert [len(nl.utterances_of(r, 130)) for r in runs[:6]] == [1, 2, 1, 1, 2, 1]
    assert sum(len(nl.utterances_of(r, 130)) == 2 for r in runs) == 6
    assert runs[-1][1] - runs[-1][0] == 1
    # C 33 x 193: cpg 5 against 4; last group 2 chunks; last chunk 1 frame; 5 chunks = register sets 0 1 0 1 0
    runs = nl.group_runs(33, 193, 5)
    assert nl.chunks_per_utt(193) == 4 and nl.last_chunk_frames(193) == 1
    assert len(runs) == 27 and runs[-1][1] - runs[-1][0] == 2
    assert all(len(nl.utterances_of(r, 193)) >= 2 for r in runs[:-1])
    # SPKRADV 33 x 193: the 64-group rule
    runs = nl.group_runs(33, 193, 3)
    assert len(runs) == 44 and any(len(nl.utterances_of(r, 193)) == 2 for r in runs)
    # D 33 x 130: gated region two whole utterances per group, last group one; the generic region's groups of 4 cross
    runs = nl.group_runs(33, 130, 6)
    assert [nl.utterances_of(r, 130) for r in runs[:2]] == [[0, 1], [2, 3]] and nl.utterances_of(runs[-1], 130) == [32]
    assert any(len(nl.utterances_of(r, 130)) == 2 for r in nl.group_runs(33, 130, 4))
    # enc0 / dec0 / D 129 x 100: 258 windows at ft = 2, five utterances per group
    assert 129 * nl.ceil_div(100, 128 - 48) == 258 and 129 * nl.ceil_div(100, 192 - 48) == 129
    runs = nl.group_runs(129, 100, 10)
    assert all(len(nl.utterances_of(r, 100)) == 5 for r in runs[:-1]) and len(nl.utterances_of(runs[-1], 100)) == 4
    # enc1 129 x 120: the fill rule, 37 groups of 7 chunks against 2 chunks per utterance
    assert 129 * nl.ceil_div(120, 128 - 18) == 258
    runs = nl.group_runs(129, 120, 7)
    assert len(runs) == 37 and runs[1][0] % 2 == 1  # the second group begins inside an utterance
    # enc1 26 x 257: cpg 4 against 5 chunks per utterance; last chunk 1 frame
    assert nl.chunks_per_utt(257) == 5 and nl.last_chunk_frames(257) == 1
    assert any(len(nl.utterances_of(r, 257)) == 2 for r in nl.group_runs(26, 257, 4))
