"""The CPU restatement of the codebook search's chain (tests/vq_search_ref.py) against the reference quantizer's stored
indices, and the inputs the GPU test of the frame-per-lane kernel uses."""
import numpy as np
import pytest

from tests.helpers import golden
from tests.vq_search_ref import NEAR_TIE_FRAMES, NEAR_TIE_SEEDS, near_tie_case, vq_search_ref


def test_restated_chain_reproduces_the_reference_quantizers_indices():
    fx = golden("quantizer.npz")
    idx, clean = vq_search_ref(fx["tie_x"].reshape(-1, 64), fx["tie_w"])
    assert clean.all()
    assert np.array_equal(idx.reshape(fx["tie_idx"].shape), fx["tie_idx"])
    assert (idx[:9] == 7).all()  # rows on the duplicated code: the first index
    idx, clean = vq_search_ref(fx["x0"].transpose(0, 2, 1).reshape(-1, 64), fx["init_weight"])
    assert clean.all()
    assert np.array_equal(idx.reshape(fx["idx0"].shape), fx["idx0"])


@pytest.mark.parametrize("D,K", sorted(NEAR_TIE_SEEDS))
def test_near_tie_inputs_leave_no_frame_out_and_sit_on_the_twins(D, K):
    x, w = near_tie_case(D, K, NEAR_TIE_FRAMES, NEAR_TIE_SEEDS[D, K])
    idx, clean = vq_search_ref(x, w)
    assert clean.all(), int((~clean).sum())
    near = idx[: 2 * NEAR_TIE_FRAMES // 3]
    assert np.isin(near, (10, K // 2, K // 2 + 1)).all()
    assert len(np.unique(near)) > 1  # the twins do take frames: the rounding of the norms decides them
