"""CPU, no engine: the frame packing the six probability methods of engine.py share (_pack_frames, _split_probs)."""
import numpy as np
import pytest

from probabilisticsemslam_amd.engine import KBestError, _pack_frames, _split_probs

SHAPES = [(3, 2), (0, 4), (5, 1)]  # (nL, nM): cost blocks of 10, 16 and 6 doubles, slices of 8, 4 and 6


def blocks(shapes=SHAPES):
    return [np.arange((l + m) * m, dtype=np.float64) + 100.0 * i for i, (l, m) in enumerate(shapes)]


def test_offsets_and_sizes():
    costs = blocks()
    nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(costs, [s[0] for s in SHAPES], [s[1] for s in SHAPES], "t")
    assert B == 3 and nL.dtype == np.int32 and nM.dtype == np.int32
    assert nL.tolist() == [3, 0, 5] and nM.tolist() == [2, 4, 1]
    assert costOff.dtype == np.int64 and probOff.dtype == np.int64
    assert costOff.tolist() == [0, 10, 26] and probOff.tolist() == [0, 8, 12]
    assert [int(p) for p in psizes] == [8, 4, 6]
    assert flat.dtype == np.float64 and flat.flags.c_contiguous and flat.size == 32
    assert np.array_equal(flat, np.concatenate(costs))
    assert probs.dtype == np.float64 and probs.size == 18 and not probs.any()


def test_blocks_of_any_shape_are_flattened():
    costs = blocks()
    costs[0] = costs[0].reshape(2, 5)  # column-major (nL+nM) x nM kept as the [nM][nL+nM] array it is
    costs[1] = costs[1].tolist()
    flat = _pack_frames(costs, [3, 0, 5], [2, 4, 1], "t")[3]
    assert np.array_equal(flat, np.concatenate(blocks()))


def test_views_alias_probs():
    nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames(blocks(), [3, 0, 5], [2, 4, 1], "t")
    out = _split_probs(probs, probOff, psizes, nL, nM)
    assert [o.shape for o in out] == [(2, 4), (4, 1), (1, 6)]
    probs[:] = np.arange(18)
    assert np.array_equal(out[0], np.arange(8).reshape(2, 4))
    assert np.array_equal(out[1], np.arange(8, 12).reshape(4, 1))
    assert np.array_equal(out[2], np.arange(12, 18).reshape(1, 6))
    for o in out:
        assert np.shares_memory(o, probs)
    out[2][0, 5] = -1.0
    assert probs[17] == -1.0


@pytest.mark.parametrize("delta", [-1, 1])
def test_wrong_sized_block_names_the_caller(delta):
    costs = blocks()
    costs[1] = np.zeros(16 + delta)
    with pytest.raises(KBestError, match=r"^permanent_probs: a cost block is not \(nL \+ nM\) x nM$"):
        _pack_frames(costs, [3, 0, 5], [2, 4, 1], "permanent_probs")


def test_no_frames():
    nL, nM, B, flat, costOff, probOff, psizes, probs = _pack_frames([], [], [], "t")
    assert B == 0
    for a, dt in ((nL, np.int32), (nM, np.int32), (flat, np.float64), (costOff, np.int64), (probOff, np.int64), (probs, np.float64)):
        assert a.dtype == dt and a.shape == (0,)
    assert len(psizes) == 0
    assert _split_probs(probs, probOff, psizes, nL, nM) == []
