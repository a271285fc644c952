"""CPU, no engine: the frame packing the six probability methods of engine.py share (_pack_frames, _split_probs) and the draw
buffers its four sampling methods share (_pack_draws, _split_draws)."""
import numpy as np
import pytest

from probabilisticsemslam_amd.engine import KBestError, _pack_draws, _pack_frames, _split_draws, _split_probs

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


def test_draw_offsets_and_sizes():
    nM = np.array([s[1] for s in SHAPES], np.int32)
    n, asgOff, lpOff, assign, logp, key = _pack_draws(nM, 3, np.int64(3), None, "t")
    assert n == 3 and type(n) is int and key is None
    assert asgOff.dtype == np.int64 and lpOff.dtype == np.int64
    assert asgOff.tolist() == [0, 6, 18] and lpOff.tolist() == [0, 3, 6]
    assert assign.dtype == np.int32 and assign.size == 21 and not assign.any()
    assert logp.dtype == np.float64 and logp.size == 9 and not logp.any()
    key = _pack_draws(nM, 3, 3, [5, 2**63 + 1, 0], "t")[5]
    assert key.dtype == np.uint64 and key.flags.c_contiguous and key.tolist() == [5, 2**63 + 1, 0]


def test_draw_views_alias_the_flat_arrays():
    nM = np.array([s[1] for s in SHAPES], np.int32)
    n, asgOff, lpOff, assign, logp, _ = _pack_draws(nM, 3, 3, None, "t")
    asg, lp = _split_draws(assign, asgOff, logp, lpOff, nM, n)
    assert [a.shape for a in asg] == [(3, 2), (3, 4), (3, 1)] and [p.shape for p in lp] == [(3,)] * 3
    assign[:] = np.arange(21)
    logp[:] = np.arange(9)
    assert np.array_equal(asg[0], np.arange(6).reshape(3, 2))
    assert np.array_equal(asg[1], np.arange(6, 18).reshape(3, 4))
    assert np.array_equal(asg[2], np.arange(18, 21).reshape(3, 1))
    assert [p.tolist() for p in lp] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]
    for a, p in zip(asg, lp):
        assert np.shares_memory(a, assign) and np.shares_memory(p, logp)
    asg[2][2, 0] = -1
    lp[1][0] = -2.5
    assert assign[20] == -1 and logp[3] == -2.5


def test_no_draw_frames():
    nM = np.zeros(0, np.int32)
    n, asgOff, lpOff, assign, logp, key = _pack_draws(nM, 0, 3, None, "t")
    for a, dt in ((asgOff, np.int64), (lpOff, np.int64), (assign, np.int32), (logp, np.float64)):
        assert a.dtype == dt and a.shape == (0,)
    assert key is None and _pack_draws(nM, 0, 3, [], "t")[5].shape == (0,)
    assert _split_draws(assign, asgOff, logp, lpOff, nM, n) == ([], [])


@pytest.mark.parametrize("who", ["sample_assoc", "clustered_sample_assoc", "hybrid_frontier_sample_assoc", "hybrid_sample_assoc"])
@pytest.mark.parametrize("keys", [[1, 2], [1, 2, 3, 4], [[1, 2, 3]], 7])
def test_frame_key_of_the_wrong_shape_names_the_caller(who, keys):
    with pytest.raises(KBestError, match=rf"^{who}: frame_key must hold one key per frame$"):
        _pack_draws(np.array([2, 4, 1], np.int32), 3, 3, keys, who)
