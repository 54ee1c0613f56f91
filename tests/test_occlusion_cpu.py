"""The occluder stage of the training-batch maker without a device: the integer area resize and the blend of tests/occlusion_reference.py
(the definition csrc/augment.hip restates), the host plan of whmr_amd.datasets.train_batch and the draws of ``draw_occlusions``."""
import random

import numpy as np
import pytest

import occlusion_reference as OR
from whmr_amd.datasets import OccluderBank, TrainBatchMaker, draw_occlusions
from whmr_amd.datasets import train_batch as TB
from whmr_amd.datasets.train_batch import plan_occlusions


def _rgba(rng, h, w):
    return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)


# ----------------------------------------------------------------------------- resize
def test_resize_is_the_identity_at_factor_one():
    img = _rgba(np.random.default_rng(0), 13, 9)
    assert np.array_equal(OR.area_resize_u8(img, 9, 13), img)


def test_resize_two_to_one_is_the_rounded_block_mean():
    img = _rgba(np.random.default_rng(1), 12, 10)
    s = img.astype(np.int64).reshape(6, 2, 5, 2, 4).sum(axis=(1, 3))
    assert np.array_equal(OR.area_resize_u8(img, 5, 6), ((2 * s + 4) // 8).astype(np.uint8))


def _float_area_average(img, nw, nh):
    """float64 area average from real overlaps: output u covers [u S / n, (u + 1) S / n) source texels"""
    def weights(S, n):
        u, j = np.arange(n, dtype=np.float64)[:, None], np.arange(S, dtype=np.float64)[None, :]
        return np.maximum(0.0, np.minimum((u + 1) * S / n, j + 1) - np.maximum(u * S / n, j)) / (S / n)
    h, w = img.shape[:2]
    return np.einsum('vy,yxc,ux->vuc', weights(h, nh), img.astype(np.float64), weights(w, nw))


def test_resize_stays_within_half_a_level_of_the_float64_area_average():
    rng = np.random.default_rng(2)
    for _ in range(12):
        h, w = (int(v) for v in rng.integers(1, 70, 2))
        nw, nh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
        img = _rgba(rng, h, w)
        d = np.abs(OR.area_resize_u8(img, nw, nh).astype(np.float64) - _float_area_average(img, nw, nh))
        assert d.max() <= 0.5 + 1e-9, (h, w, nw, nh, d.max())


# ----------------------------------------------------------------------------- rounding
def test_sizes_and_centres_round_half_to_even():
    assert OR.paste_size(5, 5, 0.5) == (2, 2) and OR.paste_size(7, 7, 0.5) == (4, 4)
    assert OR.paste_start(10.5, 11.5, 0, 0) == (10, 12)
    sizes = np.array([[5, 7]])
    rows, ptr = plan_occlusions([np.array([[0, 0.5, 100.5, 101.5]])], sizes)           # (w, h) = (7, 5) -> (4, 2); centre -> (100, 102)
    assert rows.tolist() == [[0, 4, 2, 100 - 2, 102 - 1]] and ptr.tolist() == [0, 1]


# ----------------------------------------------------------------------------- paste
def test_alpha_zero_leaves_the_patch_and_alpha_255_copies():
    rng = np.random.default_rng(3)
    patch = rng.integers(0, 256, (256, 256, 3)).astype(np.uint8)
    obj = _rgba(rng, 20, 30)
    obj[..., 3] = 0
    assert np.array_equal(OR.occlude_patch(patch, [obj], [(0, 1.0, 100, 90)]), patch)
    obj[..., 3] = 255
    out = OR.occlude_patch(patch, [obj], [(0, 1.0, 100, 90)])
    assert np.array_equal(out[80:100, 85:115], obj[..., :3])
    rest = np.ones((256, 256), dtype=bool)
    rest[80:100, 85:115] = False
    assert np.array_equal(out[rest], patch[rest])


@pytest.mark.parametrize('cx, cy', [(3, 128), (253, 128), (128, 2), (128, 254), (32, 128), (224, 128), (1, 1), (255, 255)])
def test_rectangles_cut_by_the_borders_and_by_the_kept_columns(cx, cy):
    """a 20 x 30 opaque object over each patch border and over columns 32 / 224: the clipped paste equals the slice of an unclipped canvas, and
    restricted to the kept columns it equals the kept columns of the whole-patch paste"""
    rng = np.random.default_rng(4)
    patch = rng.integers(0, 256, (256, 256, 3)).astype(np.uint8)
    obj = _rgba(rng, 20, 30)
    obj[..., 3] = rng.choice([0, 255, 90], size=(20, 30))
    out = OR.occlude_patch(patch, [obj], [(0, 1.0, cx, cy)])
    canvas = np.zeros((256 + 80, 256 + 80, 3), dtype=np.uint8)
    canvas[40:-40, 40:-40] = patch
    big = OR.paste_over(canvas, obj, cx - 15 + 40, cy - 10 + 40, x_range=(0, 336))
    assert np.array_equal(out, big[40:-40, 40:-40])
    assert (out != patch).any()
    kept = OR.occlude_patch(patch, [obj], [(0, 1.0, cx, cy)], x_range=(OR.X0, OR.X1))
    assert np.array_equal(kept[:, OR.X0:OR.X1], out[:, OR.X0:OR.X1])
    assert np.array_equal(kept[:, :OR.X0], patch[:, :OR.X0]) and np.array_equal(kept[:, OR.X1:], patch[:, OR.X1:])


def test_order_matters_for_overlapping_pastes():
    rng = np.random.default_rng(5)
    patch = rng.integers(0, 256, (256, 256, 3)).astype(np.uint8)
    a, b = _rgba(rng, 40, 40), _rgba(rng, 40, 40)
    a[..., 3], b[..., 3] = 200, 120
    ab = OR.occlude_patch(patch, [a, b], [(0, 1.0, 100, 100), (1, 1.0, 110, 110)])
    ba = OR.occlude_patch(patch, [a, b], [(1, 1.0, 110, 110), (0, 1.0, 100, 100)])
    assert not np.array_equal(ab, ba)
    assert np.array_equal(ab, OR.occlude_patch(OR.occlude_patch(patch, [a, b], [(0, 1.0, 100, 100)]), [a, b], [(1, 1.0, 110, 110)]))


# ----------------------------------------------------------------------------- host plan
def _bank_objects():
    rng = np.random.default_rng(6)
    return [_rgba(rng, h, w) for h, w in ((1, 1), (5, 7), (40, 33), (128, 96))]


def _standin_maker(occluders):
    """a TrainBatchMaker without a device: only what the occlusion plan reads (the bank is packed into host memory)"""
    m = TrainBatchMaker.__new__(TrainBatchMaker)
    m.is_train = True
    m.bank = OccluderBank(occluders, 'cpu') if occluders is not None else None
    return m


def test_bank_packs_objects_back_to_back():
    objs = _bank_objects()
    bank = OccluderBank(objs, 'cpu')
    assert len(bank) == 4 and bank.sizes.tolist() == [[1, 1], [5, 7], [40, 33], [128, 96]]
    assert bank.table.dtype.is_floating_point is False and bank.table.tolist() == [[0, 1, 1], [4, 5, 7], [144, 40, 33], [5424, 128, 96]]
    raw = bank.bank.numpy()
    assert raw.dtype == np.uint8 and raw.size == 5424 + 128 * 96 * 4
    for (off, h, w), o in zip(bank.table.tolist(), objs):
        assert np.array_equal(raw[off:off + h * w * 4].reshape(h, w, 4), o)


@pytest.mark.parametrize('bad', [[], [np.zeros((3, 3, 3), np.uint8)], [np.zeros((3, 3, 4), np.float32)], [np.zeros((0, 3, 4), np.uint8)],
                                 [np.zeros((3, 4), np.uint8)], [[[0, 0, 0, 0]]]])
def test_bank_rejects_what_is_not_uint8_rgba(bad):
    with pytest.raises(ValueError):
        OccluderBank(bad, 'cpu')


def test_plan_equals_the_reference_rectangles_and_drops_what_cannot_show():
    objs = _bank_objects()
    m = _standin_maker(objs)
    occ = [np.array([[3, 1.0, 128, 128], [2, 0.73, 30.5, 250.5], [1, 0.5, 11.5, 10.5], [3, 0.2, 229.4, 3.6]]),
           np.array([[0, 0.3, 100, 100],                # 1 x 1 at 0.3 -> size 0: dropped
                     [1, 1.0, 20, 100],                 # 7 wide about x = 20: ends at 24 <= 32, dropped
                     [1, 1.0, 228, 100],                # starts at 225 >= 224, dropped
                     [2, 1.0, 100, 300],                # rows 280 ..: dropped
                     [2, 0.5, 34, 0]]),                 # straddles column 32 and row 0: kept
           np.zeros((0, 4))]
    rows, ptr = m._occlusion_plan(occ, 3)
    assert rows.dtype == np.int32 and ptr.dtype == np.int32 and ptr.tolist() == [0, 3, 4, 4]
    want0 = OR.rectangles(objs, occ[0])
    assert want0[2] == (1, 4, 2, 12 - 2, 10 - 1)
    assert rows[:3].tolist() == [list(r) for r in (want0[0], want0[1], want0[3])]          # the 5 x 7 object about x = 12 misses column 32
    assert rows[3].tolist() == list(OR.rectangles(objs, occ[1])[-1])
    # every kept rectangle meets the kept columns and the rows
    assert ((rows[:, 3] + rows[:, 1] > 32) & (rows[:, 3] < 224) & (rows[:, 4] + rows[:, 2] > 0) & (rows[:, 4] < 256)).all()


def test_plan_rejects_bad_input():
    m = _standin_maker(_bank_objects())
    for bad in (4, -1, 1.5):
        with pytest.raises(ValueError):
            m._occlusion_plan([np.array([[bad, 0.5, 100, 100]])], 1)
    with pytest.raises(ValueError):
        m._occlusion_plan([np.array([[0, 1.5, 100, 100]])], 1)                            # the resize only shrinks
    with pytest.raises(ValueError):
        m._occlusion_plan([np.zeros((0, 4))], 2)                                          # one entry per sample
    with pytest.raises(ValueError):
        _standin_maker(None)._occlusion_plan([np.zeros((0, 4))], 1)                       # occlusions= without a bank
    rows, ptr = _standin_maker(None)._occlusion_plan(None, 3)
    assert len(rows) == 0 and ptr.tolist() == [0, 0, 0, 0]


def test_plan_draws_when_training_only():
    m = _standin_maker(_bank_objects())
    np.random.seed(7)
    random.seed(7)
    rows, ptr = m._occlusion_plan(None, 5)
    assert ptr[0] == 0 and ptr[-1] == len(rows) and (np.diff(ptr) <= 7).all() and len(rows) > 0
    m.is_train = False
    assert len(m._occlusion_plan(None, 5)[0]) == 0


# ----------------------------------------------------------------------------- draws
def test_draws_are_reproducible_and_consume_the_reference_streams():
    n, n_occ = 40, 9
    a = draw_occlusions(n, n_occ, rng=np.random.RandomState(11), pyrng=random.Random(12))
    rng, pyrng = np.random.RandomState(11), random.Random(12)
    b = draw_occlusions(n, n_occ, rng=rng, pyrng=pyrng)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    counts = np.array([len(x) for x in a])
    assert counts.min() >= 1 and counts.max() <= 7 and set(counts) == set(range(1, 8))
    rows = np.concatenate(a)
    assert rows.dtype == np.float64 and rows.shape[1] == 4
    assert (rows[:, 1] >= 0.2).all() and (rows[:, 1] <= 1.0).all() and (rows[:, 2:] >= 0).all() and (rows[:, 2:] < 256).all()
    assert (rows[:, 0] == np.floor(rows[:, 0])).all() and rows[:, 0].min() >= 0 and rows[:, 0].max() < n_occ
    # replay by hand: per sample one randint, then per paste one double for the factor and two for the centre (numpy), one choice (Python)
    r2, p2, seq = np.random.RandomState(11), random.Random(12), list(range(n_occ))
    for x in a:
        assert r2.randint(1, 8) == len(x)
        for row in x:
            assert p2.choice(seq) == row[0]
            f, cx, cy = r2.random_sample(), r2.random_sample(), r2.random_sample()
            assert row[1] == 0.2 + (1.0 - 0.2) * f and row[2] == 256 * cx and row[3] == 256 * cy
    s1, s2 = rng.get_state(), r2.get_state()
    assert s1[0] == s2[0] and np.array_equal(s1[1], s2[1]) and s1[2:] == s2[2:]
    assert pyrng.getstate() == p2.getstate()
    assert TB.RES == 256
