"""The two pure pieces of the decoder's host side (comic_amd/decoder.py): the layout of the staging blocks and the loss
coefficients.  The expected values are the formulas the training and scoring contexts used before both had one definition,
written out: offsets as literals, coefficients as the numpy lines."""
import numpy as np
import pytest

from comic_amd import decoder as cdec

# (B, T) -> (offset of the float fields, size of the block) in bytes
TRAIN_LAYOUT = {(1, 1): (24, 36),       # three int32 words padded to four
                (2, 3): (64, 136),      # 14 words, no padding
                (3, 5): (144, 324)}
SCORE_LAYOUT = {(1, 1): (16, 20), (2, 3): (56, 80), (3, 5): (136, 196)}


@pytest.mark.parametrize('shape', sorted(TRAIN_LAYOUT))
def test_training_layout(shape):
    B, T = shape
    fields = cdec.train_stage_fields(B, T)
    assert [f[0] for f in fields] == ['seed', 'inputs', 'targets', 'lens', 'wmask', 'coef', 'row_scale']
    assert [f[1] for f in fields] == ['int64'] + ['int32'] * 3 + ['float32'] * 3
    off, nbytes = cdec.staging_layout(fields)
    o_f32, total = TRAIN_LAYOUT[shape]
    assert list(off) == [f[0] for f in fields]
    assert (off['seed'], off['inputs'], off['targets'], off['lens']) == (0, 8, 8 + 4 * B * T, 8 + 8 * B * T)
    assert (off['wmask'], off['coef'], off['row_scale']) == (o_f32, o_f32 + 4 * B * T, o_f32 + 8 * B * T)
    assert nbytes == total
    assert o_f32 == 8 + 4 * ((2 * B * T + B + 1) // 2 * 2) and total == o_f32 + 12 * B * T     # the contexts' own lines


@pytest.mark.parametrize('shape', sorted(SCORE_LAYOUT))
def test_scoring_layout(shape):
    B, T = shape
    fields = cdec.score_stage_fields(B, T)
    assert [f[:2] for f in fields] == [('inputs', 'int32'), ('targets', 'int32'), ('lens', 'int32'), ('wmask', 'float32')]
    off, nbytes = cdec.staging_layout(fields)
    o_f32, total = SCORE_LAYOUT[shape]
    assert list(off) == ['inputs', 'targets', 'lens', 'wmask']
    assert (off['inputs'], off['targets'], off['lens'], off['wmask']) == (0, 4 * B * T, 8 * B * T, o_f32)
    assert nbytes == total
    assert o_f32 == 4 * ((2 * B * T + B + 1) // 2 * 2) and total == o_f32 + 4 * B * T


def _wmask():
    """[4,6] with an all-padding row and rows of different lengths."""
    w = np.zeros((4, 6), np.float32)
    for b, n in enumerate((6, 0, 3, 1)):
        w[b, :n] = 1.0
    return w


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(g, w)


def test_xe_coefficients():
    wmask, (B, T) = _wmask(), _wmask().shape
    den_xe = np.float32(wmask.sum() + np.float32(1e-12))
    rs = np.full((B, T), np.float32(1.0) / den_xe, np.float32)
    coef = wmask / den_xe
    _same(cdec.loss_coefficients(wmask, None, None, B), (coef, rs))
    assert coef[1].sum() == 0.0


def test_xe_coefficients_with_a_given_denominator():
    wmask, (B, T) = _wmask(), _wmask().shape
    den_xe = np.float32(37.5)
    rs = np.full((B, T), np.float32(1.0) / den_xe, np.float32)
    coef = wmask / den_xe
    _same(cdec.loss_coefficients(wmask, None, 37.5, B), (coef, rs))


def test_scst_coefficients_from_host_rewards():
    wmask, (B, T) = _wmask(), _wmask().shape
    rewards = np.array([0.75, -1.5, 0.1, -0.3])            # float64, as a caller's scores arrive
    den = wmask.sum(axis=1, keepdims=True) + np.float32(1e-12)
    rb = (np.asarray(rewards, np.float32)[:, None] / np.float32(B))
    rs = np.broadcast_to(rb / den, (B, T)).astype(np.float32)
    coef = wmask / den * rb
    _same(cdec.loss_coefficients(wmask, rewards, None, B), (coef, rs))
    assert np.isfinite(rs).all() and not coef[1].any()      # the all-padding row: a huge row scale on a zero loss row


def test_device_rewards_leave_zeros_for_the_device_to_fill():
    wmask, (B, T) = _wmask(), _wmask().shape
    zeros = np.zeros((B, T), np.float32)
    _same(cdec.loss_coefficients(wmask, cdec.DEVICE_REWARDS, None, B), (zeros, zeros))
