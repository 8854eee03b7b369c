"""No-GPU checks of the test-time losses: known answers of tests/losses_ref.py derived by hand from trainer.py, the argument
checks of the dvsg_loss_* entries (no kernel is launched), and the `checkpoints` index round trip."""
import ctypes
import os

import numpy as np
import pytest

import inputs
import losses_ref as L


@pytest.fixture(scope="module")
def lib():
    from coupe.dvsg_amd import _lib
    return _lib.load()


def test_zero_mask_gives_zero_through_div_no_nan():
    rng = np.random.default_rng(0)
    p, g = rng.uniform(size=(2, 3, 4, 3)), rng.uniform(size=(2, 3, 4, 3))
    assert L.masked_MSE(p, g, np.zeros((2, 3, 4, 3))) == 0.0
    assert L.masked_MSE(p, g, np.zeros((2, 3, 4))) == 0.0
    assert L.get_surf_loss(np.zeros((1, 2, 3, 2)), np.zeros((1, 4, 4)), np.zeros((1, 4, 4)), [0.0], 4, 4) == 0.0


def test_masked_mse_of_a_constant_offset_under_a_half_ones_mask():
    """pred - gt = 0.5 everywhere, mask 1 on the left half: sum = 0.25 * n/2, sum mask = n/2, so 0.25 per sample."""
    g = np.random.default_rng(1).uniform(size=(3, 4, 8, 3))
    m = np.zeros((3, 4, 8))
    m[:, :, :4] = 1.0
    assert L.masked_MSE(g + 0.5, g, m) == pytest.approx(0.25, abs=1e-15)
    assert L.masked_MSE(g + 0.5, g, np.repeat(m[..., None], 3, axis=3)) == pytest.approx(0.25, abs=1e-15)
    # a mask of 0.5 there: (0.5 * 0.5)^2 * n/2 over 0.5 * n/2 = 0.125
    assert L.masked_MSE(g + 0.5, g, 0.5 * m) == pytest.approx(0.125, abs=1e-15)


def test_identity_is_mean_abs_F():
    F = np.zeros((2, 25, 2))
    F[0, 3, 1] = -0.5
    F[1, :, 0] = 0.1
    # sample 0: 0.5 / 50; sample 1: 25 * 0.1 / 50
    assert L.identity_loss(F) == pytest.approx((0.01 + 0.05) / 2, abs=1e-15)


def test_distortion_at_zero_displacement_is_an_eighth():
    """trainer.py:252-323 as written.  On the 5 x 5 grid mapped to [0,1] every cell has side 0.25 and s = 1.  With
    R(a, b) = (b, -a): terms 1 and 4 give v - v_1 - R(v_0 - v_1) = 0; terms 2 and 3 rotate the other way and give
    (0, -+0.5), i.e. 4 * 0.25^2 = 0.25 per cell.  (0 + 0.25 + 0.25 + 0) / 4 = 0.125."""
    for dt in (np.float64, np.float32):
        assert L.distortion_loss(inputs.v_src(2), np.zeros((2, 25, 2)), 5, dt) == 0.125


def test_distortion_of_a_one_cell_displacement():
    """The centre control point moved one cell (0.25) to the right.  It is v, v_0 or v_1 of three cells in each of the four
    terms; with e the bracket of :266 and d = (0.25, 0): as v, e += d; as v_0, e -= R(d) = (0, -0.25); as v_1, e += R(d) - d.
    Terms 1 and 4 (e = 0 before): 1/16 + 1/16 + 2/16 each.  Term 2 (e = (0, -0.5)): +1/16 - 3/16 + 6/16.  Term 3
    (e = (0, 0.5)): +1/16 + 5/16 - 2/16.  The sum of e^2 over all cells and terms grows by 16/16 = 1, and the loss -- that sum
    over 16 cells and 4 terms -- by 1/64: 0.125 + 0.015625."""
    F = np.zeros((1, 25, 2))
    F[0, 12, 0] = 0.25
    assert L.distortion_loss(inputs.v_src(1), F, 5) == pytest.approx(0.140625, abs=1e-15)


def test_surf_index_h_times_w_reads_the_sentinel():
    h, w = 3, 4
    xo = np.full((1, h, w), 0.25)
    yo = np.full((1, h, w), -0.5)
    surf = np.zeros((1, 2, 2, 2))
    surf[0, 1, 0] = (0, h)        # idx = 0 + h * w: the appended -1 (:364-365)
    surf[0, 1, 1] = (1, 2)        # idx = 1 + 2 w: an ordinary pixel
    surf[0, 0, 0] = (0, 0)        # normalised (-1, -1): equals the sentinel, contributes 0
    surf[0, 0, 1] = (w - 1, h - 1)   # normalised (1, 1)
    num, got = L.surf_sums(surf, xo, yo, w, h)
    assert got[0, 0].tolist() == [-1.0, -1.0] and got[0, 1].tolist() == [0.25, -0.5]
    assert num[0] == pytest.approx(0.75 ** 2 + 1.5 ** 2, abs=1e-15)
    assert L.get_surf_loss(surf, xo, yo, [2.0], w, h) == pytest.approx((0.75 ** 2 + 1.5 ** 2) / 2, abs=1e-15)


def test_loss_entries_reject_bad_arguments_with_a_status(lib):
    n = ctypes.c_size_t()
    assert lib.dvsg_loss_workspace_bytes(1, 8, 8, None) == -1
    assert lib.dvsg_loss_workspace_bytes(0, 8, 8, ctypes.byref(n)) == -1
    assert lib.dvsg_loss_workspace_bytes(2, 720, 1280, ctypes.byref(n)) == 0
    assert n.value == 2 * max(5 * 180, 1024) * 16
    assert lib.dvsg_loss_image_f32(None, 8, 8, 8, 1, 4, 4, 25, None, None, 8, 8, None, 8, 1 << 20, None) == -1
    assert b"NULL" in lib.dvsg_last_error_string()
    assert lib.dvsg_loss_image_f32(8, 8, 8, 8, 1, 4, 4, 99, None, None, 8, 8, None, 8, 1 << 20, None) == -1
    assert b"P=99" in lib.dvsg_last_error_string()
    assert lib.dvsg_loss_image_f32(8, 8, 8, 8, 1, 4, 4, 25, None, None, 8, 8, None, 8, 16, None) == -3    # workspace too small
    assert b"dvsg_loss_workspace_bytes" in lib.dvsg_last_error_string()
    assert lib.dvsg_loss_image_f32(8, 8, 8, 8, 1, 4, 4, 25, None, None, 8, 8, None, 12, 1 << 20, None) == -3   # misaligned
    assert lib.dvsg_loss_temporal_f32(8, 8, None, 8, 8, 1, 4, 4, 8, 8, None, 8, 1 << 20, None) == -1
    assert lib.dvsg_loss_temporal_f32(8, 8, 8, 8, 8, 1, 0, 4, 8, 8, None, 8, 1 << 20, None) == -1
    assert lib.dvsg_loss_masked_mse_f32(8, 8, 8, 1, 4, 4, 0, 0, 8, 8, None, 8, 1 << 20, None) == -1
    assert lib.dvsg_loss_masked_mse_f32(8, 8, 8, 1, 4, 4, 3, 0, None, 8, None, 8, 1 << 20, None) == -1
    assert lib.dvsg_loss_grid_f32(8, 8, 1, 8, 8, 8, 8, 8, None) == -1
    assert b"num_control_points=8" in lib.dvsg_last_error_string()
    assert lib.dvsg_loss_grid_f32(8, None, 1, 5, 8, 8, 8, 8, None) == -1
    assert lib.dvsg_loss_surf_f32(8, 8, 8, 8, 1, 0, 4, 4, 25, None, 8, 8, None, None) == -1
    assert lib.dvsg_loss_surf_f32(8, None, 8, 8, 1, 4, 4, 4, 25, None, 8, 8, None, None) == -1


def test_build_loss_train_refuses_cor_and_unknown_keys():
    from coupe.dvsg_amd import trainer
    with pytest.raises(NotImplementedError, match="correlationNet"):
        trainer.build_loss_train({}, {}, loss_applied=('image', 'cor'))
    with pytest.raises(KeyError):
        trainer.build_loss_train({}, {}, loss_applied=('stab',))


def test_record_score_round_trips_through_load_ckpt_dir(tmp_path):
    from coupe.dvsg_amd import weights
    d = str(tmp_path)
    for name, val in (("m_00001.npz", 1.0), ("m_00002.npz", 2.0), ("m_00003.npz", 3.0)):
        np.savez(os.path.join(d, name), **{"x:0": np.full(2, val, np.float32)})
    weights.record_score(d, "m_00001.npz", 0.5)
    weights.record_score(d, "m_00002.npz", 0.25)
    lines = weights.record_score(d, "m_00003.npz", 0.75)
    assert lines == ["m_00002.npz 0.25", "m_00001.npz 0.5", "m_00003.npz 0.75", "m_00003.npz 0.75"]
    assert open(os.path.join(d, "checkpoints")).read().splitlines() == lines
    assert weights.load_ckpt_dir(d, by_score=True)["x:0"][0] == 2.0     # the lowest loss
    assert weights.load_ckpt_dir(d, by_score=False)["x:0"][0] == 3.0    # the most recent
    lines = weights.record_score(d, "m_00001.npz", 0.125)               # re-scored: one entry, now the best and the latest
    assert lines == ["m_00001.npz 0.125", "m_00002.npz 0.25", "m_00003.npz 0.75", "m_00001.npz 0.125"]
    assert weights.load_ckpt_dir(d, by_score=True)["x:0"][0] == 1.0
    assert sorted(os.listdir(d)) == ["checkpoints", "m_00001.npz", "m_00002.npz", "m_00003.npz"]   # nothing deleted
    with pytest.raises(ValueError):
        weights.record_score(d, "m_00004.npz", float("nan"))
