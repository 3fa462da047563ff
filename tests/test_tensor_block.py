"""Host side of the device-resident load (Optimizer.load_tensors): how a torch
tensor becomes one strided block of ipmz_qp_device_data.  No GPU: CPU tensors
have a data_ptr and strides too, and _tensor_block looks at nothing else."""
import pytest
import torch

import ipmz_amd as I

B, ROWS, COLS = 3, 5, 12


def test_batched_matrix():
    t = torch.zeros((B, ROWS, COLS), dtype=torch.float64)
    assert I._tensor_block(t, B, ROWS, COLS) == (t.data_ptr(), COLS, ROWS * COLS)


def test_shared_matrix_has_qp_stride_zero():
    t = torch.zeros((ROWS, COLS), dtype=torch.float64)
    assert I._tensor_block(t, B, ROWS, COLS) == (t.data_ptr(), COLS, 0)


def test_batched_vector():
    t = torch.zeros((B, COLS), dtype=torch.float64)
    ptr, _, sq = I._tensor_block(t, B, None, COLS)
    assert (ptr, sq) == (t.data_ptr(), COLS)


def test_shared_vector_has_qp_stride_zero():
    t = torch.zeros(COLS, dtype=torch.float64)
    ptr, _, sq = I._tensor_block(t, B, None, COLS)
    assert (ptr, sq) == (t.data_ptr(), 0)


def test_row_strided_view_is_not_copied():
    big = torch.zeros((B, ROWS + 2, COLS + 7), dtype=torch.float64)
    v = big[:, :ROWS, :COLS]
    assert not v.is_contiguous()
    assert I._tensor_block(v, B, ROWS, COLS) == (big.data_ptr(), COLS + 7, (ROWS + 2) * (COLS + 7))
    w = big[:, 1:ROWS + 1, 1:COLS + 1]  # the pointer moves with the view: 8-byte aligned only
    assert I._tensor_block(w, B, ROWS, COLS) == (big.data_ptr() + 8 * (COLS + 7 + 1), COLS + 7, (ROWS + 2) * (COLS + 7))
    u = torch.zeros((B, COLS + 3), dtype=torch.float64)[:, 1:COLS + 1]
    ptr, _, sq = I._tensor_block(u, B, None, COLS)
    assert (ptr, sq) == (u.data_ptr(), COLS + 3)


def test_expanded_shared_matrix_has_qp_stride_zero():
    t = torch.zeros((ROWS, COLS), dtype=torch.float64)
    e = t.unsqueeze(0).expand(B, ROWS, COLS)
    assert e.stride(0) == 0
    assert I._tensor_block(e, B, ROWS, COLS) == (t.data_ptr(), COLS, 0)
    v = torch.zeros(COLS, dtype=torch.float64)
    ptr, _, sq = I._tensor_block(v.expand(B, COLS), B, None, COLS)
    assert (ptr, sq) == (v.data_ptr(), 0)


def test_rejects_other_dtypes():
    with pytest.raises(ValueError, match="float64"):
        I._tensor_block(torch.zeros((B, ROWS, COLS), dtype=torch.float32), B, ROWS, COLS)
    with pytest.raises(ValueError, match="float64"):
        I._tensor_block(torch.zeros(COLS, dtype=torch.int64), B, None, COLS)


def test_rejects_wrong_shapes():
    for shape in [(B, ROWS, COLS + 1), (B + 1, ROWS, COLS), (ROWS + 1, COLS), (COLS,), (B, COLS)]:
        with pytest.raises(ValueError, match="shape"):
            I._tensor_block(torch.zeros(shape, dtype=torch.float64), B, ROWS, COLS)
    for shape in [(B, COLS + 1), (COLS - 1,), (B, ROWS, COLS)]:
        with pytest.raises(ValueError, match="shape"):
            I._tensor_block(torch.zeros(shape, dtype=torch.float64), B, None, COLS)


def test_rejects_inner_stride():
    t = torch.zeros((B, COLS, ROWS), dtype=torch.float64).transpose(1, 2)  # (B, ROWS, COLS), columns ROWS apart
    with pytest.raises(ValueError, match="inner stride"):
        I._tensor_block(t, B, ROWS, COLS)
    v = torch.zeros((B, 2 * COLS), dtype=torch.float64)[:, ::2]
    with pytest.raises(ValueError, match="inner stride"):
        I._tensor_block(v, B, None, COLS)


def test_exports_list_the_device_entry_points():
    names = sorted(I.EXPORTS)
    assert "ipmz_batch_load_device" in names and "ipmz_batch_copy_state" in names
    assert hasattr(I.lib, "ipmz_batch_load_device") and hasattr(I.lib, "ipmz_batch_copy_state")
