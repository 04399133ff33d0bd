"""GPU: _lib.call checks a wrapper's tensors against the header's parameters and passes None through as NULL."""
import pytest
import torch

from hvpr_amd import kernels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _points(dtype=torch.float32):
    """3 points of frame 0: (batch index, x, y, z, intensity) rows."""
    return torch.tensor([[0, 1, 2, 3, 0.5], [0, 4, 5, 6, 0.5], [0, 7, 8, 9, 0.5]], dtype=dtype, device=DEV)


def test_frame_offsets_of_three_points():
    assert kernels.frame_offsets(_points(), 1).tolist() == [0, 3]


def test_wrong_dtype_is_a_type_error_naming_the_header_parameter():
    with pytest.raises(TypeError, match=r"hvpr_frame_offsets_f32: points must be torch\.float32, got torch\.float64"):
        kernels.frame_offsets(_points(torch.float64), 1)


def test_strided_view_is_a_value_error():
    wide = torch.zeros((3, 10), dtype=torch.float32, device=DEV)
    wide[:, ::2] = _points()
    view = wide[:, ::2]
    assert view.shape == (3, 5) and not view.is_contiguous()
    with pytest.raises(ValueError, match="hvpr_frame_offsets_f32: points must be contiguous"):
        kernels.frame_offsets(view, 1)
    assert kernels.frame_offsets(view.contiguous(), 1).tolist() == [0, 3]


def test_cpu_tensor_is_refused_by_name():
    with pytest.raises(RuntimeError, match=r"hvpr_frame_offsets_f32: points .*no CPU fallback"):
        kernels.frame_offsets(_points().cpu(), 1)


def test_none_reaches_the_library_as_null():
    """m_device = NULL means all M rows (include/hvpr_amd.h): the same bits as a device count of M; topk_idx = NULL is accepted."""
    g = torch.Generator().manual_seed(3)
    f = torch.randn((4, 64), generator=g).to(DEV)
    bank = kernels.PackedBank(torch.randn((2000, 64), generator=g).to(DEV))
    out = kernels.memory_readout_fwd(f, bank, 20, m_device=None)
    counted, idx = kernels.memory_readout_fwd(f, bank, 20, m_device=torch.tensor([4], dtype=torch.int32, device=DEV), want_idx=True)
    assert out.shape == (4, 64) and torch.isfinite(out).all() and torch.equal(out, counted)
    assert idx.shape == (4, 20) and idx.dtype == torch.int32
