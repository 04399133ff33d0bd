"""A frame's calibration, once: the reference's Calibration (pcdet/utils/calibration_kitti.py) as functions over the matrices.

A calibration is a dict of Tr_velo2cam (3, 4) / R0 (3, 3) / P2 (3, 4), as kitti_dataset.read_calib gives it, or the reference's
Calibration object (V2C / R0 / P2).  Everything that forms the lidar-to-rect product takes it from `lidar_to_rect_matrix`:

  lidar_to_rect / rect_to_lidar   the point transforms (:50-73), in the dtype of the matrices as given.
  fov_matrices                    the float32 pair get_fov_flag's kernel reads.
  pack_calib                      the (B, 26) float32 table the library's calls take (CALIB_WORDS words per frame).
"""
import numpy as np
import torch

CALIB_WORDS = 26


def parts(calib):
    """(V2C, R0, P2) of a dict or of the reference's Calibration object."""
    if isinstance(calib, dict):
        return calib["Tr_velo2cam"], calib["R0"], calib["P2"]
    return calib.V2C, calib.R0, calib.P2


def as_dict(calib):
    """The dict form (what the augment planner takes); None stays None."""
    if calib is None or isinstance(calib, dict):
        return calib
    V2C, R0, P2 = parts(calib)
    return {"Tr_velo2cam": V2C, "R0": R0, "P2": P2}


def lidar_to_rect_matrix(V2C, R0):
    """(4, 3): the product of calibration_kitti.py:71, in the dtype numpy gives it for these two matrices."""
    return np.dot(V2C.T, R0.T)


def _hom(points):
    return np.hstack((points, np.ones((points.shape[0], 1), dtype=np.float32)))


def lidar_to_rect(points, calib):
    """calibration_kitti.py:65-73: (N, 3) lidar points -> rect camera points."""
    V2C, R0, _ = parts(calib)
    return np.dot(_hom(points), lidar_to_rect_matrix(V2C, R0))


def rect_to_lidar(points, calib):
    """calibration_kitti.py:50-63: (N, 3) rect camera points -> lidar points, through the 4 x 4 inverse."""
    V2C, R0, _ = parts(calib)
    R0_ext = np.hstack((R0, np.zeros((3, 1), dtype=np.float32)))
    R0_ext = np.vstack((R0_ext, np.zeros((1, 4), dtype=np.float32)))
    R0_ext[3, 3] = 1
    V2C_ext = np.vstack((V2C, np.zeros((1, 4), dtype=np.float32)))
    V2C_ext[3, 3] = 1
    return np.dot(_hom(points), np.linalg.inv(np.dot(R0_ext, V2C_ext).T))[:, 0:3]


def _f32_parts(calib):
    return tuple(np.asarray(m, np.float32) for m in parts(calib))


def fov_matrices(calib, device):
    """The lidar-to-rect product and P2^T as the reference forms them (float32 numpy products), on the device."""
    V2C, R0, P2 = _f32_parts(calib)
    a = np.ascontiguousarray(lidar_to_rect_matrix(V2C, R0).astype(np.float32))
    p = np.ascontiguousarray(P2.T.astype(np.float32))
    return torch.from_numpy(a).to(device), torch.from_numpy(p).to(device)


def pack_calib(calibs, image_shapes):
    """(B, 26) float32, one row per frame: the 4 x 3 lidar-to-rect product formed in float32 (row-major), P2 (3 x 4, row-major),
    image height, image width."""
    out = np.zeros((len(calibs), CALIB_WORDS), np.float32)
    for i, (c, shape) in enumerate(zip(calibs, image_shapes)):
        V2C, R0, P2 = _f32_parts(c)
        out[i, 0:12] = lidar_to_rect_matrix(V2C, R0).astype(np.float32).reshape(-1)
        out[i, 12:24] = P2.reshape(-1)
        out[i, 24], out[i, 25] = float(shape[0]), float(shape[1])
    return out
