"""The bird's-eye-view picture of a batch, made where the batch is: the reference's tools/vis.py (kitti_vis: point_to_vis_bev +
draw_box_in_bev) over csrc/bev_render.hip.

`render_bev(batch_dict, records)` takes the loader's batch (`points` with the batch column, `point_frame_offsets`) and the
`sync=False` records of `post_processing` and returns (B, H, W, 3) uint8 on the device: the height picture of the points, the
predictions outlined in their class's ink, the ground truth (when the batch has `gt_boxes`) in an ink of its own.  Nothing is
read back; the one read is the caller's, of the image it writes to disk (`write_png`).

Differences from the reference, all stated in include/hvpr_amd.h (v1):
  * heading sign: rotation_2d turns clockwise for a positive angle while a lidar heading is counter-clockwise, so the reference
    draws every box mirrored.  `heading_sign=-1` (the default here) draws it as it lies; +1 is the reference's drawing.
  * the reference outlines a box with three segments (the edge between corners 1 and 2 stays open); so does this.
  * UNPINNED: cv2.line's rasterisation (the rule here is exact in integers: 4 d^2 <= thickness^2), and the reference's stop at
    the 80 000th occupied cell (no cap here).
"""
import struct
import zlib

import numpy as np
import torch

from . import kernels

PIXEL = 0.1
THICKNESS = 2
# ink 0 is "nothing drawn"; inks 1.. are the classes in CLASS_NAMES order (repeating past the list), the last ink the ground truth
CLASS_COLOURS = ((0, 255, 0), (0, 255, 255), (255, 255, 0), (255, 128, 0), (255, 0, 255))
GT_COLOUR = (255, 64, 64)


def class_palette(num_class):
    """(num_class + 2, 3) uint8: unused ink 0, one ink per class, the ground truth's."""
    rows = [(0, 0, 0)] + [CLASS_COLOURS[i % len(CLASS_COLOURS)] for i in range(int(num_class))] + [GT_COLOUR]
    return np.array(rows, np.uint8)


class BevRenderer:
    """Keeps what a sequence of pictures shares: the view, the palette on the device and the workspace."""

    def __init__(self, point_cloud_range, num_class, pixel=PIXEL, thickness=THICKNESS, heading_sign=-1, palette=None,
                 score_thresh=None, draw_gt=True, device="cuda:0"):
        self.range = np.ascontiguousarray(point_cloud_range, np.float32).reshape(6)
        self.pixel, self.thickness, self.heading_sign = float(pixel), int(thickness), int(heading_sign)
        self.num_class, self.score_thresh, self.draw_gt = int(num_class), score_thresh, bool(draw_gt)
        pal = class_palette(num_class) if palette is None else np.ascontiguousarray(palette, np.uint8)
        if pal.ndim != 2 or pal.shape[1] != 3 or pal.shape[0] < 2:
            raise ValueError("BevRenderer: palette must be (n_ink >= 2, 3) uint8")
        self.gt_ink = pal.shape[0] - 1
        self.palette = torch.from_numpy(pal).pin_memory().to(device, non_blocking=True)
        self.workspace = None

    def tables(self, batch_dict, records):
        """The box tables of one batch: the records stacked to (B, P, ...) and, when present, `gt_boxes` (B, G, 8)."""
        tables = []
        if records:
            stack = lambda k: torch.stack([r[k] for r in records]).contiguous()            # noqa: E731
            t = {"boxes": stack("pred_boxes"), "labels": stack("pred_labels"), "ink": 0,
                 "count": torch.cat([r["pred_count"].reshape(1) for r in records]).contiguous()}
            if self.score_thresh is not None:
                t["scores"], t["thresh"] = stack("pred_scores"), float(self.score_thresh)
            tables.append(t)
        gt = batch_dict.get("gt_boxes") if self.draw_gt else None
        if gt is not None and gt.shape[1] > 0:
            # a padded row is all zeros, class 0 included: the class column serves as the score, so only real rows are drawn
            gt = gt.contiguous()
            t = {"boxes": gt, "ink": self.gt_ink}
            if gt.shape[2] >= 8:
                t["scores"], t["thresh"] = gt[:, :, 7].contiguous(), 0.5
            tables.append(t)
        return tables

    def __call__(self, batch_dict, records=None, want_counts=False):
        points = batch_dict["points"]
        off = batch_dict.get("point_frame_offsets")
        if off is None:
            raise ValueError("render_bev: the batch needs point_frame_offsets (the loader's batch has them)")
        image, counts, self.workspace = kernels.render_bev(points, off, self.range, self.pixel, self.palette,
                                                           tables=self.tables(batch_dict, records), xyz_col=1,
                                                           thickness=self.thickness, heading_sign=self.heading_sign,
                                                           want_counts=want_counts, workspace=self.workspace)
        return (image, counts) if want_counts else image


def render_bev(batch_dict, records=None, point_cloud_range=None, num_class=None, pixel=PIXEL, thickness=THICKNESS, heading_sign=-1,
               palette=None, score_thresh=None, draw_gt=True, cfg=None):
    """(B, H, W, 3) uint8 on the device.  `batch_dict`: the loader's batch; `records`: the `sync=False` records, or None for the
    points alone.  The view is `point_cloud_range` (default: the config's DATA_CONFIG.POINT_CLOUD_RANGE) at `pixel` metres; the
    palette has one ink per class and one for the ground truth.  For a sequence of batches keep a BevRenderer instead."""
    if point_cloud_range is None:
        if cfg is None:
            raise ValueError("render_bev: give point_cloud_range or cfg")
        point_cloud_range = cfg.DATA_CONFIG["POINT_CLOUD_RANGE"]
    if num_class is None:
        num_class = len(cfg.CLASS_NAMES) if cfg is not None else 1
    r = BevRenderer(point_cloud_range, num_class, pixel=pixel, thickness=thickness, heading_sign=heading_sign, palette=palette,
                    score_thresh=score_thresh, draw_gt=draw_gt, device=batch_dict["points"].device)
    return r(batch_dict, records)


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def encode_png(array, level=6):
    """The bytes of an 8-bit RGB PNG of `array` (H, W, 3) uint8: every row with filter 0, one IDAT chunk."""
    a = np.ascontiguousarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: the array must be (H >= 1, W >= 1, 3) uint8")
    H, W = a.shape[:2]
    raw = np.zeros((H, 1 + 3 * W), np.uint8)
    raw[:, 1:] = a.reshape(H, 3 * W)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b""))


def write_png(path, array):
    if torch.is_tensor(array):
        array = array.cpu().numpy()
    with open(path, "wb") as f:
        f.write(encode_png(array))
