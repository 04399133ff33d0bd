"""Test infrastructure of the BEV picture (csrc/bev_render.hip, hvpr_amd/bev_vis.py): the numpy restatement of both passes, the
integer line rule included, the edge-case generators, and a small PNG decoder.

The restatement follows tools/vis.py of the reference operation by operation and type by type (kitti_vis, :279-286):
  height pass   _points_to_bevmap_reverse_kernel :9-60 under points_to_bev :63-106 and point_to_vis_bev :109-121, one height slice;
  box pass      center_to_corner_box2d :201-221 (corners_nd :153-184, rotation_2d :186-199) and draw_box_in_bev :234-246;
  line rule     the project's own (cv2.line is not pinned): 4 d^2 <= t^2 in integers.
It is checked against the reference's own run in tests/test_bev_vis_host.py (fixture G24) and is what the GPU tests compare the op
with, byte for byte."""
import struct
import zlib

import numpy as np

CLAMP = 8191
MARGIN = 1e-2          # px: how far every scaled corner coordinate of a generated box stays from an integer (float64)
F32 = np.float32


def grid_of(rng, pixel):
    """(H, W): round((hi - lo) / pixel) in float32."""
    r = np.asarray(rng, F32)
    g = np.round((r[3:5] - r[:2]) / F32(pixel)).astype(np.int64)
    return int(g[1]), int(g[0])


def height_pass(xyz, rng, pixel):
    """(height (H, W) float32, counts (H, W) int32) of one frame's points (n, 3) float32."""
    r = np.asarray(rng, F32)
    H, W = grid_of(r, pixel)
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    size = np.array([pixel, pixel, r[5] - r[2]], F32)
    grid = np.array([W, H, np.round((r[5] - r[2]) / size[2])], F32)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((xyz - r[:3]) / size)                                # float32 throughout
        keep = ((c >= 0) & (c < grid)).all(axis=1)                        # a NaN fails both
    c, z = c[keep].astype(np.int64), xyz[keep, 2]
    h = ((z.astype(np.float64) - np.float64(r[2])) / np.float64(size[2])).astype(F32)
    height, counts = np.zeros((H, W), F32), np.zeros((H, W), np.int32)
    np.maximum.at(height, (c[:, 1], c[:, 0]), h)
    np.add.at(counts, (c[:, 1], c[:, 0]), 1)
    return height, counts


def grey_of(height):
    g = np.asarray(height, F32) * F32(255.0)
    return np.minimum(g, F32(255.0)).astype(np.uint8)


def _corners32(boxes, sign):
    """(n, 4, 2) float32: corners plus centre, before the view transform."""
    b = np.asarray(boxes, F32)
    a = b[:, 6] if sign > 0 else -b[:, 6]
    sn, cs = np.sin(a).astype(F32), np.cos(a).astype(F32)
    nx, ny = np.array([-0.5, -0.5, 0.5, 0.5], F32), np.array([-0.5, 0.5, 0.5, -0.5], F32)
    x, y = b[:, 3:4] * nx, b[:, 4:5] * ny
    rx = x * cs[:, None] + y * sn[:, None]
    ry = x * -sn[:, None] + y * cs[:, None]
    return np.stack([rx + b[:, 0:1], ry + b[:, 1:2]], axis=2)


def box_segments(boxes, rng, pixel, sign=1):
    """(segments (n, 3, 4) int32 [ax, ay, bx, by], drawn (n,) bool): the three segments of every box, clamped; `drawn` is False for
    a box with a non-finite field or corner."""
    r = np.asarray(rng, F32)
    H, W = grid_of(r, pixel)
    b = np.asarray(boxes, F32)[:, :7].reshape(-1, 7)
    drawn = np.isfinite(b).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        c = _corners32(np.where(drawn[:, None], b, F32(0)), sign)
        scale = np.array([W, H], np.float64) / (r[3:5].astype(np.float64) - r[:2].astype(np.float64))
        t = (c.astype(np.float64) - r[:2].astype(np.float64)).astype(F32)
        s = (t.astype(np.float64) * scale).astype(F32)
    drawn &= ~np.isnan(s).any(axis=(1, 2))
    s = np.where(np.isnan(s), F32(0), s)
    q = np.where(s >= CLAMP, CLAMP, np.where(s <= -CLAMP, -CLAMP, np.trunc(np.clip(s, -CLAMP, CLAMP)))).astype(np.int32)
    seg = np.concatenate([q[:, [0, 2, 3]], q[:, [1, 3, 0]]], axis=2)
    return seg, drawn


def corner_margin(boxes, rng, pixel, sign=1):
    """Per box the smallest distance (px) of a scaled corner coordinate, computed in float64, from an integer; coordinates beyond
    the clamp do not count."""
    r = np.asarray(rng, np.float64)
    H, W = grid_of(rng, pixel)
    b = np.asarray(boxes, np.float64)[:, :7].reshape(-1, 7)
    a = b[:, 6] * (1.0 if sign > 0 else -1.0)
    nx, ny = np.array([-0.5, -0.5, 0.5, 0.5]), np.array([-0.5, 0.5, 0.5, -0.5])
    x, y = b[:, 3:4] * nx, b[:, 4:5] * ny
    sx = (x * np.cos(a)[:, None] + y * np.sin(a)[:, None] + b[:, 0:1] - r[0]) * (W / (r[3] - r[0]))
    sy = (-x * np.sin(a)[:, None] + y * np.cos(a)[:, None] + b[:, 1:2] - r[1]) * (H / (r[4] - r[1]))
    s = np.concatenate([sx, sy], axis=1)
    d = np.abs(s - np.round(s))
    d = np.where(np.abs(s) > CLAMP - 1, 1.0, d)
    return d.min(axis=1)


def settle_boxes(boxes, rng, pixel, gen, signs=(1, -1)):
    """The boxes with the centres of those too close to a pixel boundary nudged (by under a pixel) until every corner keeps MARGIN
    under both heading signs: the device's float32 sin / cos may differ from numpy's in the last bit, and truncation would turn
    that into a pixel.  Non-finite boxes are left alone."""
    b = np.array(boxes, F32)
    for i in range(len(b)):
        if not np.isfinite(b[i, :7]).all():
            continue
        for _ in range(1000):
            if all(corner_margin(b[i:i + 1], rng, pixel, s)[0] >= MARGIN for s in signs):
                break
            b[i, :2] += gen.uniform(-0.7, 0.7, 2).astype(F32) * F32(pixel)
        else:
            raise AssertionError("settle_boxes: no placement found")
    return b


def draw_segment(ink_plane, seg, ink, thickness):
    """ink_plane (H, W) uint32, in place: max with `ink` wherever 4 d^2 <= t^2 for the integer segment (ax, ay, bx, by)."""
    H, W = ink_plane.shape
    ax, ay, bx, by = (int(v) for v in seg)
    rad, tt = thickness // 2, thickness * thickness
    x0, x1 = max(0, min(ax, bx) - rad), min(W - 1, max(ax, bx) + rad)
    y0, y1 = max(0, min(ay, by) - rad), min(H - 1, max(ay, by) + rad)
    if x0 > x1 or y0 > y1:
        return
    py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    abx, aby, apx, apy = bx - ax, by - ay, px - ax, py - ay
    L, u = abx * abx + aby * aby, apx * abx + apy * aby
    cr = apx * aby - apy * abx
    on = np.where((u <= 0) | (L == 0), 4 * (apx * apx + apy * apy) <= tt,
                  np.where(u >= L, 4 * ((px - bx) ** 2 + (py - by) ** 2) <= tt, 4 * cr * cr <= tt * L))
    view = ink_plane[y0:y1 + 1, x0:x1 + 1]
    view[on] = np.maximum(view[on], np.uint32(ink))


def table_rows(table, n_ink):
    """(boxes, inks) of the rows of one frame's table that may be drawn.  table: dict with boxes (P, >= 7) and optionally count,
    scores + thresh, labels, ink."""
    boxes = np.asarray(table["boxes"], F32)
    P = len(boxes)
    on = np.ones((P,), bool)
    if table.get("count") is not None:
        on &= np.arange(P) < int(table["count"])
    if table.get("scores") is not None:
        with np.errstate(invalid="ignore"):
            on &= np.asarray(table["scores"], F32) >= F32(table.get("thresh", 0.0))
    ink = np.full((P,), int(table.get("ink", 1)), np.int64)
    if table.get("labels") is not None:
        ink = ink + np.asarray(table["labels"], np.int64)
    on &= (ink >= 1) & (ink < n_ink)
    return boxes[on], ink[on]


def render_frame(xyz, rng, pixel, tables, palette, thickness=2, sign=-1):
    """(image (H, W, 3) uint8, counts (H, W) int32) of one frame."""
    height, counts = height_pass(xyz, rng, pixel)
    ink_plane = np.zeros(height.shape, np.uint32)
    palette = np.asarray(palette, np.uint8)
    for t in tables:
        boxes, inks = table_rows(t, len(palette))
        seg, drawn = box_segments(boxes, rng, pixel, sign)
        for k in np.nonzero(drawn)[0]:
            for s in seg[k]:
                draw_segment(ink_plane, s, inks[k], thickness)
    image = np.repeat(grey_of(height)[:, :, None], 3, axis=2)
    image[ink_plane > 0] = palette[ink_plane[ink_plane > 0]]
    return image, counts


def render_batch(points, offsets, xyz_col, rng, pixel, tables, palette, thickness=2, sign=-1):
    """The op's outputs for a ragged batch: tables are batch-shaped dicts (boxes (B, P, S), count (B,), scores / labels (B, P))."""
    offsets = np.asarray(offsets)
    images, counts = [], []
    for b in range(len(offsets) - 1):
        per = [{k: (v[b] if k in ("boxes", "count", "scores", "labels") and v is not None else v) for k, v in t.items()} for t in tables]
        xyz = np.asarray(points)[offsets[b]:offsets[b + 1], xyz_col:xyz_col + 3]
        im, ct = render_frame(xyz, rng, pixel, per, palette, thickness, sign)
        images.append(im)
        counts.append(ct)
    return np.stack(images), np.stack(counts)


# ------------------------------------------------------------------------------------------------ generators
def frame_points(gen, n, rng, spread=1.0):
    """n rows (x, y, z, r) float32, a little wider than the view on every axis."""
    r = np.asarray(rng, np.float64)
    ext = r[3:] - r[:3]
    p = np.empty((n, 4), F32)
    for j in range(3):
        p[:, j] = gen.uniform(r[j] - 0.1 * ext[j], r[j + 3] + 0.1 * ext[j], n) * spread
    p[:, 3] = gen.uniform(0, 1, n)
    return p


def random_boxes(gen, n, rng, pixel):
    """n lidar boxes (x, y, z, dx, dy, dz, heading) float32 with centres inside the view, settled."""
    r = np.asarray(rng, np.float64)
    b = np.empty((n, 7), F32)
    b[:, 0] = gen.uniform(r[0], r[3], n)
    b[:, 1] = gen.uniform(r[1], r[4], n)
    b[:, 2] = gen.uniform(r[2], r[5], n)
    b[:, 3] = gen.uniform(6, 25, n) * pixel
    b[:, 4] = gen.uniform(3, 12, n) * pixel
    b[:, 5] = 1.5
    b[:, 6] = gen.uniform(-np.pi, np.pi, n)
    return settle_boxes(b, rng, pixel, gen)


# ------------------------------------------------------------------------------------------------ a PNG decoder for the tests
def decode_png(data):
    """(H, W, 3) uint8 of an 8-bit RGB, non-interlaced PNG whose rows all use filter 0; every chunk's CRC is checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head, seen_end = 8, b"", None, False
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(kind + body) & 0xffffffff), kind
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            seen_end = True
        pos += 12 + n
    assert seen_end and head is not None
    W, H, depth, colour, comp, filt, lace = head
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 3).copy()
