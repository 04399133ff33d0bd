"""From a KITTI directory to info records and frames: the reference's KittiDataset up to the FOV filter
(pcdet/datasets/kitti/kitti_dataset.py:12-191, 340-378) and create_kitti_infos (:386-423), written from its behaviour.

  read_calib / read_label / read_road_plane / read_image_shape / read_split    the file readers (host).
  KittiDataset.get_infos       the reference's list of info dicts: same keys, key order, shapes and dtypes (fixture G23 records
                               every one).  num_points_in_gt comes from the device: a chunk of frames per library call
                               (csrc/kitti_infos.hip), one pinned staging buffer and one upload, the count call, ONE host read of
                               the chunk's counts (`reads` counts them).
  KittiDataset.frame(index)    the dict DeviceBatchLoader takes as `frame_source(index)`: __getitem__ up to the FOV filter, which is
                               the loader's.
  create_kitti_infos           the four pickles, then the train database through gt_database.create_groundtruth_database.
  python -m hvpr_amd.kitti_dataset create_kitti_infos <dataset yaml> [data_path]

Two rounding paths, kept apart as the reference keeps them: the infos' `gt_boxes_lidar` is float64 around centres that went through
a float32 inverse (:160-167); a frame's `gt_boxes` is float32 throughout, from the float32 camera boxes (:364-375).

Unpinned against the reference: a point on a box face (Qhull's tolerance there, `<=` / `<` of csrc/box_cut.h here), a degenerate
box (counts 0 here; the reference's `except` names a scipy module that no longer exists), and get_image_shape, which reads the
PNG header here and decodes the image through skimage there.
"""
import os
import pickle
import struct
from pathlib import Path

import numpy as np
import torch

from .calibration import rect_to_lidar
from .config import _get
from .gt_database import CountReader, StagedChunk
from .preprocess import PinnedBuffer, to_device

DEFAULT_SPLIT = {"train": "train", "test": "val"}
DEFAULT_INFO_PATH = {"train": ["kitti_infos_train.pkl"], "test": ["kitti_infos_val.pkl"]}


# ------------------------------------------------------------------------------------------------ file readers
def read_calib(path):
    """{'P2', 'P3' (3, 4), 'R0' (3, 3), 'Tr_velo2cam' (3, 4)} float32: lines 2-5 of the file, the words behind the key."""
    with open(path) as f:
        lines = f.readlines()
    row = [np.array(lines[i].strip().split(" ")[1:], dtype=np.float32) for i in (2, 3, 4, 5)]
    return {"P2": row[0].reshape(3, 4), "P3": row[1].reshape(3, 4), "R0": row[2].reshape(3, 3), "Tr_velo2cam": row[3].reshape(3, 4)}


def _level(bbox, truncation, occlusion):
    """The difficulty rule of object3d_kitti.py:38-52: 0 easy, 1 moderate, 2 hard, -1 none of them."""
    height = float(bbox[3]) - float(bbox[1]) + 1
    for level, (min_height, max_trunc, max_occ) in enumerate(((40, 0.15, 0), (25, 0.3, 1), (25, 0.5, 2))):
        if height >= min_height and truncation <= max_trunc and occlusion <= max_occ:
            return level
    return -1


def read_label(path):
    """One dict per line with the fields of object3d_kitti.py:18-52: name, truncated, occluded, alpha, bbox (4,) float32, h, w, l,
    location (3,) float32, rotation_y, score (-1.0 without a 16th field), level."""
    objects = []
    with open(path) as f:
        for line in f.readlines():
            w = line.strip().split(" ")
            o = {"name": w[0], "truncated": float(w[1]), "occluded": float(w[2]), "alpha": float(w[3]),
                 "bbox": np.array([float(v) for v in w[4:8]], dtype=np.float32), "h": float(w[8]), "w": float(w[9]), "l": float(w[10]),
                 "location": np.array([float(v) for v in w[11:14]], dtype=np.float32), "rotation_y": float(w[14]),
                 "score": float(w[15]) if len(w) == 16 else -1.0}
            o["level"] = _level(o["bbox"], o["truncated"], o["occluded"])
            objects.append(o)
    return objects


def read_road_plane(path):
    """(4,) float64: line 4, turned so that the normal points up (rect camera frame: y down), divided by the normal's length."""
    with open(path) as f:
        lines = f.readlines()
    plane = np.asarray([float(v) for v in lines[3].split()])
    if plane[1] > 0:
        plane = -plane
    return plane / np.linalg.norm(plane[0:3])


def read_image_shape(path):
    """(h, w) int32 from the PNG's IHDR chunk: no image library is needed."""
    with open(path, "rb") as f:
        head = f.read(24)
    if len(head) < 24 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"{path}: not a PNG file")
    w, h = struct.unpack(">II", head[16:24])
    return np.array([h, w], dtype=np.int32)


def read_split(root_path, split):
    """The sample ids of ImageSets/<split>.txt, or None without the file."""
    p = Path(root_path) / "ImageSets" / (split + ".txt")
    if not p.exists():
        return None
    with open(p) as f:
        return [x.strip() for x in f.readlines()]


# ------------------------------------------------------------------------------------------------ geometry (host, per box)
def boxes3d_kitti_camera_to_lidar(boxes3d_camera, calib):
    """box_utils.py:91-105: (N, 7) camera boxes [x, y, z, l, h, w, r] to lidar boxes, in the dtype the input has."""
    l, h, w, r = (boxes3d_camera[:, i: i + 1] for i in (3, 4, 5, 6))
    xyz = rect_to_lidar(boxes3d_camera[:, 0:3], calib)
    xyz[:, 2] += h[:, 0] / 2
    return np.concatenate([xyz, l, w, h, -(r + np.pi / 2)], axis=-1)


def _annotations(objects, calib):
    """The `annos` dict of get_infos (:143-167) without num_points_in_gt, and the number of real (not DontCare) objects."""
    a = {}
    a["name"] = np.array([o["name"] for o in objects])
    a["truncated"] = np.array([o["truncated"] for o in objects])
    a["occluded"] = np.array([o["occluded"] for o in objects])
    a["alpha"] = np.array([o["alpha"] for o in objects])
    a["bbox"] = np.concatenate([o["bbox"].reshape(1, 4) for o in objects], axis=0)
    a["dimensions"] = np.array([[o["l"], o["h"], o["w"]] for o in objects])                  # lhw, float64
    a["location"] = np.concatenate([o["location"].reshape(1, 3) for o in objects], axis=0)   # float32
    a["rotation_y"] = np.array([o["rotation_y"] for o in objects])
    a["score"] = np.array([o["score"] for o in objects])
    a["difficulty"] = np.array([o["level"] for o in objects], np.int32)
    num_objects, num_gt = sum(o["name"] != "DontCare" for o in objects), len(objects)
    a["index"] = np.array(list(range(num_objects)) + [-1] * (num_gt - num_objects), dtype=np.int32)
    dims, rots = a["dimensions"][:num_objects], a["rotation_y"][:num_objects]
    loc_lidar = rect_to_lidar(a["location"][:num_objects], calib)                            # float32
    loc_lidar[:, 2] += dims[:, 1] / 2                                                        # rounded to float32 once
    a["gt_boxes_lidar"] = np.concatenate([loc_lidar, dims[:, 0:1], dims[:, 2:3], dims[:, 1:2], -(np.pi / 2 + rots[..., np.newaxis])],
                                         axis=1)
    return a, num_objects


def _calib_info(calib):
    """The `calib` dict of get_infos (:132-137): P2 and Tr_velo_to_cam become float64, R0_rect stays float32."""
    last = np.array([[0., 0., 0., 1.]])
    R0 = np.zeros([4, 4], dtype=calib["R0"].dtype)
    R0[3, 3] = 1.
    R0[:3, :3] = calib["R0"]
    return {"P2": np.concatenate([calib["P2"], last], axis=0), "R0_rect": R0,
            "Tr_velo_to_cam": np.concatenate([calib["Tr_velo2cam"], last], axis=0)}


# ------------------------------------------------------------------------------------------------ the counts of a chunk
class InfoCounter:
    """get_infos' count path on its own: `count(points_list, boxes_list, calibs, image_shapes)` -> per frame an (n_i,) int32 array
    of the points in the camera's view and inside each box.  points (N_i, F) on the host or the device, boxes (n_i, 7+) lidar boxes
    (rounded to float32 as the reference's corners are), calibs dicts of Tr_velo2cam / R0 / P2.  One upload, one count call and one
    host read per chunk of `frames_per_call` frames; a chunk without boxes is not read.  `reads` counts the reads."""

    def __init__(self, device="cuda:0", frames_per_call=32):
        self.device, self.frames_per_call = torch.device(device), max(1, int(frames_per_call))
        self._stage, self._ws, self._read = PinnedBuffer(torch.uint8, 1 << 16), None, CountReader()

    @property
    def reads(self):
        return self._read.reads

    def count(self, points_list, boxes_list, calibs, image_shapes):
        out = []
        for c0 in range(0, len(points_list), self.frames_per_call):
            c1 = c0 + self.frames_per_call
            boxes = [np.asarray(b).reshape(-1, 7) if np.asarray(b).size == 0 else np.asarray(b) for b in boxes_list[c0:c1]]
            chunk = StagedChunk(points_list[c0:c1], boxes, self.device, self._stage, calibs=calibs[c0:c1], image_shapes=image_shapes[c0:c1])
            if chunk.n_obj == 0:
                out.extend(np.zeros((0,), np.int32) for _ in chunk.n_box)
                continue
            counts_dev, _, self._ws = chunk.count(self._ws)
            counts = self._read(counts_dev).numpy()
            off = chunk.box_off_host.numpy()
            out.extend(counts[off[f]: off[f + 1]].copy() for f in range(len(chunk.n_box)))
        return out


# ------------------------------------------------------------------------------------------------ the dataset
class KittiDataset:
    """dataset_cfg: the DATA_CONFIG block; DATA_SPLIT and INFO_PATH default to the reference's kitti_dataset.yaml (train / val,
    kitti_infos_train.pkl / kitti_infos_val.pkl)."""

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, device="cuda:0"):
        self.dataset_cfg, self.class_names, self.training = dataset_cfg, list(class_names), bool(training)
        self.mode = "train" if self.training else "test"
        self.root_path = Path(root_path if root_path is not None else dataset_cfg["DATA_PATH"])
        self.device = torch.device(device)
        self.reads = 0
        self.set_split(_get(dataset_cfg, "DATA_SPLIT", DEFAULT_SPLIT)[self.mode])
        self.kitti_infos = []
        self.include_kitti_data(self.mode)
        if all(k in dataset_cfg for k in ("POINT_CLOUD_RANGE", "POINT_FEATURE_ENCODING", "DATA_PROCESSOR")):
            from .detector import set_model_attributes       # what build_network(cfg.MODEL, n, dataset=self) reads
            set_model_attributes(self, dataset_cfg)

    def include_kitti_data(self, mode):
        for info_path in _get(self.dataset_cfg, "INFO_PATH", DEFAULT_INFO_PATH)[mode]:
            info_path = self.root_path / info_path
            if not info_path.exists():
                continue
            with open(info_path, "rb") as f:
                self.kitti_infos.extend(pickle.load(f))

    def set_split(self, split):
        self.split = split
        self.root_split_path = self.root_path / ("training" if split != "test" else "testing")
        self.sample_id_list = read_split(self.root_path, split)

    def __len__(self):
        return len(self.kitti_infos)

    def _file(self, folder, idx, suffix):
        p = self.root_split_path / folder / ("%s.%s" % (idx, suffix))
        if not p.exists():
            raise FileNotFoundError(str(p))
        return p

    def get_lidar(self, idx):
        return np.fromfile(str(self._file("velodyne", idx, "bin")), dtype=np.float32).reshape(-1, 4)

    def get_image_shape(self, idx):
        return read_image_shape(self._file("image_2", idx, "png"))

    def get_label(self, idx):
        return read_label(self._file("label_2", idx, "txt"))

    def get_calib(self, idx):
        return read_calib(self._file("calib", idx, "txt"))

    def get_road_plane(self, idx):
        p = self.root_split_path / "planes" / ("%s.txt" % idx)
        return read_road_plane(p) if p.exists() else None

    # -------------------------------------------------------------------------------------------- infos
    def _host_info(self, sample_idx, has_label):
        """One info without num_points_in_gt -> (info, calib, number of real objects)."""
        info = {"point_cloud": {"num_features": 4, "lidar_idx": sample_idx},
                "image": {"image_idx": sample_idx, "image_shape": self.get_image_shape(sample_idx)}}
        calib = self.get_calib(sample_idx)
        info["calib"] = _calib_info(calib)
        num_objects = 0
        if has_label:
            info["annos"], num_objects = _annotations(self.get_label(sample_idx), calib)
        return info, calib, num_objects

    def get_infos(self, has_label=True, count_inside_pts=True, sample_id_list=None, frames_per_call=32):
        sample_id_list = sample_id_list if sample_id_list is not None else self.sample_id_list
        counter = InfoCounter(self.device, frames_per_call) if has_label and count_inside_pts else None
        infos = []
        step = max(1, int(frames_per_call))
        for c0 in range(0, len(sample_id_list), step):
            ids = sample_id_list[c0: c0 + step]
            chunk = [self._host_info(i, has_label) for i in ids]
            if counter is not None:
                counts = counter.count([self.get_lidar(i) for i in ids], [c[0]["annos"]["gt_boxes_lidar"] for c in chunk],
                                       [c[1] for c in chunk], [c[0]["image"]["image_shape"] for c in chunk])
                for (info, _, num_objects), n in zip(chunk, counts):
                    num_points_in_gt = -np.ones(len(info["annos"]["name"]), dtype=np.int32)
                    num_points_in_gt[:num_objects] = n
                    info["annos"]["num_points_in_gt"] = num_points_in_gt
            infos.extend(c[0] for c in chunk)
        if counter is not None:
            self.reads += counter.reads
        return infos

    # -------------------------------------------------------------------------------------------- frames
    def frame(self, index):
        """What __getitem__ holds before the FOV filter (:345-378), as DeviceBatchLoader's `frame_source` serves it."""
        info = self.kitti_infos[index]
        sample_idx = info["point_cloud"]["lidar_idx"]
        calib = self.get_calib(sample_idx)
        out = {"points": to_device(self.get_lidar(sample_idx), self.device), "frame_id": sample_idx, "calib": calib,
               "image_shape": info["image"]["image_shape"]}
        if "annos" in info:
            annos = info["annos"]
            keep = [i for i, n in enumerate(annos["name"]) if n != "DontCare"]
            camera = np.concatenate([annos["location"][keep], annos["dimensions"][keep], annos["rotation_y"][keep][..., np.newaxis]],
                                    axis=1).astype(np.float32)
            out["gt_names"], out["gt_boxes"] = annos["name"][keep], boxes3d_kitti_camera_to_lidar(camera, calib)
            road_plane = self.get_road_plane(sample_idx)
            if road_plane is not None:
                out["road_plane"] = road_plane
        return out

    def evaluation(self, det_annos, class_names):
        if "annos" not in self.kitti_infos[0].keys():
            return None, {}
        import copy
        from . import kitti_eval_device
        return kitti_eval_device.get_official_eval_result([copy.deepcopy(info["annos"]) for info in self.kitti_infos],
                                                          copy.deepcopy(det_annos), class_names)


def create_kitti_infos(dataset_cfg, class_names, data_path, save_path, device="cuda:0", frames_per_call=32):
    """kitti_infos_{train,val,trainval,test}.pkl under `save_path` (the test split without labels and counts), then the train
    database (gt_database/ and kitti_dbinfos_train.pkl under `data_path`).  Returns the dataset."""
    from . import gt_database
    data_path, save_path = Path(data_path), Path(save_path)
    dataset = KittiDataset(dataset_cfg, class_names, training=False, root_path=data_path, device=device)
    infos = {}
    for split in ("train", "val"):
        dataset.set_split(split)
        infos[split] = dataset.get_infos(has_label=True, count_inside_pts=True, frames_per_call=frames_per_call)
    infos["trainval"] = infos["train"] + infos["val"]
    dataset.set_split("test")
    infos["test"] = dataset.get_infos(has_label=False, count_inside_pts=False, frames_per_call=frames_per_call)
    for split in ("train", "val", "trainval", "test"):
        with open(save_path / ("kitti_infos_%s.pkl" % split), "wb") as f:
            pickle.dump(infos[split], f)
    dataset.set_split("train")
    gt_database.create_groundtruth_database(data_path, save_path / "kitti_infos_train.pkl", dataset.get_lidar, split="train",
                                            device=device, frames_per_call=frames_per_call)
    return dataset


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 2 and sys.argv[1] == "create_kitti_infos":
        from .config import cfg_from_yaml_file
        cfg = cfg_from_yaml_file(sys.argv[2])
        root = Path(sys.argv[3]) if len(sys.argv) > 3 else Path(os.path.dirname(os.path.abspath(__file__))).parent / "data" / "kitti"
        create_kitti_infos(cfg, ["Car", "Pedestrian", "Cyclist"], root, root)
    else:
        print("usage: python -m hvpr_amd.kitti_dataset create_kitti_infos <dataset yaml> [data_path]")
