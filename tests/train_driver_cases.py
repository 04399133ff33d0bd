"""A tiny KITTI tree with a train and a val split and a model config for it: what the epoch loader, the training loop and the two
commands are tested on.  Frames are kitti_infos_cases.labelled_frames (8 boxes a frame: two Cars with some tens of points each, so
the GT sampler's PREPARE filter leaves a bank)."""
import os
import warnings

import numpy as np
import yaml

import kitti_infos_cases as K

N_TRAIN, N_VAL, POINTS, BOXES = 6, 4, 8000, 8
NUM_POINTS = 4096                  # sample_points: the first set-abstraction level takes 4096 centres, a frame keeps >= 2048 rows


def plain(o):
    if isinstance(o, dict):
        return {k: plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    if isinstance(o, np.generic):
        return o.item()
    return o


def model_cfg(gt_sampling=True, multi_class_nms=False):
    """hvpr_car with the three-class augmentor block (with CLASS_NAMES ['Car'] it samples Car:15) and NUM_POINTS for the tiny frames."""
    from hvpr_amd import config
    cfg = config.hvpr_car_cfg()
    aug = config.cfg_from_yaml_file(os.path.join(config.CFG_DIR, "dataset_configs", "kitti_augmentor.yaml"))["DATA_AUGMENTOR_3CLASS"]
    if not gt_sampling:
        aug["DISABLE_AUG_LIST"] = ["gt_sampling"]
    cfg.DATA_CONFIG.DATA_AUGMENTOR = aug
    cfg.DATA_CONFIG.pop("_BASE_CONFIG_", None)
    for p in cfg.DATA_CONFIG.DATA_PROCESSOR:
        if p.NAME == "sample_points":
            p.NUM_POINTS = {"train": NUM_POINTS, "test": NUM_POINTS}
    cfg.MODEL.POST_PROCESSING.NMS_CONFIG.MULTI_CLASSES_NMS = bool(multi_class_nms)
    return cfg


def write_cfg(path, **kw):
    with open(path, "w") as f:
        yaml.safe_dump(plain(model_cfg(**kw)), f)
    return str(path)


def tree_frames(empty_train_frame=None):
    """(frames, splits): N_TRAIN train and N_VAL val frames; `empty_train_frame` names a train frame without any box."""
    boxes = [0 if i == empty_train_frame else BOXES for i in range(N_TRAIN)]
    train, _ = K.labelled_frames([POINTS] * N_TRAIN, boxes, seed=1)
    val, _ = K.labelled_frames([POINTS] * N_VAL, [BOXES] * N_VAL, seed=2)
    for f in val:
        f["split"] = "val"
    return train + val, {"train": [f["id"] for f in train], "val": [f["id"] for f in val], "test": []}


def write_tree_with_infos(root, cfg=None, empty_train_frame=None, device="cuda:0"):
    """The tree, its four info pickles and the train GT database under `root` (needs the GPU: the counts come from it)."""
    from hvpr_amd import kitti_dataset
    frames, splits = tree_frames(empty_train_frame)
    K.write_tree(root, K.tree_files(frames, splits))
    cfg = cfg if cfg is not None else model_cfg()
    kitti_dataset.create_kitti_infos(cfg.DATA_CONFIG, ["Car", "Pedestrian", "Cyclist"], root, root, device=device)
    return root


def sync_warnings(fn):
    """(result, synchronising calls torch warned about) of fn() under set_sync_debug_mode("warn")."""
    import torch
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, sum("synchroniz" in str(x.message).lower() for x in w)
