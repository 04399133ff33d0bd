"""Leaf helpers of pcdet/utils/common_utils.py that the hot path and the drivers use."""
import logging
import os
import sys

import numpy as np
import torch


def limit_period(val, offset=0.5, period=np.pi):
    """common_utils.py:20-23."""
    is_np = isinstance(val, np.ndarray)
    t = torch.from_numpy(val).float() if is_np else val
    out = t - torch.floor(t / period + offset) * period
    return out.numpy() if is_np else out


def mask_points_by_range(points, limit_range):
    """common_utils.py:59-62."""
    return (points[:, 0] >= limit_range[0]) & (points[:, 0] <= limit_range[3]) & \
           (points[:, 1] >= limit_range[1]) & (points[:, 1] <= limit_range[4])


def create_logger(log_file=None, rank=0, name="hvpr_amd"):
    """common_utils.py:130-144: INFO on rank 0 and ERROR elsewhere, to stdout and on rank 0 to `log_file`.  One logger per name,
    process and log file; a second call for the same one adds no handler."""
    logger = logging.getLogger("%s.%d.%s" % (name, os.getpid(), log_file))
    logger.setLevel(logging.INFO if rank == 0 else logging.ERROR)
    logger.propagate = False
    if not logger.handlers:
        fmt = logging.Formatter("%(asctime)s  %(levelname)5s  %(message)s")
        handlers = [logging.StreamHandler(sys.stdout)] + ([logging.FileHandler(str(log_file))] if log_file is not None and rank == 0 else [])
        for h in handlers:
            h.setFormatter(fmt)
            logger.addHandler(h)
    return logger
