"""An epoch of batches from a KITTI directory: the sampler, the batch split and the one-ahead preparation that the reference gets
from torch's DataLoader with worker processes (pcdet/datasets/__init__.py:24-70), over `batch_loader.DeviceBatchLoader`.

  EpochSampler      the index order of one rank in one epoch: the arithmetic of the reference's DistributedSampler
                    (pcdet/datasets/__init__.py:24-38), used at world 1 too, so one rank and N ranks cut the same permutation.
  EpochLoader       iterating yields the batch dicts of `DeviceBatchLoader.prepare_batch(indices, rng)` (`num_boxes` as a list, so
                    that nothing in them is uploaded again by `load_data_to_gpu`).  The generator is made from
                    (seed, epoch, rank) once per epoch and the GT sampler's per-class pointers start over (`AugmentPlanner.reset`),
                    as the state of the reference's workers does when they are forked again: an epoch is a pure function of
                    (seed, epoch, rank).
  build_dataloader  (dataset, loader, sampler) from a DATA_CONFIG block.

One-ahead preparation (`prefetch=True`).  `prepare_batch` reads the device twice; on the stream the training step runs on, the first
read waits for the whole previous step.  So batch k + 1 is prepared under `torch.cuda.stream(loader_stream)` before batch k is handed
out: its reads wait for loader work only.  A batch is handed over with an event the consumer's stream waits on, and every device
tensor of it gets `record_stream(consumer stream)`: it was allocated on the loader's stream and is read on another, and without that
the caching allocator may give its memory to the next batch while the step still reads it.  No Python threads, no extra processes.
The host may run at most `max_ahead` steps ahead of the device: the consumer calls `step_done()` after each step, which records an
event and waits for the one from `max_ahead` steps back (the loader's pinned staging buffers are written again one batch later, and
nothing else bounds the distance once no read waits for the step)."""
import collections
import math

import numpy as np
import torch

from .augment import ObjectBank
from .batch_loader import DeviceBatchLoader
from .config import _get
from .kitti_dataset import KittiDataset


class EpochSampler:
    """Indices of rank `rank` of `world` over a dataset of n frames.  Training: torch.randperm(n) seeded with seed + epoch;
    evaluation: arange(n).  Either is padded with its own head to a multiple of `world` and cut [rank::world].  Iterating yields
    the batches (lists of indices); drop_last is false, the last batch may be short."""

    def __init__(self, n, batch_size, training, seed=0, rank=0, world=1):
        if n < 1 or batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError("EpochSampler: n, batch_size, world >= 1 and 0 <= rank < world")
        self.n, self.batch_size, self.training = int(n), int(batch_size), bool(training)
        self.seed, self.rank, self.world, self.epoch = int(seed), int(rank), int(world), 0
        self.num_samples = int(math.ceil(self.n / self.world))
        self.total_size = self.num_samples * self.world

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def indices(self):
        if self.training:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(self.n, generator=g).tolist()
        else:
            order = list(range(self.n))
        order += order[: self.total_size - len(order)]
        return order[self.rank: self.total_size: self.world]

    def __iter__(self):
        order = self.indices()
        for i in range(0, len(order), self.batch_size):
            yield order[i: i + self.batch_size]

    def __len__(self):
        return int(math.ceil(self.num_samples / self.batch_size))


class EpochLoader:
    """The batches of `sampler`'s current epoch, prepared by `batch_loader` (module docstring).  `dataset` is kept for the caller
    (`loader.dataset`, as torch's DataLoader has it).  `len()` is the number of batches."""

    def __init__(self, dataset, batch_loader, sampler, seed=0, prefetch=True, max_ahead=2):
        self.dataset, self.batch_loader, self.sampler = dataset, batch_loader, sampler
        self.seed, self.prefetch, self.max_ahead = int(seed), bool(prefetch), max(1, int(max_ahead))
        self._stream = None
        self._steps = collections.deque()

    def __len__(self):
        return len(self.sampler)

    def _epoch_rng(self):
        return np.random.RandomState([self.seed, self.sampler.epoch, self.sampler.rank])

    def step_done(self):
        """The consumer's mark after a step is enqueued: bounds how far the host runs ahead of the device."""
        if not self.prefetch or not torch.cuda.is_available():
            return
        ev = torch.cuda.Event()
        ev.record()
        self._steps.append(ev)
        if len(self._steps) > self.max_ahead:
            self._steps.popleft().synchronize()

    def _prepare(self, indices, rng):
        batch = self.batch_loader.prepare_batch(indices, rng)
        if isinstance(batch.get("num_boxes"), np.ndarray):
            # host bookkeeping stays on the host: `load_data_to_gpu` uploads every ndarray it finds, a synchronising copy per step
            batch["num_boxes"] = batch["num_boxes"].tolist()
        return batch

    def _prepare_ahead(self, indices, rng):
        with torch.cuda.stream(self._stream):
            batch = self._prepare(indices, rng)
            ready = torch.cuda.Event()
            ready.record(self._stream)
        return batch, ready

    @staticmethod
    def _hand_over(batch, ready):
        consumer = torch.cuda.current_stream()
        consumer.wait_event(ready)
        for v in batch.values():
            if torch.is_tensor(v) and v.is_cuda:
                v.record_stream(consumer)
        return batch

    def __iter__(self):
        rng = self._epoch_rng()
        if self.batch_loader.planner is not None:
            self.batch_loader.planner.reset()
        self._steps.clear()
        if not self.prefetch:
            for indices in self.sampler:
                yield self._prepare(indices, rng)
            return
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.batch_loader.device)
        self._stream.wait_stream(torch.cuda.current_stream())       # whatever the loader reads (the bank) was put there before
        ahead = None
        for indices in self.sampler:
            nxt = self._prepare_ahead(indices, rng)
            if ahead is not None:
                yield self._hand_over(*ahead)
            ahead = nxt
        if ahead is not None:
            yield self._hand_over(*ahead)


def gt_sampling_cfg(dataset_cfg):
    """The gt_sampling entry of DATA_AUGMENTOR, listed in DISABLE_AUG_LIST or not (the bank is built either way; the planner
    decides whether it is sampled from)."""
    aug = _get(dataset_cfg, "DATA_AUGMENTOR")
    if aug is None:
        return None
    for c in (aug if isinstance(aug, list) else aug["AUG_CONFIG_LIST"]):
        if c["NAME"] == "gt_sampling":
            return c
    return None


def with_default_augmentor(dataset_cfg):
    """A model config that carries no DATA_AUGMENTOR trains with the block of cfgs/dataset_configs/kitti_augmentor.yaml (the
    reference's hvpr.yaml:29-54)."""
    if "DATA_AUGMENTOR" in dataset_cfg:
        return dataset_cfg
    import os
    from .config import CFG_DIR, AttrDict, cfg_from_yaml_file
    aug = cfg_from_yaml_file(os.path.join(CFG_DIR, "dataset_configs", "kitti_augmentor.yaml"))["DATA_AUGMENTOR"]
    return AttrDict(dataset_cfg, DATA_AUGMENTOR=aug)


def build_dataloader(dataset_cfg, class_names, batch_size, dist=False, root_path=None, training=True, seed=0, device="cuda:0",
                     prefetch=True, max_ahead=2):
    """(dataset, loader, sampler) as pcdet/datasets/__init__.py:41-70 returns them.  Training builds the ObjectBank of the GT sampler
    from its DB_INFO_PATH; `sample_points` is taken when DATA_PROCESSOR lists that step.  With `dist` the rank and world size are
    torch.distributed's."""
    if training:
        dataset_cfg = with_default_augmentor(dataset_cfg)
    dataset = KittiDataset(dataset_cfg, class_names, training=training, root_path=root_path, device=device)
    if len(dataset) == 0:
        raise FileNotFoundError(f"no info records under {dataset.root_path} for mode '{dataset.mode}': run "
                                "`python -m hvpr_amd.kitti_dataset create_kitti_infos` first")
    bank = None
    if training:
        s = gt_sampling_cfg(dataset_cfg)
        if s is not None:
            bank = ObjectBank.from_db_info_files(dataset.root_path, s["DB_INFO_PATH"], class_names, prepare=_get(s, "PREPARE"),
                                                 num_point_features=int(_get(s, "NUM_POINT_FEATURES", 4)), device=device)
        else:
            bank = ObjectBank({}, dataset.root_path, class_names, device=device)
    sample_points = any(p["NAME"] == "sample_points" for p in dataset_cfg["DATA_PROCESSOR"])
    batch_loader = DeviceBatchLoader(dataset_cfg, class_names, dataset.frame, len(dataset), bank=bank, training=training,
                                     device=device, sample_points=sample_points)
    rank, world = 0, 1
    if dist:
        import torch.distributed as td
        rank, world = td.get_rank(), td.get_world_size()
    sampler = EpochSampler(len(dataset), batch_size, training, seed=seed, rank=rank, world=world)
    return dataset, EpochLoader(dataset, batch_loader, sampler, seed=seed, prefetch=prefetch, max_ahead=max_ahead), sampler
