"""ogbench_amd -- MI355X-native batched OGBench envs and offline replay.

Drop-in for the hot path of hliuson/ogbench:
  * ``make(env_id, num_envs=N, device=...)``  ~ ``gymnasium.make(env_id)`` for the
    locomaze (pointmaze) and powderworld registries, batched on one GPU;
  * ``make_env_and_datasets``/``load_dataset`` ~ ogbench/utils.py, returning
    HBM-resident dataset dicts of torch tensors;
  * ``datasets.GCDataset``/``HGCDataset`` ~ impls/utils/datasets.py, sampling with
    a fused HIP gather + hindsight-relabel kernel, and ``datasets.ATCDataset``,
    anchor / positive observation pairs for ATC pretraining in one launch, and
    ``datasets.ReplayBuffer``, batched on-device inserts and uniform sampling, and
    ``datasets.GCReplayBuffer``, hindsight goal sampling over an on-device episode
    ring filled by the batched envs, and ``datasets.HGCReplayBuffer``, the
    hierarchical (HIQL) batch over the same ring;
  * ``FrameStack`` ~ FrameStackWrapper of impls/utils/env_utils.py, the stacked
    observations of a batched env composed on the device (``env_utils`` holds
    the matching ``make_env_and_datasets(name, frame_stack=k)``).
All compute runs in libogbx.so (HIP, gfx950); there is no CPU fallback.
"""

from .datasets import ATCDataset, Dataset, GCDataset, GCReplayBuffer, HGCDataset, HGCReplayBuffer, ReplayBuffer
from .locomaze import MazeEnv, parse_env_id
from .powderworld import PowderworldEnv
from .registry import make, registered_env_ids
from .utils import load_dataset, make_env_and_datasets
from .wrappers import FrameStack

__all__ = ['ATCDataset', 'Dataset', 'FrameStack', 'GCDataset', 'GCReplayBuffer', 'HGCDataset', 'HGCReplayBuffer', 'MazeEnv', 'PowderworldEnv', 'ReplayBuffer', 'load_dataset', 'make', 'make_env_and_datasets', 'parse_env_id',
           'registered_env_ids']
