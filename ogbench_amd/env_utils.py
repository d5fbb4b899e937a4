"""The env side of impls/utils/env_utils.py (hliuson/ogbench) for the batched envs."""

from __future__ import annotations

from . import utils
from .wrappers import FrameStack


def make_env_and_datasets(dataset_name, frame_stack=None, dataset_path=None, **kw):
    """``make_env_and_datasets`` of impls/utils/env_utils.py:79-103.

    Makes the batched env and the compact datasets of ``dataset_name``
    (``utils.make_env_and_datasets(..., compact_dataset=True)``; ``kw`` goes
    there: ``num_envs``, ``device``, ``dataset_dir``, env options), wraps the
    env in ``FrameStack(env, frame_stack)`` when ``frame_stack`` is not None and
    resets it.  Returns (env, train_dataset, val_dataset), the datasets being
    the HBM-resident dicts ``datasets.Dataset`` / ``GCDataset`` take.
    """
    env, train_dataset, val_dataset = utils.make_env_and_datasets(
        dataset_name, dataset_path=dataset_path, compact_dataset=True, **kw)
    if frame_stack is not None:
        env = FrameStack(env, frame_stack)
    env.reset()
    return env, train_dataset, val_dataset
