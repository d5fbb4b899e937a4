"""Seeded medium/hard powderworld worlds shared by the powder test files."""

import numpy as np

from oracle import powder_full_np as orc


def seeded_world(rng, n, size, ne):
    """Random full worlds: elements of the set, walls on the border, random
    velocities and momenta (the states a trajectory reaches)."""
    elems = orc.ELEM_IDS[ne] + [0, 0, 0]
    ids = rng.choice(elems, size=(n, size, size))
    ids[:, 0, :] = ids[:, -1, :] = ids[:, :, 0] = ids[:, :, -1] = orc.WALL
    w = orc.from_ids(ids)
    w[:, 3:5] = (rng.randn(n, 2, size, size) * 2.5).astype(np.float32) * (rng.rand(n, 1, size, size) < 0.3)
    w[:, 6] = rng.choice([-2, 0, 2], size=(n, size, size)) * np.isin(ids, orc.FLUIDS)
    w[:, 8] = rng.rand(n, size, size) < 0.2
    stone = ids == orc.STONE
    w[:, 2] = np.where(stone, rng.rand(n, size, size) < 0.5, w[:, 2])
    return w.astype(np.float32)
