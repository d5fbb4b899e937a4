"""GPU: ATCDataset.sample and GCReplayBuffer.sample_atc run one host body
(datasets._AtcHost).  The same misuse raises the same message from both, takes
no call from either counter and leaves both samplers working: their next
batches are the ones the restatements (tests/atc_np.py, tests/online_atc_np.py)
build from the recorded draws."""

import numpy as np
import pytest
import torch

import atc_np as anp
import online_atc_np as oan
import online_np as onp
from ogbench_amd.datasets import ATCDataset, Dataset, GCReplayBuffer

pytestmark = pytest.mark.gpu
B, K = 4, 1
FRAME = (8, 8, 3)
ATC_CFG = dict(frame_stack=3, p_aug=1.0)  # every call's coin comes up: an injected crop_from is staged
RING_CFG = dict(onp.GOLDEN_CONFIGS['geom_neg'], **ATC_CFG)
N, T, STEPS = 3, 6, 8

MISUSES = [
    (dict(k=K, draws=dict(v_pick=np.zeros(B, np.int64))), "unknown draw 'v_pick'"),
    (dict(k=K, draws=dict(pick=np.zeros(3, np.int64))), "draw 'pick' must have 4 entries, got 3"),
    (dict(k=K, draws=dict(crop_from=np.zeros((B, 3), np.int64))),
     "draws['crop_from'] must have shape (4, 2), got (4, 3)"),
    (dict(k=-1), 'k must be >= 0, got -1'),
]


def _np(t):
    return t.cpu().numpy()


def _assert_batch(out, exp, what):
    assert [k for k in out if not k.startswith('_')] == list(exp) == list(anp.KEYS), what
    for k, v in exp.items():
        got = _np(out[k])
        assert got.dtype == v.dtype and got.shape == v.shape, (what, k)
        np.testing.assert_array_equal(got, v, err_msg=f'{what} {k}')


def test_one_host_body_for_the_dataset_and_the_ring(gpu):
    rng = np.random.RandomState(5)
    term = np.zeros(30, np.float32)
    term[9::10] = 1  # 3 trajectories of 10 rows
    data = dict(observations=rng.randint(0, 256, (30,) + FRAME).astype(np.uint8), terminals=term)
    ds = ATCDataset(Dataset(data, device=gpu), dict(ATC_CFG), seed=7)

    ex = dict(observations=np.zeros(FRAME, np.uint8))
    ring = GCReplayBuffer.create(ex, N, T, RING_CFG, device=gpu, seed=7)
    ref = onp.OnlineNp(ex, N, T)
    for step in range(STEPS):
        batch = dict(observations=rng.randint(0, 256, (N,) + FRAME).astype(np.uint8))
        done = np.array([step == 2, step == 4, step in (1, 6)])
        ring.add({k: torch.as_tensor(v).to(gpu) for k, v in batch.items()}, torch.as_tensor(done).to(gpu))
        ref.add(batch, done)

    calls = ds._calls, ring._calls
    for kw, message in MISUSES:
        raised = []
        for sample in (ds.sample, ring.sample_atc):
            with pytest.raises(ValueError) as err:
                sample(B, **kw)
            raised.append(str(err.value))
        assert raised == [message, message]
    assert (ds._calls, ring._calls) == calls  # a refused call draws nothing

    out = ds.sample(B, K, record_draws=True)
    draws = {k: _np(v) for k, v in out['_draws'].items()}
    exp, idxs = anp.batch(data, ATC_CFG, K, draws, draws.pop('crop_from'))
    _assert_batch(out, exp, 'dataset')
    np.testing.assert_array_equal(_np(out['_idxs']), idxs)

    out = ring.sample_atc(B, K, record_draws=True)
    draws = {k: _np(v) for k, v in out['_draws'].items()}
    exp, idxs = oan.batch(ref, RING_CFG, K, dict(pick=draws['pick']), draws['crop_from'])
    _assert_batch(out, exp, 'ring')
    np.testing.assert_array_equal(_np(out['_idxs']), idxs)

    assert (ds._calls - calls[0], ring._calls - calls[1]) == (1, 1)
