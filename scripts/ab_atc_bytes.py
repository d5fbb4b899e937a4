#!/usr/bin/env python
"""Same-bytes record of the ATC samplers (ATCDataset.sample,
GCReplayBuffer / HGCReplayBuffer.sample_atc) for an A/B of two trees, the
method of profiles/atc_host_refactor_ab.txt: run once per built tree, each in a
fresh process, and compare the two files with cmp.

  python scripts/ab_atc_bytes.py TREE_ROOT OUT.npz

Saves every tensor, key order, refill identity and raised message of every
call, and per sampler its call counter, atc_table_builds, atc_bad_samples()
and numpy's global stream, into an .npz with fixed zip timestamps.
"""
import io
import os
import sys
import zipfile

import numpy as np

root, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
import torch  # noqa: E402

import ogbench_amd  # noqa: E402,F401
from ogbench_amd import _lib  # noqa: E402
from ogbench_amd.datasets import ATCDataset, Dataset, GCReplayBuffer, HGCReplayBuffer  # noqa: E402

assert os.path.dirname(os.path.dirname(_lib.LIB_PATH)) == root.rstrip('/'), (_lib.LIB_PATH, root)
dev = torch.device('cuda:0')
B = 8
REC = {}
RAISED = []


def put(name, v):
    assert name not in REC, name
    REC[name] = np.asarray(v)


def save_batch(tag, out):
    put(f'{tag}/keys', np.array(list(out), dtype='U'))
    for k, v in out.items():
        if isinstance(v, dict):
            put(f'{tag}/{k}/keys', np.array(list(v), dtype='U'))
            for k2, v2 in v.items():
                put(f'{tag}/{k}/{k2}', v2.cpu().numpy())
        else:
            put(f'{tag}/{k}', v.cpu().numpy())


def attempt(tag, fn):
    try:
        out = fn()
    except Exception as e:  # the message is the record
        msg = f'{type(e).__name__}: {e}'
        put(f'{tag}/raised', np.array(msg))
        RAISED.append((tag, msg))
        return None
    save_batch(tag, out)
    return out


def drive(name, make, sample_name, nrows):
    np.random.seed(123)
    try:
        s = make()
    except Exception as e:
        msg = f'{type(e).__name__}: {e}'
        put(f'{name}/construct_raised', np.array(msg))
        RAISED.append((name, msg))
        return
    sample = getattr(s, sample_name)
    for k in (0, 1, 3):
        t = f'{name}/k{k}'
        plain = attempt(f'{t}/plain', lambda: sample(B, k))
        if plain is not None:
            k2 = {0: 1, 1: 3, 3: 0}[k]
            ptrs = [v.data_ptr() for v in plain.values()]
            again = attempt(f'{t}/refill_k{k2}', lambda: sample(B, k2, out=plain))
            put(f'{t}/refill_same_dict', again is plain)
            if again is not None:
                put(f'{t}/refill_same_storage', [v.data_ptr() for v in again.values()] == ptrs)
            wrong = attempt(f'{t}/refill_other_B', lambda: sample(B // 2, k, out=plain))
            put(f'{t}/refill_other_B_same_dict', wrong is plain)
        rows = np.arange(B, dtype=np.int64) % max(1, nrows - 12)
        attempt(f'{t}/idxs', lambda: sample(B, k, idxs=rows))
        attempt(f'{t}/idxs_bad', lambda: sample(B, k, idxs=np.arange(B, dtype=np.int64) + nrows - 4))
        rec = attempt(f'{t}/record', lambda: sample(B, k, record_draws=True))
        attempt(f'{t}/evaluation', lambda: sample(B, k, evaluation=True))
        attempt(f'{t}/record_evaluation', lambda: sample(B, k, evaluation=True, record_draws=True))
        if rec is not None:
            draws = {kk: vv.clone() for kk, vv in rec['_draws'].items()}
            attempt(f'{t}/inject_draws', lambda: sample(B, k, draws=draws, record_draws=True))
            attempt(f'{t}/inject_pick', lambda: sample(B, k, draws=dict(pick=draws['pick'])))
            attempt(f'{t}/inject_rows', lambda: sample(B, k, idxs=rec['_idxs'], draws=draws, record_draws=True))
        attempt(f'{t}/plain_again', lambda: sample(B, k))
    attempt(f'{name}/k_huge', lambda: sample(B, 1000))
    attempt(f'{name}/k_negative', lambda: sample(B, -1))
    put(f'{name}/calls', s._calls)
    put(f'{name}/atc_table_builds', getattr(s, 'atc_table_builds', -1))
    put(f'{name}/atc_bad_samples', s.atc_bad_samples() if hasattr(s, 'atc_bad_samples') else -1)
    put(f'{name}/numpy_stream', np.random.get_state()[1])
    put(f'{name}/numpy_stream_pos', np.random.get_state()[2])


rng = np.random.RandomState(0)
term = np.zeros(30, np.float32)
term[9::10] = 1
OBS = {'state': rng.normal(size=(30, 5)).astype(np.float32),
       'vis': rng.randint(0, 256, (30, 8, 8, 3)).astype(np.uint8)}
CFG = dict(frame_stack=3, p_aug=0.5)
for form, obs in OBS.items():
    base = dict(observations=obs, terminals=term)
    drive(f'ds_periodic_{form}', lambda: ATCDataset(Dataset(dict(base), device=dev), dict(CFG), seed=7), 'sample', 30)
    drive(f'ds_table_{form}', lambda: ATCDataset(Dataset(dict(base), device=dev), dict(CFG), seed=7, _periodic=False),
          'sample', 30)
    valids = (np.random.RandomState(4).rand(30) < 0.7).astype(np.float32)
    drive(f'ds_valids_{form}', lambda: ATCDataset(Dataset(dict(base, valids=valids), device=dev), dict(CFG), seed=7),
          'sample', 30)

GC = dict(discount=0.99, value_p_curgoal=0.2, value_p_trajgoal=0.5, value_p_randomgoal=0.3, value_geom_sample=True,
          actor_p_curgoal=0.0, actor_p_trajgoal=1.0, actor_p_randomgoal=0.0, actor_geom_sample=False,
          gc_negative=True)
N, T, STEPS = 3, 6, 8
EX = {'state': np.zeros(5, np.float32), 'vis': np.zeros((8, 8, 3), np.uint8)}
RING_CFG = {'state': dict(GC, frame_stack=None, p_aug=None), 'vis': dict(GC, **CFG)}


def ring(cls, form, extra):
    def make():
        cfg = dict(RING_CFG[form], **extra)
        buf = cls.create(dict(observations=EX[form]), N, T, cfg, device=dev, seed=7)
        r = np.random.RandomState(9)
        for step in range(STEPS):
            ex = EX[form]
            hi = 256 if ex.dtype == np.uint8 else 100
            obs = r.randint(0, hi, (N,) + ex.shape).astype(ex.dtype)
            done = np.array([step == 2, step == 4, step == 6])
            buf.add(dict(observations=torch.as_tensor(obs).to(dev)), torch.as_tensor(done).to(dev))
        return buf
    return make


for form in EX:
    drive(f'ring_gc_{form}', ring(GCReplayBuffer, form, {}), 'sample_atc', N * T)
    drive(f'ring_hgc_{form}', ring(HGCReplayBuffer, form, dict(subgoal_steps=3)), 'sample_atc', N * T)
# an empty ring
np.random.seed(123)
empty = GCReplayBuffer.create(dict(observations=EX['state']), N, T, RING_CFG['state'], device=dev, seed=7)
attempt('ring_empty/plain', lambda: empty.sample_atc(B, 0))
torch.cuda.synchronize()

with zipfile.ZipFile(out_path, 'w', zipfile.ZIP_STORED) as z:
    for name, arr in REC.items():
        buf = io.BytesIO()
        np.save(buf, arr, allow_pickle=False)
        z.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())
print(f'{len(REC)} arrays -> {out_path} (calls that raised: {len(RAISED)})')
for tag, msg in RAISED:
    print(f'  raised {tag}: {msg[:150]}')
