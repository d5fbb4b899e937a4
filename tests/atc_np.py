"""NumPy restatement of ATCDataset.sample (anchor / positive observation
pairs), written from its closed forms.  Test infrastructure: the CPU tests
check it against the reference's recorded batches
(tests/golden/atc_golden.npz), the GPU tests check atc_sample_kernel against it.

Closed forms
  valid(k)    the candidates c, in order, with c + k <= traj_end[c]; the
              candidates are the rows with valids > 0 when the dataset has
              'valids', else every row
  idxs        valid(k)[draws['pick']] (or draws['idxs'])
  keys        observations = obs(idxs), positive_observations = obs(idxs + k)
  obs(rows)   observations[rows]; with frame_stack F the F-frame stack of
              visual_np.stacked
  crop        with crop offsets, both keys when they are 4-D (visual_np.crop at
              padding cfg['augment_padding'], default 4)
"""

import numpy as np

import visual_np as vnp

PADDING = 4
KEYS = ('observations', 'positive_observations')


def valid_idxs(data, k):
    tend = vnp.traj_end(data['terminals'])
    cand = np.nonzero(np.asarray(data['valids']) > 0)[0] if 'valids' in data else np.arange(len(tend))
    return cand[cand + k <= tend[cand]].astype(np.int64)


def batch(data, cfg, k, draws, crop_from=None):
    """One ATCDataset.sample with the given draws ('pick', positions into
    valid(k), or 'idxs', the rows themselves).  Returns the batch in the
    reference's key order and the anchor rows."""
    valid = valid_idxs(data, k)
    if len(valid) == 0:
        raise ValueError(f'No valid ATC indices found for k={k}.')
    idxs = np.asarray(draws['idxs'], np.int64) if 'idxs' in draws else valid[np.asarray(draws['pick'], np.int64)]
    F = cfg.get('frame_stack')
    frames = data['observations']
    tend = vnp.traj_end(data['terminals'])

    def obs(rows):
        return vnp.stacked(frames, rows, tend, F) if F is not None else frames[rows]

    out = {'observations': obs(idxs), 'positive_observations': obs(idxs + k)}
    if crop_from is not None:
        for key in KEYS:
            if out[key].ndim == 4:
                out[key] = vnp.crop(out[key], crop_from, cfg.get('augment_padding', PADDING))
    return out, idxs


# ------------------------------------------------------------------ the fixture
# tests/golden/atc_golden.npz (make_golden_atc.py): the configs it ran and their k
CASES = {
    'state': (dict(frame_stack=None, p_aug=None), 1),
    'stack_state': (dict(frame_stack=3, p_aug=1.0), 3),
    'vis': (dict(frame_stack=3, p_aug=1.0), 2),
    'vis_pre': (dict(frame_stack=3, p_aug=1.0), 2),
    'vis_pad1': (dict(frame_stack=None, p_aug=1.0, augment_padding=1), 7),
    'regular': (dict(frame_stack=None, p_aug=1.0), 4),
    'k_last': (dict(frame_stack=3, p_aug=None), 29),
}
PREPROCESSED = ('vis_pre',)  # built with preprocess_frame_stack=True


def fixture_case(gold, case):
    """(dataset, k, the reference's valid(k), the rows it drew, draws ('pick'
    and, when the call drew them, 'crop_from'), expected batch, its key
    order)."""
    def part(tag):
        p = f'{case}_{tag}_'
        return {k[len(p):]: gold[k] for k in gold if k.startswith(p)}

    draws = part('draw')
    draws.pop('coin', None)
    return (part('in'), int(gold[f'{case}_k']), gold[f'{case}_valid'], gold[f'{case}_idxs'], draws, part('out'),
            [str(k) for k in gold[f'{case}_keys']])
