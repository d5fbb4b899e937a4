"""NumPy restatement of the TRL branch of GCDataset.sample (the value midpoint
and the keys around it), written from its closed forms.  Test infrastructure:
the CPU tests check it against the reference's recorded batches
(tests/golden/trl_golden.npz), the GPU tests check trl_sample_kernel against
it.

Closed forms
  pick table  every row r with traj_end[r] != r, whether or not the dataset
              has 'valids'; sample rows and random goals come from it
  GC part     oracle/gcdataset_np.sample over that pick table
  midpoint    draws['midpoint'], one row per sample in [idx, value goal)
  keys        value_goal_observations = actor_goal_observations = obs(value goal)
              value_offsets = goal - idx, value_midpoint_offsets = mid - idx
              value_midpoint_observations = obs(mid)
              value_midpoint_actions = actions[mid], next_actions = actions[idx + 1]
              value_midpoint_goals / value_cur_goals / value_next_goals =
                oracle_reps[mid / idx / idx + 1], or obs(...) without them
  obs(rows)   observations[rows]; with frame_stack F the F-frame stack of
              visual_np.stacked
  crop        with crop offsets, every 4-D array among observations,
              next_observations, value_goals, actor_goals and the six
              observation-valued TRL keys (visual_np.crop, one offset pair per
              sample)
"""

import numpy as np

import visual_np as vnp
from oracle import gcdataset_np as orc

CROP_KEYS = ('observations', 'next_observations', 'value_goals', 'actor_goals', 'value_goal_observations',
             'actor_goal_observations', 'value_midpoint_observations', 'value_midpoint_goals', 'value_cur_goals',
             'value_next_goals')


def pick_table(terminals):
    tend = vnp.traj_end(terminals)
    return np.nonzero(tend != np.arange(len(tend)))[0]


def prepare(data):
    return dict(valid=pick_table(data['terminals']), term_locs=np.nonzero(np.asarray(data['terminals']) > 0)[0])


def batch(data, cfg, draws, crop_from=None, idxs=None):
    """One TRL GCDataset.sample with the given draws (the eleven GC draws and
    'midpoint').  Returns the batch in the reference's key order and the
    index vectors."""
    prep = prepare(data)
    out, idxs, vg, ag = orc.sample(data, cfg, draws, idxs=idxs, prep=prep)
    mid = np.asarray(draws['midpoint'], np.int64)
    F = cfg.get('frame_stack')
    frames = data['observations']
    tend = vnp.traj_end(data['terminals'])

    def obs(rows):
        return vnp.stacked(frames, rows, tend, F) if F is not None else frames[rows]

    def goal(rows):
        return data['oracle_reps'][rows] if 'oracle_reps' in data else obs(rows)

    if F is not None:
        out['observations'] = obs(idxs)
        out['next_observations'] = obs(idxs + 1)
        out['value_goals'] = goal(vg)
        out['actor_goals'] = goal(ag)
    out['value_goal_observations'] = obs(vg)
    out['actor_goal_observations'] = obs(vg)
    out['value_offsets'] = vg - idxs
    out['value_midpoint_offsets'] = mid - idxs
    out['value_midpoint_observations'] = obs(mid)
    out['value_midpoint_actions'] = data['actions'][mid]
    out['next_actions'] = data['actions'][idxs + 1]
    out['value_midpoint_goals'] = goal(mid)
    out['value_cur_goals'] = goal(idxs)
    out['value_next_goals'] = goal(idxs + 1)
    if crop_from is not None:
        for k in CROP_KEYS:
            if out[k].ndim == 4:
                out[k] = vnp.crop(out[k], crop_from)
    return out, dict(idxs=idxs, vg=vg, ag=ag, mid=mid)


# ------------------------------------------------------------------ the fixture
# tests/golden/trl_golden.npz (make_golden_trl.py): the configs it ran
STATE_CFG = dict(discount=0.9, value_p_curgoal=0.0, value_p_trajgoal=1.0, value_p_randomgoal=0.0,
                 value_geom_sample=True, actor_p_curgoal=0.0, actor_p_trajgoal=0.5, actor_p_randomgoal=0.5,
                 actor_geom_sample=False, gc_negative=False, p_aug=None, frame_stack=None, agent_name='trl')
CASES = {
    'state': STATE_CFG,
    'reps': dict(STATE_CFG, value_geom_sample=False),
    'regular': STATE_CFG,
    'vis': dict(STATE_CFG, agent_name='latent_trl', frame_stack=3, p_aug=1.0),
}


def fixture_case(gold, case):
    """(dataset, draws incl. 'midpoint' and, when the call cropped,
    'crop_from', expected batch, its key order)."""
    def part(tag):
        p = f'{case}_{tag}_'
        return {k[len(p):]: gold[k] for k in gold if k.startswith(p)}

    draws = part('draw')
    draws.pop('coin', None)
    return part('in'), draws, part('out'), [str(k) for k in gold[f'{case}_keys']]
