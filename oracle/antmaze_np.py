"""NumPy restatement of the antmaze wrapper -- TEST INFRASTRUCTURE ONLY (the
checker of ogbench_amd/csrc/antmaze.h and bench.py's cpu_baseline leg; never a
product path).

Follows the reference's MazeEnv.reset/step (ogbench/locomaze/maze.py:373-466)
and AntEnv.get_ob/reset_model/set_xy (ogbench/locomaze/ant.py:97-122) for
loco_env_type 'ant' over a batch, around caller-supplied post-physics states
(the ant's articulated dynamics are out of scope):
  ob = concat(qpos, qvel); success = ||qpos[:2] - goal|| <= 0.5 (maze.py:86,
  486-490; the 2-norm rounded as NumPy's BLAS does, sqrt(fma(dy, dy, dx*dx)));
  teleport: qpos[:2] := an out-portal when within 1.5 radii of an in-portal
  (maze.py:442-451; the out-portal index is injected);
  terminated = success & terminate_at_goal; reward = success (-1 for a
  single-task env); TimeLimit truncation at max_episode_steps; reset ob =
  qpos0 + uniform(-0.1, 0.1) with xy := init_xy, qvel = 0.1 * normal.
Pinned by tests/golden/antmaze_golden.npz and antmaze_edges_golden.npz
(tests/test_antmaze_cpu.py).
"""

from fractions import Fraction

import numpy as np

QPOS0 = np.array([0, 0, 0.75, 1, 0, 0, 0] + [0] * 8, np.float64)  # ant.xml qpos0
GOAL_TOL = 0.5
# maze.py:322-329 (init_ij, goal_ij) of the large maze
LARGE_TASKS = np.array([[1, 1, 7, 10], [5, 4, 7, 1], [7, 4, 1, 10], [3, 8, 5, 4], [1, 1, 5, 4]])
# maze.py:338-345 of the teleport maze
TELEPORT_TASKS = np.array([[1, 10, 7, 1], [1, 1, 7, 10], [5, 6, 7, 10], [7, 1, 7, 10], [5, 6, 7, 1]])


def ij_to_xy(i, j):
    return j * 4.0 - 4, i * 4.0 - 4  # maze.py:558-562


def within(dx, dy, tol=GOAL_TOL):
    """sqrt(fma(dy, dy, dx*dx)) <= tol, exactly: the plain float expression
    decides every pair except those within 1e-12 of the boundary, which are
    rounded once through rationals.  A NaN or infinite distance is outside."""
    dx = np.asarray(dx, np.float64)
    dy = np.asarray(dy, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        r = np.sqrt(dx * dx + dy * dy)
        out = r <= tol
        near = np.abs(r - tol) <= 1e-12
    for k in np.nonzero(near)[0]:
        s = float(Fraction(float(dy[k])) ** 2 + Fraction(float(dx[k] * dx[k])))
        out[k] = np.sqrt(s) <= tol
    return out


def teleport_table(info):
    """(in_xy [I,2], out_xy [O,2], radius) of a reference _teleport_info dict
    (maze.py:151-161; tests/golden/teleport_golden.json)."""
    ins = np.array([ij_to_xy(i, j) for i, j in info['teleport_in_ijs']], np.float64)
    outs = np.array([ij_to_xy(i, j) for i, j in info['teleport_out_ijs']], np.float64)
    return ins, outs, float(info['teleport_radius'])


def reset_obs(task, noise, body_draws, tasks=LARGE_TASKS, *, task_xy=None, add_noise_to_goal=True):
    """Batched MazeEnv.reset ob and goal: task [N] 1-based, noise [N,4]
    uniform(-1,1) add_noise draws, body_draws [N,29] reset_model draws.
    task_xy [N,4] (init_xy, goal_xy cell centres; a task_info option) replaces
    the table rows; without add_noise_to_goal the goal is the cell centre."""
    noise = np.asarray(noise, np.float64)
    if task_xy is not None:
        ix, iy, gx, gy = np.asarray(task_xy, np.float64).T
    else:
        t = tasks[np.asarray(task) - 1]
        ix, iy = ij_to_xy(t[:, 0], t[:, 1])
        gx, gy = ij_to_xy(t[:, 2], t[:, 3])
    init = np.stack([ix + noise[:, 0] * 4.0 / 4, iy + noise[:, 1] * 4.0 / 4], 1)
    if add_noise_to_goal:
        goal = np.stack([gx + noise[:, 2] * 4.0 / 4, gy + noise[:, 3] * 4.0 / 4], 1)
    else:
        goal = np.stack([gx, gy], 1).astype(np.float64)
    ob = np.concatenate([QPOS0 + body_draws[:, :15], 0.0 + 0.1 * body_draws[:, 15:]], 1)
    ob[:, :2] = init
    return ob, goal


def goal_obs(goal, goal_states):
    """info['goal'] of MazeEnv.reset (maze.py:407-418): the body state after
    the goal reset's random physics steps (given, [N,29]) with set_xy(goal_xy),
    as get_ob() concatenates it (ant.py:97-122)."""
    g = np.array(goal_states, np.float64, copy=True)
    g[:, :2] = goal
    return g


class Batch:
    """State of N antmaze envs between wrapper steps.

    Keyword options (defaults = the registered multi-task large maze):
    terminate_at_goal, reward_task_id (single-task: every env takes that task
    whatever `task` says, reward is -1 / 0), add_noise_to_goal, task_xy
    ([N,4], the task_info option), teleport (teleport_table(...)).
    With track_body (implied by teleport), after a step body_q / body_v hold
    the reference's data.qpos / data.qvel (the teleport's set_xy and an
    auto-reset included) and final_obs the step's ob before any auto-reset."""

    def __init__(self, task, noise, body_draws, max_steps=1000, timing='post', tasks=LARGE_TASKS, *,
                 terminate_at_goal=True, reward_task_id=None, add_noise_to_goal=True, task_xy=None, teleport=None,
                 track_body=False):
        self.task = np.asarray(task).copy()
        if reward_task_id is not None:
            self.task[:] = reward_task_id or 1  # maze.py:361-362,377-381: options['task_id'] is ignored
        self.tasks = tasks
        self.add_noise_to_goal = add_noise_to_goal
        ob, self.goal = reset_obs(self.task, noise, body_draws, tasks, task_xy=task_xy,
                                  add_noise_to_goal=add_noise_to_goal)
        self.reset_ob = ob
        self.xy = ob[:, :2].copy()
        self.body_q, self.body_v = ob[:, :15].copy(), ob[:, 15:].copy()
        self.final_obs = None
        self.elapsed = np.zeros(len(self.task), np.int64)
        self.max_steps = max_steps
        self.timing = timing
        self.terminate_at_goal = terminate_at_goal
        self.single_task = reward_task_id is not None
        self.teleport = teleport
        self.track_body = track_body or teleport is not None

    def step(self, qpos, qvel, auto_reset=False, rng=None, *, tp_out=None, reset_noise=None, reset_states=None):
        """One wrapper step on post-physics states.  tp_out [N]: the out-portal
        index np.random.randint would return for each env that teleports.
        With auto_reset the ending envs are reset (the host loop's
        reset(options={'task_id': same})) from `rng` draws (timing leg of
        bench.py), or from reset_noise [N,4] (add_noise draws) and reset_states
        [N,29] (the reset_model state before set_xy) rows."""
        obs = np.concatenate([qpos, qvel], 1)
        xy = self.xy if self.timing == 'pre' else qpos[:, :2]
        succ = within(xy[:, 0] - self.goal[:, 0], xy[:, 1] - self.goal[:, 1])
        self.elapsed += 1
        trunc = self.elapsed >= self.max_steps
        term = succ & bool(self.terminate_at_goal)
        reward = succ.astype(np.float32)
        if self.single_task:
            reward = reward - np.float32(1.0)
        if self.track_body:
            self.body_q, self.body_v = np.array(qpos, np.float64), np.array(qvel, np.float64)
            self.final_obs = obs.copy()
        if self.teleport is not None:
            ins, outs, radius = self.teleport
            todo = np.ones(len(obs), bool)
            for cx, cy in ins:  # the first matching in-portal wins (the reference's break)
                hit = todo & within(qpos[:, 0] - cx, qpos[:, 1] - cy, radius * 1.5)
                self.body_q[hit, :2] = outs[np.asarray(tp_out)[hit]]
                todo &= ~hit
        self.xy = (self.body_q if self.teleport is not None else qpos)[:, :2].copy()
        if auto_reset:
            done = np.nonzero(term | trunc)[0]
            if len(done):
                if reset_states is None:
                    ob, goal = reset_obs(self.task[done], rng.uniform(-1, 1, (len(done), 4)),
                                         np.concatenate([rng.uniform(-0.1, 0.1, (len(done), 15)),
                                                         rng.standard_normal((len(done), 14))], 1), self.tasks)
                else:
                    ob, goal = reset_obs(self.task[done], np.asarray(reset_noise)[done], np.zeros((len(done), 29)),
                                         self.tasks, add_noise_to_goal=self.add_noise_to_goal)
                    init = ob[:, :2].copy()
                    ob = np.array(np.asarray(reset_states)[done], np.float64)
                    ob[:, :2] = init
                obs[done] = ob
                self.goal[done] = goal
                self.xy[done] = ob[:, :2]
                if self.track_body:
                    self.body_q[done], self.body_v[done] = ob[:, :15], ob[:, 15:]
                self.elapsed[done] = 0
        return obs, reward, term, trunc, succ
