"""GPU: eval counters kernel (ogbx_eval_accumulate) and batched evaluate()."""

import numpy as np
import pytest
import torch

import ogbench_amd
from ogbench_amd.evaluation import accumulate, evaluate

pytestmark = pytest.mark.gpu


def test_accumulate_matches_host_recount(gpu):
    rng = np.random.RandomState(0)
    n, T, steps = 100_000, 5, 12
    task = rng.randint(1, T + 1, n).astype(np.int32)
    rem = rng.randint(0, 3, n).astype(np.int32)
    counters = torch.zeros(T, 2, dtype=torch.int64, device=gpu)
    remaining = torch.tensor(rem, device=gpu)
    exp = np.zeros((T, 2), np.int64)
    for _ in range(steps):
        s = rng.rand(n) < 0.3
        te = rng.rand(n) < 0.2
        tr = rng.rand(n) < 0.1
        accumulate(counters, torch.tensor(s, device=gpu).view(torch.uint8), torch.tensor(te, device=gpu).view(torch.uint8),
                   torch.tensor(tr, device=gpu).view(torch.uint8), torch.tensor(task, device=gpu), remaining)
        done = (te | tr) & (rem > 0)
        np.add.at(exp[:, 0], task[done] - 1, s[done].astype(np.int64))
        np.add.at(exp[:, 1], task[done] - 1, 1)
        rem = rem - done
    assert np.array_equal(counters.cpu().numpy(), exp)
    assert np.array_equal(remaining.cpu().numpy(), rem)


def test_evaluate_greedy_pointmaze_arena(gpu):
    env = ogbench_amd.make('pointmaze-arena-v0', num_envs=2048, device=gpu, auto_reset=True, max_episode_steps=200)

    def greedy(obs, goal):
        return torch.clamp((goal - obs) / 0.2, -1, 1).to(torch.float32)

    metrics, total, local = evaluate(greedy, env, episodes_per_env=2, seed=3)
    assert total[:, 1].sum().item() == 2048 * 2
    assert metrics['evaluation/overall_success'] == 1.0


def test_evaluate_counts_every_episode_powder(gpu):
    env = ogbench_amd.make('powderworld-easy-v0', num_envs=500, device=gpu, auto_reset=True, max_episode_steps=6)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(0)

    def rand_policy(obs, goal):
        return torch.randint(0, 8, (obs.shape[0],), device=gpu, generator=gen, dtype=torch.int32)

    metrics, total, _ = evaluate(rand_policy, env, episodes_per_env=3, seed=1)
    t = total.cpu().numpy()
    assert t[:, 1].sum() == 1500
    assert np.array_equal(t[:, 1], np.bincount(np.arange(500) % 5, minlength=5) * 3)
    assert set(metrics) == {f'evaluation/{ti["task_name"]}_success' for ti in env.task_infos} | {
        'evaluation/overall_success'}


def test_rccl_cabi_allgather_single_rank(gpu):
    """The C-ABI RCCL communicator (ogbx_comm_create / ogbx_eval_allgather) on
    one rank: the gather is the identity, and gather_counters(comm=...) sums it."""
    import torch

    from ogbench_amd.evaluation import RcclComm, comm_unique_id, gather_counters

    uid = comm_unique_id()
    assert len(uid) == 128
    comm = RcclComm(1, 0, gpu, uid)
    c = torch.arange(10, dtype=torch.int64, device=gpu).view(5, 2) * 7 + 3
    out = comm.allgather(c)
    assert out.shape == (1, 5, 2) and torch.equal(out[0], c)
    total, per_rank = gather_counters(c, comm=comm)
    assert torch.equal(total, c) and per_rank.shape == (1, 5, 2)
    comm.close()


# ---- ogbx_eval_accumulate at its edges, against the same NumPy recount ----


def _recount(counters, s, te, tr, task, rem):
    """What one accumulate call does, on host arrays (in place).  A row whose
    task id is outside 1..T ends its episode (remaining drops) but adds to no
    counter (include/ogbx.h); success counts as 1 whenever its byte is non-zero."""
    T = counters.shape[0]
    done = ((te != 0) | (tr != 0)) & (rem > 0)
    ok = done & (task >= 1) & (task <= T)
    np.add.at(counters[:, 0], task[ok] - 1, (s[ok] != 0).astype(np.int64))
    np.add.at(counters[:, 1], task[ok] - 1, 1)
    rem -= done.astype(np.int32)


def _accumulate_both(gpu, counters, remaining, exp, rem, s, te, tr, task):
    accumulate(counters, *(torch.tensor(np.ascontiguousarray(v, np.uint8), device=gpu) for v in (s, te, tr)),
               torch.tensor(task, device=gpu), remaining)
    _recount(exp, s, te, tr, task, rem)


def _u8(rng, n, p):
    return (rng.rand(n) < p).astype(np.uint8)


@pytest.mark.parametrize('n', [1, 255, 256, 257, 262_145])
def test_accumulate_sizes(gpu, n):
    """One lane, a block less one, a full block, a block and one, and one env
    more than the 1,024 x 256 launch covers in one trip (the grid-stride loop)."""
    rng = np.random.RandomState(n)
    T = 5
    task = rng.randint(1, T + 1, n).astype(np.int32)
    rem = rng.randint(0, 3, n).astype(np.int32)
    rem[-1] = 2                                             # the last env always has something to add
    counters = torch.zeros(T, 2, dtype=torch.int64, device=gpu)
    remaining = torch.tensor(rem, device=gpu)
    exp = np.zeros((T, 2), np.int64)
    for step in range(3):
        s = rng.choice(np.array([0, 1, 2, 255], np.uint8), n)
        te, tr = _u8(rng, n, 0.5), _u8(rng, n, 0.3)
        te[-1] = 1
        _accumulate_both(gpu, counters, remaining, exp, rem, s, te, tr, task)
    assert exp[:, 1].sum() >= 2
    assert np.array_equal(counters.cpu().numpy(), exp)
    assert np.array_equal(remaining.cpu().numpy(), rem)


def test_accumulate_every_lane_on_one_counter(gpu):
    """All 262,145 envs finish task 2 in one call: every lane of every
    workgroup adds to the same LDS counter pair."""
    n, T = 262_145, 3
    one = torch.ones(n, dtype=torch.uint8, device=gpu)
    zero = torch.zeros(n, dtype=torch.uint8, device=gpu)
    counters = torch.zeros(T, 2, dtype=torch.int64, device=gpu)
    remaining = torch.full((n,), 2, dtype=torch.int32, device=gpu)
    accumulate(counters, one, one, zero, torch.full((n,), 2, dtype=torch.int32, device=gpu), remaining)
    assert counters.cpu().tolist() == [[0, 0], [n, n], [0, 0]]
    assert torch.equal(remaining.cpu(), torch.full((n,), 1, dtype=torch.int32))


@pytest.mark.parametrize('T', [1, 64])
def test_accumulate_task_limit_accepted(gpu, T):
    rng = np.random.RandomState(T)
    n = 64 * 9 + 1
    task = (np.arange(n) % T + 1).astype(np.int32)          # every task present
    assert set(task.tolist()) == set(range(1, T + 1))
    rem = np.full(n, 2, np.int32)
    counters = torch.zeros(T, 2, dtype=torch.int64, device=gpu)
    remaining = torch.tensor(rem, device=gpu)
    exp = np.zeros((T, 2), np.int64)
    for step in range(2):
        _accumulate_both(gpu, counters, remaining, exp, rem, _u8(rng, n, 0.5), _u8(rng, n, 0.7), _u8(rng, n, 0.2),
                         task)
    assert (exp[:, 1] > 0).all()
    assert np.array_equal(counters.cpu().numpy(), exp)
    assert np.array_equal(remaining.cpu().numpy(), rem)


@pytest.mark.parametrize('T', [0, 65])
def test_accumulate_task_limit_rejected(gpu, T):
    n = 300
    one = torch.ones(n, dtype=torch.uint8, device=gpu)
    task = torch.ones(n, dtype=torch.int32, device=gpu)
    counters = torch.full((T, 2), 7, dtype=torch.int64, device=gpu)
    remaining = torch.full((n,), 3, dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError):
        accumulate(counters, one, one, one, task, remaining)
    assert (counters.cpu() == 7).all()
    assert (remaining.cpu() == 3).all()


def test_accumulate_out_of_range_task_ids(gpu):
    """include/ogbx.h: a task id outside 1..T adds to no counter, and the
    env's remaining is decremented all the same."""
    rng = np.random.RandomState(4)
    n, T = 1000, 4
    task = rng.choice(np.array([0, -1, T + 1, 1, 2, 3, 4, -2**31, 2**31 - 1], np.int32), n)
    task[:3] = [0, -1, T + 1]
    rem = np.full(n, 2, np.int32)
    counters = torch.zeros(T, 2, dtype=torch.int64, device=gpu)
    remaining = torch.tensor(rem, device=gpu)
    exp = np.zeros((T, 2), np.int64)
    ones = np.ones(n, np.uint8)
    _accumulate_both(gpu, counters, remaining, exp, rem, ones, ones, ones * 0, task)
    valid = (task >= 1) & (task <= T)
    assert exp[:, 1].sum() == valid.sum() < n and (rem == 1).all()
    assert np.array_equal(counters.cpu().numpy(), exp)
    assert np.array_equal(remaining.cpu().numpy(), rem)


def test_accumulate_success_bytes_and_flags(gpu):
    """Success bytes 0, 1, 2, 255 count as 0, 1, 1, 1; terminated and truncated
    both set count once; rows with remaining == 0 never count."""
    T = 2
    s = np.array([0, 1, 2, 255] * 6, np.uint8)
    te = np.array([1] * 4 + [0] * 4 + [1] * 4 + [0] * 4 + [1] * 4 + [255] * 4, np.uint8)
    tr = np.array([0] * 4 + [1] * 4 + [1] * 4 + [0] * 4 + [1] * 4 + [2] * 4, np.uint8)
    rem = np.array([1] * 16 + [0] * 4 + [5] * 4, np.int32)
    task = np.array([1, 1, 1, 1, 2, 2, 2, 2] * 3, np.int32)
    counters = torch.zeros(T, 2, dtype=torch.int64, device=gpu)
    remaining = torch.tensor(rem, device=gpu)
    exp = np.zeros((T, 2), np.int64)
    _accumulate_both(gpu, counters, remaining, exp, rem, s, te, tr, task)
    # rows 0-3 and 8-11 count for task 1, rows 4-7 and 20-23 for task 2, three successes in each group of
    # four; rows 12-15 have no flag set and rows 16-19 nothing remaining
    assert exp.tolist() == [[6, 8], [6, 8]]
    assert rem.tolist() == [0] * 12 + [1] * 4 + [0] * 4 + [4] * 4
    assert np.array_equal(counters.cpu().numpy(), exp)
    assert np.array_equal(remaining.cpu().numpy(), rem)


def test_accumulate_remaining_runs_out_on_different_steps(gpu):
    """Six steps in which every env ends an episode; env i owes i % 7 episodes,
    so it stops counting after that many steps."""
    rng = np.random.RandomState(6)
    n, T = 700, 5
    task = (np.arange(n) % T + 1).astype(np.int32)
    rem = (np.arange(n) % 7).astype(np.int32)
    owed = rem.copy()
    counters = torch.zeros(T, 2, dtype=torch.int64, device=gpu)
    remaining = torch.tensor(rem, device=gpu)
    exp = np.zeros((T, 2), np.int64)
    ones = np.ones(n, np.uint8)
    for step in range(6):
        _accumulate_both(gpu, counters, remaining, exp, rem, _u8(rng, n, 0.4), ones, _u8(rng, n, 0.5), task)
        assert np.array_equal(rem, np.maximum(owed - step - 1, 0))
        assert np.array_equal(remaining.cpu().numpy(), rem)
    assert exp[:, 1].sum() == np.minimum(owed, 6).sum()
    assert np.array_equal(counters.cpu().numpy(), exp)


def test_accumulate_adds_to_counters_and_carries_past_32_bits(gpu):
    n, T = 10, 3
    start = np.array([[2**32 - 3, 2**32 - 3], [5, 9], [2**40 + 1, 2**32 - 1]], np.int64)
    counters = torch.tensor(start, device=gpu)
    exp = start.copy()
    rem = np.ones(n, np.int32)
    remaining = torch.tensor(rem, device=gpu)
    ones = np.ones(n, np.uint8)
    task = np.array([1] * 6 + [2] + [3] * 3, np.int32)
    _accumulate_both(gpu, counters, remaining, exp, rem, ones, ones, ones, task)
    assert exp.tolist() == [[2**32 + 3, 2**32 + 3], [6, 10], [2**40 + 4, 2**32 + 2]]
    assert np.array_equal(counters.cpu().numpy(), exp)


def test_accumulate_no_envs_is_a_no_op(gpu):
    counters = torch.full((3, 2), 11, dtype=torch.int64, device=gpu)
    e8 = torch.empty(0, dtype=torch.uint8, device=gpu)
    e32 = torch.empty(0, dtype=torch.int32, device=gpu)
    accumulate(counters, e8, e8, e8, e32, e32)
    assert (counters.cpu() == 11).all()
