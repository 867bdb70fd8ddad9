"""BatchedEnv.step_envs / crafter_step_envs on the device: envs stepped at their own pace through random subsets equal the oracle
playing each env's own action sequence, on every subset kernel; rows that are not named stay bit-identical; a batch stepped by
subsets equals a batch stepped whole, mixed with step() and rollout() on a handle that keeps a dispatch order; bad index lists
are refused on the host or, whole, on the device."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests.parity import assert_same, sha8
from tests.rollout import oracle_rollouts

pytestmark = pytest.mark.gpu

LENGTH = 20
CALLS = 150
SIZES = (1, 2, 7, 40)
SAMPLED = 6


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env):
  return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(env.device)


def _other_rules():
  from crafter_amd import tables
  rules = copy.deepcopy(tables.load_rules())
  rules['items']['health'] = {'max': 5, 'initial': 5}
  return rules


@functools.lru_cache(maxsize=None)
def _schedule(n):
  """-> (sample, calls): SAMPLED env rows and CALLS pairs (idx, actions) of random subsets, sizes drawn from SIZES (40: every env, in
  a random order).  The small subsets name sampled envs first, in turn, so that every sampled env steps often enough."""
  rs = np.random.RandomState(1000 + n)
  sample = [int(v) for v in rs.choice(n, SAMPLED, replace=False)]
  others = np.setdiff1d(np.arange(n), sample)
  turn, calls = 0, []
  for _ in range(CALLS):
    size = int(rs.choice(SIZES))
    if size >= n or size == 40:
      idx = rs.permutation(n)
    else:
      k = min(size, 3)
      mine = [sample[(turn + j) % SAMPLED] for j in range(k)]
      turn += k
      idx = rs.permutation(np.concatenate([mine, rs.choice(others, size - k, replace=False)]).astype(np.int64))
    calls.append((idx.astype(np.int32), rs.randint(0, 17, len(idx)).astype(np.int32)))
  return sample, calls


def _own_tapes(n):
  sample, calls = _schedule(n)
  tapes = {row: [] for row in sample}
  for idx, acts in calls:
    for i, a in zip(idx.tolist(), acts.tolist()):
      if i in tapes:
        tapes[i].append(a)
  return {row: np.asarray(t, np.int32) for row, t in tapes.items()}


def _seeds(n):
  return [13 * i + 2 for i in range(n)]


@functools.lru_cache(maxsize=None)
def _reference(n, key):
  """The oracle playing each sampled env's own action sequence (key: the world's constructor arguments), computed once per world."""
  kw = dict(key)
  if kw.pop('other_rules', False):
    kw['rules'] = _other_rules()
  sample, _ = _schedule(n)
  tapes = _own_tapes(n)
  seeds = _seeds(n)
  return oracle_rollouts([{'kwargs': dict(seed=seeds[row], length=LENGTH, **kw), 'auto_reset': True, 'actions': tapes[row]} for row in sample])


# name: (envs, BatchedEnv / oracle arguments, environment, the step instance)
KERNELS = {
    'wide': (40, {}, {}, 'crafter_step_kernel<1, 1, 1>'),
    'fused-111': (40, {}, {'CRAFTER_STEP_WIDE': '0'}, 'crafter_step_kernel<1, 1, 1>'),
    'fused-110': (40, {'other_rules': True}, {}, 'crafter_step_kernel<1, 1, 0>'),
    'fused-100': (40, {'area': (32, 32)}, {}, 'crafter_step_kernel<1, 0, 0>'),
    'fused-021': (24, {'area': (256, 256)}, {}, 'crafter_step_kernel<0, 2, 1>'),
    'fused-000': (40, {'area': (256, 256), 'view': (7, 9), 'size': (84, 72)}, {}, 'crafter_step_kernel<0, 0, 0>'),
    'wide-no-pool': (40, {}, {}, 'crafter_step_kernel<1, 1, 1>'),
}


@pytest.mark.parametrize('name', list(KERNELS))
def test_own_pace_equals_the_oracle(name, monkeypatch):
  """Every env lives at its own pace: whatever subsets it was stepped in, its obs / reward / done at each of ITS steps and its
  state at the end are the oracle's of its seed playing its own actions, auto-resets included."""
  n, kw, environ, instance = KERNELS[name]
  for k, v in environ.items():
    monkeypatch.setenv(k, v)
  sample, calls = _schedule(n)
  tapes = _own_tapes(n)
  want = _reference(n, tuple(sorted(kw.items())))
  for row, w in zip(sample, want):
    assert len(tapes[row]) >= 45 and sum(w['done']) >= 2, (row, len(tapes[row]), sum(w['done']))
  env_kw = {k: v for k, v in kw.items() if k != 'other_rules'}
  if kw.get('other_rules'):
    env_kw['rules'] = _other_rules()
  env = _batched(n, seeds=_seeds(n), length=LENGTH, gen_period=-1 if name == 'wide-no-pool' else 0, **env_kw)
  assert env.step_instance == instance
  assert env.pool_status(stats=False)['state'] == ('off' if name == 'wide-no-pool' else 'running')
  env.reset()
  got = {row: ([], [], []) for row in sample}
  for idx, acts in calls:
    obs, reward, done, _ = env.step_envs(_dev(idx, env), _dev(acts, env), info=False)
    rows = [i for i in idx.tolist() if i in got]
    if rows:
      o, r, d = obs[rows].cpu().numpy(), reward[rows].cpu().numpy(), done[rows].cpu().numpy()
      for j, row in enumerate(rows):
        got[row][0].append(sha8(o[j])), got[row][1].append(np.float32(r[j])), got[row][2].append(bool(d[j]))
  for row, w in zip(sample, want):
    assert got[row][2] == w['done'], f'{name}: done of env {row}'
    assert got[row][1] == w['reward'], f'{name}: reward of env {row}'
    assert got[row][0] == w['obs_sha'], f'{name}: obs of env {row}'
    assert_same(env.snapshot(row), w['final_snapshot'], f'{name}: env {row} at the end')
  env.check_errors()


def test_unnamed_rows_are_untouched():
  from crafter_amd import state
  n = 64
  env = _batched(n, seeds=_seeds(n), length=LENGTH, semantic=True)
  env.reset()
  rs = np.random.RandomState(3)
  for _ in range(30):
    env.step(_dev(rs.randint(0, 17, n), env), info=False)
  per_env = {k: v for k, v in env.state.items() if k not in state.POOL_BUFFERS and k != 'reset_q'}
  assert {'mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'terminal', 'semantic'} <= set(per_env)
  assert all(v.shape[0] == n for v in per_env.values())
  per_env.update(obs=env.obs, reward=env.reward, done=env.done)
  before = {k: v.clone() for k, v in per_env.items()}
  idx = rs.choice(n, 9, replace=False)
  rest = torch.from_numpy(np.setdiff1d(np.arange(n), idx)).to(env.device)
  env.step_envs(_dev(idx, env), _dev(rs.randint(1, 5, 9), env), info=False)
  for k, v in per_env.items():
    assert torch.equal(v[rest], before[k][rest]), k
  named = torch.from_numpy(idx).to(env.device)
  assert not torch.equal(env.state['rec'][named], before['rec'][named])
  step = env.info()['step']
  assert int((step != before['rec'].view(torch.int32)[:, env._off['step']]).sum()) == 9
  env.check_errors()


def test_partition_and_mixing_on_an_ordered_handle():
  """1536 envs keep a dispatch order.  A batch stepped whole and one stepped by step(), by one step_envs call over a permutation
  or by two over complementary halves, in turn, stay equal: outputs every round, the saved state at the end, a rollout after it."""
  n, rounds = 1536, 40
  a, b = (_batched(n, seeds=_seeds(n), length=LENGTH) for _ in range(2))
  a.reset(), b.reset()
  rs = np.random.RandomState(11)
  for t in range(rounds):
    acts = rs.randint(0, 17, n).astype(np.int32)
    a.step(_dev(acts, a), info=False)
    way = t % 3
    if way == 0:
      b.step(_dev(acts, b), info=False)
    elif way == 1:
      perm = rs.permutation(n)
      b.step_envs(_dev(perm, b), _dev(acts[perm], b), info=False)
    else:
      perm = rs.permutation(n)
      k = int(rs.randint(1, n))
      for half in (perm[:k], perm[k:]):
        b.step_envs(_dev(half, b), _dev(acts[half], b), info=False)
    assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done), t
  sa, sb = a.save_state().tensors, b.save_state().tensors
  assert set(sa) == set(sb)
  for k in sa:
    assert torch.equal(sa[k], sb[k]), k
  tape = _dev(rs.randint(0, 17, (16, n)), a)
  ra, rb = a.rollout(tape), b.rollout(tape)
  for x, y in zip(ra, rb):
    assert torch.equal(x, y)
  order = b.dispatch_order()
  assert order is not None and np.array_equal(np.sort(order), np.arange(n))
  assert int(a.info()['episode'].min()) >= 2
  a.check_errors(), b.check_errors()


def test_refusals():
  from crafter_amd import CrafterDeviceError
  n = 16
  env = _batched(n, seeds=_seeds(n), length=LENGTH)
  env.reset()
  env.step(_dev(np.full(n, 5), env), info=False)
  with pytest.raises(ValueError):
    env.step_envs([1, 2, 1], [0, 0, 0])
  with pytest.raises(ValueError):
    env.step_envs([1, n], [0, 0])
  with pytest.raises(ValueError):
    env.step_envs([1, 2], [0, 0, 0])
  with pytest.raises(ValueError):
    env.step_envs(_dev([1, 2], env), _dev([0], env))
  env.check_errors()
  for bad in ([4, 9, 4], [4, n, 9]):
    before = {k: v.clone() for k, v in env.state.items()}
    out = env.obs.clone(), env.reward.clone(), env.done.clone()
    env.step_envs(_dev(bad, env), _dev([5, 5, 5], env), info=False)
    with pytest.raises(CrafterDeviceError, match='ST_BAD_COPY'):
      env.check_errors()
    status = env._rec_i32[:, env._off['status']]
    assert sorted(torch.nonzero(status).flatten().tolist()) == [4, 9] and int(status[4]) == 64
    status.zero_()
    for k, v in env.state.items():
      assert torch.equal(v, before[k]), k
    assert torch.equal(env.obs, out[0]) and torch.equal(env.reward, out[1]) and torch.equal(env.done, out[2])
  obs, _, _, info = env.step_envs(_dev([4, 9], env), _dev([5, 5], env))   # and the handle steps on
  assert info['step'][4] == 2 and info['step'][3] == 1
  env.check_errors()
