"""BatchedEnv.rollout_envs / crafter_step_n_envs on the device: one rollout_envs call over a subset equals T step_envs calls over it
on a twin batch, on every rollout instance, with the pool, without it and out of pooled worlds; each env's own tape equals the
oracle's; rows that are not named stay bit-identical; a batch rolled out by subsets equals a batch rolled out whole on a handle
that keeps a dispatch order; bad index lists are refused on the host or, whole, on the device; and the planning loop the call
exists for."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests.parity import assert_same, sha8
from tests.rollout import oracle_rollouts
from tests.test_gpu_step_envs import KERNELS

pytestmark = pytest.mark.gpu

LENGTH = 20
CALLS = 40
SIZES = (1, 2, 7, 40)
STEPS = (1, 3, 16, 37)
SAMPLED = 6
ST_BAD_COPY = 64


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


def _seeds(n):
  return [13 * i + 2 for i in range(n)]


@functools.lru_cache(maxsize=None)
def _schedule(n, calls=CALLS):
  """-> (sample, calls): SAMPLED env rows and `calls` pairs (idx, actions [T, len(idx)]) of random subsets, sizes drawn from SIZES
  (40: every env, in a random order), T from STEPS.  The small subsets name sampled envs first, in turn."""
  rs = np.random.RandomState(2000 + n)
  sample = [int(v) for v in rs.choice(n, SAMPLED, replace=False)]
  others = np.setdiff1d(np.arange(n), sample)
  turn, out = 0, []
  for c in range(calls):
    size = SIZES[c % len(SIZES)] if c < 2 * len(SIZES) else int(rs.choice(SIZES))   # (every size and every T at least once)
    T = STEPS[(c // 2) % len(STEPS)] if c < 2 * len(STEPS) else int(rs.choice(STEPS))
    if size >= n or size == 40:
      idx = rs.permutation(n)
    else:
      k = min(size, 3)
      mine = [sample[(turn + j) % SAMPLED] for j in range(k)]
      turn += k
      idx = rs.permutation(np.concatenate([mine, rs.choice(others, size - k, replace=False)]).astype(np.int64))
    out.append((idx.astype(np.int32), rs.randint(0, 17, (T, len(idx))).astype(np.int32)))
  return sample, out


def _twin_call(a, b, idx, acts, obs=True):
  """Batch a: T step_envs calls over idx, rows idx gathered; batch b: one rollout_envs call.  -> b's outputs, asserted equal."""
  i_a, i_b = _dev(idx, a), _dev(idx, b)
  rows = i_a.long()
  acts_a = _dev(acts, a)
  want = ([], [], [])
  for t in range(acts.shape[0]):
    o, r, d, _ = a.step_envs(i_a, acts_a[t], info=False)
    want[0].append(o[rows]), want[1].append(r[rows]), want[2].append(d[rows])
  got = b.rollout_envs(i_b, _dev(acts, b), obs=obs)
  if obs:
    assert torch.equal(got[0], torch.stack(want[0])), 'obs'
  else:
    assert got[0] is None
  assert torch.equal(got[1], torch.stack(want[1])), 'reward'
  assert torch.equal(got[2], torch.stack(want[2])), 'done'
  return got


def _assert_same_state(a, b, outputs=False):
  """save_state() of both batches, key by key, every byte -- but for two things that differ by design, and nothing else.
  The rows of self.obs / self.reward / self.done, which step_envs() updates and rollout_envs() -- like rollout() -- does not:
  their content is compared call by call, and here only with outputs=True (neither batch was stepped by a call that updates them).
  And, in 'objs', the FREE records at and beyond each env's nobj: a step writes back the nobj records it leaves, so storage
  behind them keeps whatever was last stored there, which depends on when the table went back to global memory -- at every
  step, or at the end of every resident stretch, wherever the pool's period put it.  That holds between step() and rollout()
  too (measured: 40 envs, six 16-step calls: 115 free records differ and no live one, the same 115 for step_envs() x 16
  against rollout_envs(); rollout() against rollout_envs() with equal stretches: none), and no reader of the state looks there."""
  sa, sb = a.save_state().tensors, b.save_state().tensors
  assert set(sa) == set(sb)
  for k in sa:
    x, y = sa[k], sb[k]
    if k in ('obs', 'reward', 'done') and not outputs:
      continue
    if k == 'objs':
      nobj_a, nobj_b = (e._rec_i32[:, e._off['nobj']].long() for e in (a, b))
      assert torch.equal(nobj_a, nobj_b), 'nobj'
      live = torch.arange(x.shape[1], device=x.device)[None, :] < nobj_a[:, None]
      x, y = x[live], y[live]
    assert torch.equal(x, y), k


def _env_kwargs(kw):
  env_kw = {k: v for k, v in kw.items() if k != 'other_rules'}
  if kw.get('other_rules'):
    env_kw['rules'] = _other_rules()
  return env_kw


# ------------------------------------------------------------------ 1. the twin, instance by instance
@pytest.mark.parametrize('name', list(KERNELS))
def test_rollout_envs_equals_step_envs_calls(name, monkeypatch):
  """For every named env one rollout_envs call is T step_envs calls: each step's obs / reward / done, call after call, and the
  saved state at the end (_assert_same_state) -- episodes that end, and end twice, inside a stretch included."""
  n, kw, environ, instance = KERNELS[name]
  for k, v in environ.items():
    monkeypatch.setenv(k, v)
  sample, calls = _schedule(n)
  gen_period = -1 if name == 'wide-no-pool' else 0
  a, b = (_batched(n, seeds=_seeds(n), length=LENGTH, gen_period=gen_period, **_env_kwargs(kw)) for _ in range(2))
  assert a.step_instance == instance and b.step_instance == instance
  assert b.pool_status(stats=False)['state'] == ('off' if name == 'wide-no-pool' else 'running')
  a.reset(), b.reset()
  for c, (idx, acts) in enumerate(calls):
    try:
      _twin_call(a, b, idx, acts)
    except AssertionError as e:
      raise AssertionError(f'{name}: call {c} ({len(idx)} envs, T = {acts.shape[0]}): {e}') from e
  _assert_same_state(a, b)
  episodes = b.info()['episode'].cpu().numpy()
  assert all(episodes[row] >= 2 for row in sample), episodes[sample]
  a.check_errors(), b.check_errors()


# ------------------------------------------------------------------ 2. the oracle
ORACLE_CALLS = 16


def _own_tapes(n):
  sample, calls = _schedule(n, ORACLE_CALLS)
  tapes = {row: [] for row in sample}
  for idx, acts in calls:
    for j, i in enumerate(idx.tolist()):
      if i in tapes:
        tapes[i].extend(acts[:, j].tolist())
  return {row: np.asarray(t, np.int32) for row, t in tapes.items()}


@functools.lru_cache(maxsize=None)
def _reference(n):
  sample, _ = _schedule(n, ORACLE_CALLS)
  tapes = _own_tapes(n)
  seeds = _seeds(n)
  return oracle_rollouts([{'kwargs': dict(seed=seeds[row], length=LENGTH), 'auto_reset': True, 'actions': tapes[row]} for row in sample])


def test_own_tape_equals_the_oracle():
  """Whatever subsets and stretches an env was rolled out in, its obs / reward / done at each of ITS steps and its state at the
  end are the oracle's of its seed playing its own actions, auto-resets included."""
  n = 40
  sample, calls = _schedule(n, ORACLE_CALLS)
  tapes = _own_tapes(n)
  want = _reference(n)
  for row, w in zip(sample, want):
    assert len(tapes[row]) >= 45 and sum(w['done']) >= 2, (row, len(tapes[row]), sum(w['done']))
  env = _batched(n, seeds=_seeds(n), length=LENGTH)
  assert env.step_instance == 'crafter_step_kernel<1, 1, 1>'
  env.reset()
  got = {row: ([], [], []) for row in sample}
  for idx, acts in calls:
    obs, reward, done = env.rollout_envs(_dev(idx, env), _dev(acts, env))
    cols = [(j, i) for j, i in enumerate(idx.tolist()) if i in got]
    if cols:
      js = [j for j, _ in cols]
      o, r, d = obs[:, js].cpu().numpy(), reward[:, js].cpu().numpy(), done[:, js].cpu().numpy()
      for k, (_, row) in enumerate(cols):
        for t in range(acts.shape[0]):
          got[row][0].append(sha8(o[t, k])), got[row][1].append(np.float32(r[t, k])), got[row][2].append(bool(d[t, k]))
  for row, w in zip(sample, want):
    assert got[row][2] == w['done'], f'done of env {row}'
    assert got[row][1] == w['reward'], f'reward of env {row}'
    assert got[row][0] == w['obs_sha'], f'obs of env {row}'
    assert_same(env.snapshot(row), w['final_snapshot'], f'env {row} at the end')
  env.check_errors()


# ------------------------------------------------------------------ 3. out of pooled worlds
@pytest.mark.parametrize('name', ['short-episodes', 'no-pool'])
def test_envs_without_a_pooled_world(name):
  """Episodes of three steps outrun the pool, and without the pool every reset is inline: the envs stop in the rollout kernel
  and the regeneration kernel behind the stretch runs the rest of their steps, finding their compact rows through row_of."""
  n, T = 48, 40
  kw = dict(length=3) if name == 'short-episodes' else dict(length=LENGTH, gen_period=-1)
  a, b = (_batched(n, seeds=_seeds(n), **kw) for _ in range(2))
  a.reset(), b.reset()
  rs = np.random.RandomState(5)
  for c in range(5):
    idx = rs.choice(n, 17, replace=False)
    _twin_call(a, b, idx, rs.randint(0, 17, (T, 17)).astype(np.int32))
  _assert_same_state(a, b)
  status = b.pool_status()
  if name == 'short-episodes':
    assert status['state'] == 'running' and status['regenerated_inline'] > 0, status
  else:
    assert status['state'] == 'off'
  assert int(b.info()['episode'].max()) >= (10 if name == 'short-episodes' else 2)
  a.check_errors(), b.check_errors()


# ------------------------------------------------------------------ 4. rows that are not named
def test_unnamed_rows_are_untouched():
  from crafter_amd import state
  n, T = 64, 5
  env = _batched(n, seeds=_seeds(n), length=LENGTH, semantic=True)
  env.reset()
  rs = np.random.RandomState(3)
  for _ in range(30):
    env.step(_dev(rs.randint(0, 17, n), env), info=False)
  per_env = {k: v for k, v in env.state.items() if k not in state.POOL_BUFFERS and k != 'reset_q'}
  assert {'mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'terminal', 'semantic'} <= set(per_env)
  assert all(v.shape[0] == n for v in per_env.values())
  before = {k: v.clone() for k, v in per_env.items()}
  outputs = env.obs.clone(), env.reward.clone(), env.done.clone()
  idx = rs.choice(n, 9, replace=False)
  rest = torch.from_numpy(np.setdiff1d(np.arange(n), idx)).to(env.device)
  env.rollout_envs(_dev(idx, env), _dev(rs.randint(1, 5, (T, 9)), env))
  for k, v in per_env.items():
    assert torch.equal(v[rest], before[k][rest]), k
  assert torch.equal(env.obs, outputs[0]) and torch.equal(env.reward, outputs[1]) and torch.equal(env.done, outputs[2])
  named = torch.from_numpy(idx).to(env.device)
  step = env.info()['step']
  step_before = before['rec'].view(torch.int32)[:, env._off['step']]
  assert torch.equal(step[named], step_before[named] + T)
  assert int((step != step_before).sum()) == 9
  env.check_errors()


# ------------------------------------------------------------------ 5. a handle that keeps a dispatch order
def test_partition_and_mixing_on_an_ordered_handle():
  """1536 envs keep a dispatch order.  A batch rolled out whole and one rolled out by rollout(), by one rollout_envs call over a
  permutation or by two over complementary halves, in turn, stay equal: outputs every round, the saved state at the end, a
  step and a rollout after it."""
  n, rounds, T = 1536, 30, 3
  a, b = (_batched(n, seeds=_seeds(n), length=LENGTH) for _ in range(2))
  a.reset(), b.reset()
  rs = np.random.RandomState(11)
  for t in range(rounds):
    acts = rs.randint(0, 17, (T, n)).astype(np.int32)
    want = a.rollout(_dev(acts, a))
    way = t % 3
    if way == 0:
      got = b.rollout(_dev(acts, b))
    else:
      perm = rs.permutation(n)
      k = n if way == 1 else int(rs.randint(1, n))
      got = tuple(torch.empty_like(w) for w in want)
      for part in (perm[:k], perm[k:]):
        if len(part):
          rows = torch.from_numpy(part).to(b.device)
          for full, compact in zip(got, b.rollout_envs(_dev(part, b), _dev(acts[:, part], b))):
            full[:, rows] = compact
    for x, y in zip(want, got):
      assert torch.equal(x, y), t
  _assert_same_state(a, b, outputs=True)   # (neither batch's calls update self.obs / reward / done)
  acts = _dev(rs.randint(0, 17, n), a)
  for x, y in zip(a.step(acts, info=False)[:3], b.step(acts, info=False)[:3]):
    assert torch.equal(x, y)
  tape = _dev(rs.randint(0, 17, (16, n)), a)
  for x, y in zip(a.rollout(tape), b.rollout(tape)):
    assert torch.equal(x, y)
  order = b.dispatch_order()
  assert order is not None and np.array_equal(np.sort(order), np.arange(n))
  assert int(a.info()['episode'].min()) >= 2
  a.check_errors(), b.check_errors()


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
  from crafter_amd import CrafterDeviceError
  n, T = 16, 4
  env = _batched(n, seeds=_seeds(n), length=LENGTH)
  env.reset()
  env.step(_dev(np.full(n, 5), env), info=False)
  with pytest.raises(ValueError):
    env.rollout_envs([1, 2, 1], np.zeros((T, 3), np.int32))        # an env named twice
  with pytest.raises(ValueError):
    env.rollout_envs([1, n], np.zeros((T, 2), np.int32))           # out of range
  with pytest.raises(ValueError):
    env.rollout_envs([1, 2], np.zeros((T, 3), np.int32))           # actions of another width
  with pytest.raises(ValueError):
    env.rollout_envs(_dev([1, 2], env), _dev(np.zeros((T, 2, 1)), env))
  with pytest.raises(ValueError):
    env.rollout_envs([1, 2], np.zeros((0, 2), np.int32))           # T == 0
  env.check_errors()
  for bad in ([4, 9, 4], [4, n, 9]):
    before = {k: v.clone() for k, v in env.state.items()}
    outputs = env.obs.clone(), env.reward.clone(), env.done.clone()
    out = (torch.full((T, 3) + tuple(env.obs.shape[1:]), 0xA5, dtype=torch.uint8, device=env.device),
           torch.full((T, 3), -7.5, dtype=torch.float32, device=env.device), torch.full((T, 3), 0xA5, dtype=torch.uint8, device=env.device))
    got = env.rollout_envs(_dev(bad, env), _dev(np.full((T, 3), 5), env), out=out)
    assert all(x is y for x, y in zip(got, out))
    with pytest.raises(CrafterDeviceError, match='ST_BAD_COPY'):
      env.check_errors()
    status = env._rec_i32[:, env._off['status']]
    assert sorted(torch.nonzero(status).flatten().tolist()) == [4, 9] and int(status[4]) == ST_BAD_COPY and int(status[9]) == ST_BAD_COPY
    status.zero_()
    for k, v in env.state.items():
      assert torch.equal(v, before[k]), k
    assert bool((out[0] == 0xA5).all()) and bool((out[1] == -7.5).all()) and bool((out[2] == 0xA5).all())
    assert torch.equal(env.obs, outputs[0]) and torch.equal(env.reward, outputs[1]) and torch.equal(env.done, outputs[2])
  env.rollout_envs(_dev([9, 4], env), _dev(np.full((T, 2), 5), env))   # and the handle steps on
  step = env.info()['step']
  assert step[4] == 1 + T and step[9] == 1 + T and step[3] == 1
  env.check_errors()


# ------------------------------------------------------------------ 7. the surface
def test_surface():
  n, T = 32, 6
  rs = np.random.RandomState(9)
  a, b, c = (_batched(n, seeds=_seeds(n), length=LENGTH, render=render) for render in (True, True, False))
  for env in (a, b, c):
    env.reset()
  idx = rs.choice(n, 11, replace=False)
  acts = rs.randint(0, 17, (T, 11)).astype(np.int32)
  # obs=False and render=False: no frames, the same rewards and dones
  o, r, d = a.rollout_envs(_dev(idx, a), _dev(acts, a))
  assert o.shape == (T, 11) + tuple(a.obs.shape[1:]) and o.dtype == torch.uint8 and r.shape == (T, 11) and d.shape == (T, 11)
  o2, r2, d2 = b.rollout_envs(_dev(idx, b), _dev(acts, b), obs=False)
  o3, r3, d3 = c.rollout_envs(idx, acts)   # (host arguments)
  assert o2 is None and o3 is None
  assert torch.equal(r, r2) and torch.equal(d, d2) and torch.equal(r, r3) and torch.equal(d, d3)
  # out= tensors are written and returned as given
  out = tuple(torch.zeros_like(x) for x in (o, r, d))
  got = b.rollout_envs(_dev(idx, b), _dev(acts, b), out=out)
  want = a.rollout_envs(_dev(idx, a), _dev(acts, a))
  assert all(x is y for x, y in zip(got, out))
  for x, y in zip(got, want):
    assert torch.equal(x, y)
  with pytest.raises(ValueError):
    b.rollout_envs(_dev(idx, b), _dev(acts, b), out=(out[0], out[1][:, :5], out[2]))
  with pytest.raises(ValueError):
    b.rollout_envs(_dev(idx, b), _dev(acts, b), out=(out[0], out[1].double(), out[2]))
  # T == 1, actions [n]: step_envs on a twin
  for _ in range(25):
    idx = rs.choice(n, 5, replace=False)
    one = rs.randint(0, 17, 5).astype(np.int32)
    obs, reward, done, _ = a.step_envs(_dev(idx, a), _dev(one, a), info=False)
    o, r, d = b.rollout_envs(_dev(idx, b), _dev(one, b))
    rows = _dev(idx, a).long()
    assert o.shape[:2] == (1, 5) and torch.equal(o[0], obs[rows]) and torch.equal(r[0], reward[rows]) and torch.equal(d[0], done[rows])
  _assert_same_state(a, b)
  # an empty idx enqueues nothing
  before = {k: v.clone() for k, v in b.state.items()}
  launched = b.pool_status(stats=False)['launched']
  o, r, d = b.rollout_envs([], np.zeros((T, 0), np.int32))
  assert o.shape[:2] == (T, 0) and r.shape == (T, 0) and d.shape == (T, 0)
  torch.cuda.synchronize()
  for k, v in b.state.items():
    assert torch.equal(v, before[k]), k
  assert b.pool_status(stats=False)['launched'] == launched
  a.check_errors(), b.check_errors(), c.check_errors()


# ------------------------------------------------------------------ 8. the loop it exists for
def test_random_shooting_planner():
  """Eight roots of a 256-env batch plan by random shooting: each round clones every root into eight scratch rows, plays a
  12-step random tape in each (one rollout_envs call, no frames), takes the first action of the tape with the largest return,
  and steps the roots with it -- everything on the device.  A twin playing the tapes with 12 step_envs calls chooses the same
  actions and ends in the same state."""
  n, depth, rounds, cands = 256, 12, 6, 8
  roots = np.array([3, 40, 77, 90, 101, 200, 230, 255], np.int32)
  scratch = np.arange(128, 128 + len(roots) * cands, dtype=np.int32)
  src = np.repeat(roots, cands)
  rs = np.random.RandomState(21)
  envs = [_batched(n, seeds=_seeds(n), length=LENGTH) for _ in range(2)]
  warm = rs.randint(0, 17, (10, n)).astype(np.int32)   # (the roots ten steps into their episodes: the playouts cross the episode's end)
  for env in envs:
    env.reset()
    env.rollout(_dev(warm, env), obs=False)
  chosen = ([], [])
  for _ in range(rounds):
    tape = rs.randint(0, 17, (depth, len(scratch))).astype(np.int32)
    outs = []
    for which, env in enumerate(envs):
      assert env.pool_status(stats=False)['state'] == 'running'
      tape_d, scratch_d, roots_d = _dev(tape, env), _dev(scratch, env), _dev(roots, env)
      env.copy_envs(_dev(src, env), scratch_d)
      if which == 0:
        reward = env.rollout_envs(scratch_d, tape_d, obs=False)[1]
      else:
        rows = scratch_d.long()
        reward = torch.stack([env.step_envs(scratch_d, tape_d[t], info=False)[1][rows] for t in range(depth)])
      best = reward.sum(0).view(len(roots), cands).argmax(1)
      action = tape_d[0].view(len(roots), cands).gather(1, best[:, None]).flatten().contiguous()
      chosen[which].append(action.clone())
      obs, reward, done, _ = env.step_envs(roots_d, action, info=False)
      rows = roots_d.long()
      outs.append((obs[rows].clone(), reward[rows].clone(), done[rows].clone()))
    for x, y in zip(*outs):
      assert torch.equal(x, y)
  assert torch.equal(torch.stack(chosen[0]), torch.stack(chosen[1]))
  _assert_same_state(*envs)
  episodes = envs[0].info()['episode'].cpu().numpy()
  assert episodes[scratch].max() >= 1   # (a playout ran over an episode's end)
  for env in envs:
    assert env.pool_status(stats=False)['state'] == 'running'
    env.check_errors()
