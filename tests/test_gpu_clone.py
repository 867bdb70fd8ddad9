"""Copies of environments on the device (BatchedEnv.copy_envs / save_state / load_state, crafter_amd.Env deepcopy / pickle)
against the oracle: a copy of env s taken after tape A[:k] and stepped with tape B is the oracle of seed(s) playing
A[:k, s] ++ B, later episodes included; the source and the envs not named are unaffected."""
import copy
import gc
import pickle

import numpy as np
import pytest
import torch

from tests.parity import assert_same, sha8
from tests.rollout import oracle_rollouts

pytestmark = pytest.mark.gpu


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env):
  return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(env.device)


class _Recorder:
  """Per-step obs sha8 / reward / done of a few envs."""

  def __init__(self, rows):
    self.rows = [int(r) for r in rows]
    self.sha, self.reward, self.done = {r: [] for r in self.rows}, {r: [] for r in self.rows}, {r: [] for r in self.rows}

  def add(self, obs, reward, done):
    o, r, d = obs[self.rows].cpu().numpy(), reward[self.rows].cpu().numpy(), done[self.rows].cpu().numpy()
    for i, row in enumerate(self.rows):
      self.sha[row].append(sha8(o[i]))
      self.reward[row].append(np.float32(r[i]))
      self.done[row].append(bool(d[i]))


def _check_tail(rec, row, want, first, where):
  """The recorded steps of `row` from step `first` on against the oracle's run `want`."""
  got_n = len(rec.sha[row]) - first
  assert got_n > 0
  assert rec.sha[row][first:] == want['obs_sha'][first:first + got_n], f'{where}: obs'
  assert rec.reward[row][first:] == want['reward'][first:first + got_n], f'{where}: reward'
  assert rec.done[row][first:] == want['done'][first:first + got_n], f'{where}: done'


def _branch(n, area=(64, 64), semantic=False, length=20, k=30, after=70, use_rollout=False, seed0=0):
  """Steps n envs through tape A (with manual resets of half of them at steps 2 and k // 2, so that episode numbers differ), copies
  envs of the reset half onto envs of the other half, and runs tape B; checks the sampled envs against the oracle."""
  seeds = [seed0 + 11 * i + 3 for i in range(n)]
  env = _batched(n, area=area, seeds=seeds, length=length, semantic=semantic)
  rs = np.random.RandomState(n + seed0)
  A = rs.randint(0, 17, (k, n)).astype(np.int32)
  B = rs.randint(0, 17, (after, n)).astype(np.int32)
  mask = rs.rand(n) < 0.5
  r_at = k // 2
  pairs = max(4, n // 16)
  src = rs.permutation(np.nonzero(mask)[0])[:pairs]
  dst = rs.permutation(np.nonzero(~mask)[0])[:pairs]
  others = np.setdiff1d(np.arange(n), np.concatenate([src, dst]))
  sample = list(dst[:5]) + list(src[:2]) + list(rs.permutation(others)[:2])
  rec = _Recorder(sample)
  env.reset()
  for t in range(k):
    rec.add(*env.step(_dev(A[t], env), info=False)[:3])
    if t in (2, r_at):
      env.reset(_dev(mask, env).to(torch.uint8))
  r = env.records()
  assert (r['episode'][src] != r['episode'][dst]).all()
  assert (r['nobj'][dst] > r['nobj'][src]).any(), 'no destination held more objects than its source'
  rec_before = env.state['rec'].clone()
  env.copy_envs(src, dst)
  assert torch.equal(env.obs[dst], env.obs[src])
  if semantic:
    sem = env.info()['semantic']
    assert torch.equal(sem[dst], sem[src])
  r2 = env.state['rec']
  assert torch.equal(r2[dst], r2[src]) and torch.equal(r2[others], rec_before[others]) and torch.equal(r2[src], rec_before[src])
  if use_rollout:
    o, rw, d = env.rollout(_dev(B, env))
    for t in range(after):
      rec.add(o[t], rw[t], d[t])
  else:
    for t in range(after):
      rec.add(*env.step(_dev(B[t], env), info=False)[:3])
  source = {int(d_): int(s_) for s_, d_ in zip(src, dst)}
  specs = []
  for row in sample:
    s = source.get(row, row)
    specs.append({'kwargs': dict(seed=seeds[s], length=length, area=area), 'auto_reset': True,
                  'actions': np.concatenate([A[:, s], B[:, row]]), 'reset_at': [2, r_at] if mask[s] else []})
  want = oracle_rollouts(specs)
  for row, w in zip(sample, want):
    _check_tail(rec, row, w, k, f'env {row} (copy of {source.get(row, row)})')
    assert_same(env.snapshot(row), w['final_snapshot'], f'env {row} at the end')
    if row in source:
      assert sum(w['done'][k:]) >= 3, 'a copy must pass three episode ends'
  env.check_errors()
  return env


@pytest.mark.parametrize('n', [4096, 1024, 256])
def test_copy_envs_each_default_instance(n):
  """4096: crafter_step_early_kernel, 1024: the default kernel, 256: crafter_step_wide_kernel; pool on."""
  env = _branch(n)
  assert env.pool_status()['state'] == 'running'


def test_copy_envs_large_world_semantic():
  """crafter_step_kernel<0, 2, 1>: objmap in HBM, holes in the slot table, semantic on."""
  env = _branch(1024, area=(256, 256), semantic=True, length=20, k=12, after=62)
  assert not env.slot_map_derived


def test_rollout_after_copy_envs():
  _branch(512, length=20, k=20, after=64, use_rollout=True, seed0=5)


def test_clone_under_load_follows_lineage():
  """4096 envs, episodes of 20 steps (requests always queued and in flight): a fresh disjoint set of clones every 3 steps,
  no synchronisation of the test's own; every env's lineage (seed, actions) is tracked through the clones."""
  n, T, length = 4096, 210, 20
  seeds = [7 * i + 1 for i in range(n)]
  env = _batched(n, seeds=seeds, length=length)
  rs = np.random.RandomState(17)
  lineage = [(s, []) for s in seeds]
  last_copy = np.zeros(n, np.int64)
  sample = rs.choice(n, 24, replace=False)
  rec = _Recorder(sample)
  env.reset()
  adopted0 = None
  for t in range(T):
    if t % 3 == 2:
      perm = rs.permutation(n)
      src, dst = perm[:64], perm[64:128]
      env.copy_envs(_dev(src, env), _dev(dst, env))
      for s, d in zip(src, dst):
        lineage[d] = (lineage[s][0], list(lineage[s][1]))
        last_copy[d] = t
      if adopted0 is None:
        adopted0 = env.pool_status()['adopted']
    a = rs.randint(0, 17, n).astype(np.int32)
    rec.add(*env.step(_dev(a, env), info=False)[:3])
    for i in range(n):
      lineage[i][1].append(int(a[i]))
  specs = [{'kwargs': dict(seed=lineage[i][0], length=length), 'auto_reset': True, 'actions': np.array(lineage[i][1])}
           for i in sample]
  want = oracle_rollouts(specs)
  for i, w in zip(sample, want):
    first = int(last_copy[i])
    tail = len(lineage[i][1]) - (T - first)
    got = rec.sha[i][first:]
    assert got == w['obs_sha'][tail:], f'env {i}: obs after its last copy'
    assert rec.reward[i][first:] == w['reward'][tail:] and rec.done[i][first:] == w['done'][tail:], f'env {i}'
    assert_same(env.snapshot(int(i)), w['final_snapshot'], f'env {i}')
  assert env.pool_status()['adopted'] > adopted0
  env.check_errors()


def test_save_run_load_rerun_through_the_night():
  n, k, T = 64, 140, 160
  seeds = [31 * i + 5 for i in range(n)]
  env = _batched(n, seeds=seeds)
  rs = np.random.RandomState(3)
  A = rs.randint(0, 17, (k + T, n)).astype(np.int32)
  env.reset()
  for t in range(k):
    env.step(_dev(A[t], env), info=False)
  store = env.save_state()

  def run():
    outs, frames = [], []
    for t in range(T):
      o, r, d, _ = env.step(_dev(A[k + t], env), info=False)
      outs.append((o.clone(), r.clone(), d.clone()))
      if t % 10 == 9:
        frames.append(env.render((512, 512)).clone())
    return outs, frames, [env.snapshot(i) for i in range(0, n, 9)]

  first = run()
  env.load_state(store)
  second = run()
  for (o1, r1, d1), (o2, r2, d2) in zip(first[0], second[0]):
    assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
  for f1, f2 in zip(first[1], second[1]):
    assert torch.equal(f1, f2)
  for s1, s2 in zip(first[2], second[2]):
    assert_same(s2, s1, 'second pass')
  env.check_errors()
  from oracle.crafter_oracle import OracleEnv
  for i in (0, 27):
    o = OracleEnv(seed=seeds[i])
    o.reset()
    nights = 0
    for t in range(k + T):
      ob, _, d, _ = o.step(int(A[t, i]))
      if d:   # the batch resets on its own
        ob = o.reset()
      if t >= k:
        nights += o.daylight < 0.5
        assert sha8(ob) == sha8(second[0][t - k][0][i].cpu().numpy()), (i, t)
        if (t - k) % 10 == 9:
          assert np.array_equal(o.render((512, 512)), second[1][(t - k) // 10][i].cpu().numpy()), (i, t)
    assert nights > 0, 'the rerun never reached the night'
    assert_same(env.snapshot(i), o.snapshot(), f'env {i}')


def test_load_across_batches_rows_and_slot_tables():
  k, after = 25, 30
  a_seeds = [100 + i for i in range(64)]
  b_seeds = [900 + i for i in range(256)]
  rs = np.random.RandomState(5)
  A = rs.randint(0, 17, (k, 64)).astype(np.int32)
  B = rs.randint(0, 17, (after, 256)).astype(np.int32)
  for a_max, b_max in ((256, 256), (256, 512), (512, 256)):
    ea = _batched(64, seeds=a_seeds, length=40, max_objects=a_max)
    eb = _batched(256, seeds=b_seeds, length=40, max_objects=b_max)
    ea.reset()
    eb.reset()
    for t in range(k):
      ea.step(_dev(A[t], ea), info=False)
      eb.step(_dev(rs.randint(0, 17, 256), eb), info=False)
    rows = np.array([3, 17, 40, 63])
    dst = np.array([200, 5, 77, 128])
    store = ea.save_state(rows)
    assert store.max_objects == a_max
    eb.load_state(store, dst)
    assert eb.cfg.max_objects == max(a_max, b_max)
    for s, d in zip(rows, dst):
      assert_same(eb.snapshot(int(d)), ea.snapshot(int(s)), f'loaded row {d}')
    assert torch.equal(eb.obs[dst], ea.obs[rows])
    rec = _Recorder(dst)
    for t in range(after):
      rec.add(*eb.step(_dev(B[t], eb), info=False)[:3])
    specs = [{'kwargs': dict(seed=a_seeds[s], length=40), 'auto_reset': True, 'actions': np.concatenate([A[:, s], B[:, d]])}
             for s, d in zip(rows, dst)]
    for (s, d), w in zip(zip(rows, dst), oracle_rollouts(specs)):
      assert rec.sha[d] == w['obs_sha'][k:] and rec.reward[d] == w['reward'][k:] and rec.done[d] == w['done'][k:], (a_max, b_max, d)
      assert_same(eb.snapshot(int(d)), w['final_snapshot'], f'{a_max}->{b_max} row {d}')
    eb.check_errors()


def test_env_deepcopy_and_pickle():
  import crafter_amd
  from oracle.crafter_oracle import OracleEnv
  rs = np.random.RandomState(9)
  A, B, C_ = rs.randint(0, 17, 30), rs.randint(0, 17, 50), rs.randint(0, 17, 50)
  env = crafter_amd.Env(seed=42, length=60)
  env.reset()
  for a in A:
    env.step(int(a))
  twin = copy.deepcopy(env)
  pick = pickle.loads(pickle.dumps(env))
  assert twin._episode == env._episode == pick._episode and twin._step == env._step == pick._step == 30
  assert twin._batch._handle.value != env._batch._handle.value

  def play(e, tape):
    out = []
    for t, a in enumerate(tape):
      ob, r, d, _ = e.step(int(a))
      out.append((sha8(ob), np.float32(r), bool(d)))
      if t == 20:
        out.append(sha8(e.render((512, 512))))
      if d:
        out.append(sha8(e.reset()))
    return out

  def oracle(tape):
    o = OracleEnv(seed=42, length=60)
    o.reset()
    for a in A:
      o.step(int(a))
    return play(o, tape), o

  got_env = play(env, B)
  want_env, _ = oracle(B)
  assert got_env == want_env
  del env
  gc.collect()
  got_twin = play(twin, C_)
  want_twin, o = oracle(C_)
  assert got_twin == want_twin
  assert_same(twin._batch.snapshot(0), o.snapshot(), 'deepcopy')
  assert play(pick, C_) == want_twin


def test_bad_indices_refused():
  from crafter_amd.batched import CrafterDeviceError
  env = _batched(32, seeds=list(range(32)), length=30)
  env.reset()
  for t in range(5):
    env.step(_dev(np.full(32, t % 17), env), info=False)
  for src, dst in (([0, 1], [2, 2]), ([0, 1], [1, 3]), ([0], [32]), ([-1], [3]), ([0, 1], [2])):
    with pytest.raises(ValueError):
      env.copy_envs(src, dst)
  before = [env.snapshot(i) for i in range(32)]
  obs = env.obs.clone()
  for src, dst in (([0, 1], [2, 2]), ([0, 1], [1, 3]), ([0], [40])):
    env.copy_envs(_dev(src, env), _dev(dst, env))
    for i in range(32):
      assert_same(env.snapshot(i), before[i], f'env {i} after a refused copy')
    assert torch.equal(env.obs, obs)
    with pytest.raises(CrafterDeviceError, match='ST_BAD_COPY'):
      env.check_errors()
    env.state['rec'].view(torch.int32)[:, env._off['status']] = 0
  store = env.save_state([0, 1])
  with pytest.raises(ValueError):
    env.load_state(store, [3, 3])
  env.load_state(store, _dev([4, 4], env))
  assert_same(env.snapshot(4), before[4], 'env 4 after a refused load')
  with pytest.raises(CrafterDeviceError, match='ST_BAD_COPY'):
    env.check_errors()
