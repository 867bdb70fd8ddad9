"""Level selection on the device (BatchedEnv.reseed / reset(seeds=, episodes=) / levels(), crafter_amd.Env.reset(seed=),
VecEnvView.reseed): a reseeded env is bit for bit the env that was constructed with that seed, across episode ends and with the
world pool serving it again; envs not named are untouched; and the levels are the oracle's."""
import copy
import multiprocessing as mp

import numpy as np
import pytest
import torch

from tests.parity import assert_same, sha8

pytestmark = pytest.mark.gpu

LENGTH = 20   # episode ends, and with them pool adoptions, every few steps


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **{**dict(length=LENGTH), **k})


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def _tape(seed, steps, n):
  return np.random.RandomState(seed).randint(0, 17, (steps, n)).astype(np.int32)


def _seeds(n):
  """(the levels under test, the seeds a batch has before it is reseeded)"""
  return [5 * i + 2 for i in range(n)], [7 * i + 100001 for i in range(n)]


def _run(env, tape):
  for a in tape:
    env.step(_dev(a, env), info=False)


def _pool_episodes(env):
  """[2, N] episode number each pool entry holds (0: empty), once every batch in flight has landed."""
  torch.cuda.synchronize(env.device)
  from crafter_amd import abi
  hdr = env.state['pool_hdr'].cpu().numpy().view(abi.POOL_HDR_DTYPE).reshape(2, env.num_envs)
  return np.where(hdr['ready'] >> np.uint64(32) != 0, hdr['ready'] & np.uint64(0xFFFFFFFF), 0).astype(np.int64)


def _assert_rows_equal(a, b, rows_a, rows_b=None, where=''):
  """rec, mat, mt and the slot table up to nobj of a's rows_a against b's rows_b."""
  rows_b = rows_a if rows_b is None else rows_b
  ia, ib = torch.as_tensor(rows_a, device=a.device), torch.as_tensor(rows_b, device=b.device)
  for name in ('rec', 'mat', 'mt'):
    assert torch.equal(a.state[name][ia], b.state[name][ib]), f'{where}: {name}'
  nobj = a._rec_i32[ia, a._off['nobj']]
  live = (torch.arange(a.cfg.max_objects, device=a.device)[None, :] < nobj[:, None])[:, :, None]
  assert torch.equal(a.state['objs'][ia] * live, b.state['objs'][ib] * live), f'{where}: objs'


def _follow(pairs, tape, ends=None, on_step=None):
  """Steps every batch of `pairs` [(batch, reference batch, rows or None)] through `tape`; batch[rows] must equal reference[rows]
  in obs / reward / done at every step."""
  envs = []
  for b, ref, _ in pairs:
    for e in (b, ref):
      if all(e is not x for x in envs):
        envs.append(e)
  for t, a in enumerate(tape):
    for e in envs:
      e.step(_dev(a, e), info=False)
    for b, ref, rows in pairs:
      for name in ('obs', 'reward', 'done'):
        x, y = getattr(b, name), getattr(ref, name)
        if rows is not None:
          x, y = x[rows], y[rows]
        assert torch.equal(x, y), f'step {t}: {name}'
    if ends is not None:
      ends += pairs[0][0].done.to(torch.int64)
    if on_step:
      on_step(t)


def _equivalence(n, area=(64, 64), pre=25, post=70, min_ends=3, old_episode=2):
  S, other = _seeds(n)
  A = _batched(n, area=area, seeds=S)
  A.reset()
  B = _batched(n, area=area, seeds=other)
  B.reset()
  _run(B, _tape(n, pre, n))
  # the stale-entry case: B's entries hold worlds of the OLD seeds under the numbers A's episodes 2 .. 4 carry
  assert B.records()['episode'].min() == old_episode
  held = _pool_episodes(B)
  assert (((held >= 2) & (held <= 4)).any(axis=0)).all(), 'a row of B holds no pooled world numbered 2 .. 4'
  assert (B.state['gen_latest'].cpu().numpy() >= 3).all()
  obs = B.reset(seeds=S)
  assert B.seeds == S
  assert torch.equal(obs, A.obs)
  ends = torch.zeros(n, dtype=torch.int64, device=B.device)
  adopted = {}

  def note(t):
    if t == post - 41:
      adopted['before'] = B.pool_status()['adopted']
  _follow([(B, A, None)], _tape(n + 1, post, n), ends, note)
  _assert_rows_equal(B, A, np.arange(n), where='at the end')
  assert int(ends.min()) >= min_ends, f'a row passed only {int(ends.min())} episode ends'
  ps = B.pool_status()
  assert ps['state'] == 'running'
  assert ps['adopted'] > adopted['before'], 'no env of B adopted a pooled world in the last 40 steps: the pool did not come back'
  A.check_errors()
  B.check_errors()
  return A, B


# ------------------------------------------------------------------ 1. equivalence, pool on
@pytest.mark.parametrize('n', [256, 1024])
def test_reset_with_seeds_equals_a_batch_constructed_with_them(n):
  """256: crafter_step_wide_kernel, 1024: the default kernel.  B (other seeds, 25 steps in: episodes 2 - 3, its pool two worlds
  ahead) is reset to A's seeds; from there every row of B is A's, over at least three episode ends, and the pool serves it."""
  _equivalence(n)


# ------------------------------------------------------------------ 2. partial mask
def test_partial_mask_leaves_the_other_rows_alone():
  n = 256
  S, other = _seeds(n)
  A = _batched(n, seeds=S)
  A.reset()
  B, ctl = _batched(n, seeds=other), _batched(n, seeds=other)
  pre = _tape(n, 25, n)
  for e in (B, ctl):
    e.reset()
    _run(e, pre)
  mask = (np.arange(n) % 2 == 0).astype(np.uint8)
  named, unnamed = np.nonzero(mask)[0], np.nonzero(mask == 0)[0]
  junk = [s if m else 'not read' for s, m in zip(S, mask)]
  B.reset(mask, seeds=junk)
  ctl.reset(_dev(mask, ctl, np.uint8))
  assert [B.seeds[i] for i in named] == [S[i] for i in named] and [B.seeds[i] for i in unnamed] == [other[i] for i in unnamed]
  dn, du = _dev(named, B, np.int64), _dev(unnamed, B, np.int64)
  assert torch.equal(B.obs[dn], A.obs[dn]) and torch.equal(B.obs[du], ctl.obs[du])
  ends = torch.zeros(n, dtype=torch.int64, device=B.device)
  _follow([(B, A, dn), (B, ctl, du)], _tape(n + 1, 70, n), ends)
  assert int(ends.min()) >= 3
  _assert_rows_equal(B, A, named, where='named rows')
  _assert_rows_equal(B, ctl, unnamed, where='unnamed rows')
  assert B.pool_status()['state'] == 'running'
  for e in (A, B, ctl):
    e.check_errors()


# ------------------------------------------------------------------ 3. against the oracle
def _oracle_level(job):
  """OracleEnv(seed) from its episode-th reset(): first obs hash, then per step obs hash / reward / done, and the final snapshot."""
  seed, episode, actions = job
  from oracle.crafter_oracle import OracleEnv
  env = OracleEnv(seed=seed, length=LENGTH)
  env._episode = episode - 1
  out = {'reset_sha': sha8(env.reset()), 'sha': [], 'reward': [], 'done': []}
  for a in actions:
    obs, r, d, _ = env.step(int(a))
    if d:
      obs = env.reset()
    out['sha'].append(sha8(obs))
    out['reward'].append(np.float32(r))
    out['done'].append(bool(d))
  out['snapshot'] = env.snapshot()
  return out


def test_reseeded_levels_are_the_oracles():
  from tests.rollout import _worker_init
  n, steps = 64, 60
  rows = [1, 8, 23, 40, 41, 63]
  levels = [(-7, 1), ('a level', 2), (12345, 5), (0, 1), (2 ** 40 + 3, 2), (977, 5)]   # (seed, episode)
  tape = _tape(3, steps, n)
  jobs = [(s, k, tape[:, r]) for r, (s, k) in zip(rows, levels)]
  with mp.get_context('fork').Pool(len(jobs), initializer=_worker_init) as pool:   # (fork: the string seed hashes as it does here)
    want = pool.map_async(_oracle_level, jobs, chunksize=1).get(timeout=600)
  env = _batched(n, seeds=_seeds(n)[1])
  env.reset()
  _run(env, _tape(4, 7, n))
  seeds, episodes, mask = list(env.seeds), [1] * n, np.zeros(n, np.uint8)
  for r, (s, k) in zip(rows, levels):
    seeds[r], episodes[r], mask[r] = s, k, 1
  obs = env.reset(mask, seeds=seeds, episodes=episodes)
  got = obs[rows].cpu().numpy()
  for i, w in enumerate(want):
    assert sha8(got[i]) == w['reset_sha'], f'row {rows[i]}: first frame'
  assert env.records()['episode'][rows].tolist() == [k for _, k in levels]
  for t in range(steps):
    obs, reward, done, _ = env.step(_dev(tape[t], env), info=False)
    o, r, d = obs[rows].cpu().numpy(), reward[rows].cpu().numpy(), done[rows].cpu().numpy()
    for i, w in enumerate(want):
      assert sha8(o[i]) == w['sha'][t] and np.float32(r[i]) == w['reward'][t] and bool(d[i]) == w['done'][t], (rows[i], t)
  for i, w in enumerate(want):
    assert sum(w['done']) >= 2
    assert_same(env.snapshot(rows[i]), w['snapshot'], f'row {rows[i]} at the end')
  env.check_errors()


# ------------------------------------------------------------------ 4. reseed without reset
@pytest.mark.parametrize('use_rollout', [False, True], ids=['step', 'rollout'])
def test_reseed_takes_effect_at_the_next_auto_reset(use_rollout):
  """The episode in progress plays on as in a control batch; the auto-reset at its end starts (new seed, episode 1), and from there
  the row is A's -- A plays each row's tape from the step behind that row's episode end."""
  n, T = 256, 70
  S, other = _seeds(n)
  B, ctl = _batched(n, seeds=other), _batched(n, seeds=other)
  pre = _tape(n, 25, n)
  for e in (B, ctl):
    e.reset()
    _run(e, pre)
  episode_before = B.records()['episode']
  B.reseed(S)
  assert (B.records()['episode'] == 0).all() and (B.records()['step'] == ctl.records()['step']).all()
  tape = _tape(n + 1, T, n)

  def play(env, tp):
    if use_rollout:
      return env.rollout(_dev(tp, env))
    o, r, d = [], [], []
    for a in tp:
      obs, reward, done, _ = env.step(_dev(a, env), info=False)
      o.append(obs.clone()), r.append(reward.clone()), d.append(done.clone())
    return torch.stack(o), torch.stack(r), torch.stack(d)
  bo, br, bd = play(B, tape)
  co, cr, cd = play(ctl, tape)
  first = cd.to(torch.int64).argmax(dim=0).cpu().numpy()   # the step that ends the episode in progress
  assert cd.any(dim=0).all() and first.max() < LENGTH
  A = _batched(n, seeds=S)
  reset_obs = A.reset().clone()
  shifted = np.zeros_like(tape)
  for r in range(n):
    shifted[:T - first[r] - 1, r] = tape[first[r] + 1:, r]
  ao, ar, ad = play(A, shifted)
  for u in np.unique(first):
    rows = _dev(np.nonzero(first == u)[0], B, np.int64)
    where = f'rows whose episode ends at step {u}'
    assert torch.equal(bo[:u, rows], co[:u, rows]), f'{where}: obs of the episode in progress'
    assert torch.equal(br[:u + 1, rows], cr[:u + 1, rows]) and torch.equal(bd[:u + 1, rows], cd[:u + 1, rows]), where
    assert torch.equal(bo[u, rows], reset_obs[rows]), f'{where}: first frame of the new level'
    k = T - u - 1
    assert torch.equal(bo[u + 1:, rows], ao[:k, rows]), f'{where}: obs of the new level'
    assert torch.equal(br[u + 1:, rows], ar[:k, rows]) and torch.equal(bd[u + 1:, rows], ad[:k, rows]), where
    assert int(ad[:k, rows].sum(dim=0).min()) >= 2
  assert B.pool_status()['state'] == 'running'
  assert (episode_before >= 2).all()
  for e in (A, B, ctl):
    e.check_errors()


# ------------------------------------------------------------------ 5. large world
def test_large_world():
  """area (256, 256): maps and slot table in global memory (crafter_step_kernel<0, 2, 1>).  12 + 45 steps: B is in episode 1 when
  it is reseeded, its pool holds worlds 2 and 3 of the old seeds; 45 steps of 20-step episodes hold two episode ends."""
  A, B = _equivalence(64, area=(256, 256), pre=12, post=45, min_ends=2, old_episode=1)
  assert not B.slot_map_derived


# ------------------------------------------------------------------ 6. pool off / no auto-reset, and the facades
def test_without_auto_reset():
  n = 64
  S, other = _seeds(n)
  rs = np.random.RandomState(6)
  E = rs.randint(1, 4, size=n)
  A = _batched(n, seeds=S, auto_reset=False)
  for k in (1, 2, 3):   # row i is reset E[i] times: episode E[i] of seed S[i]
    A.reset(_dev(E >= k, A, np.uint8))
  B = _batched(n, seeds=other, auto_reset=False)
  assert B.pool_status()['state'] == 'off'
  B.reset()
  _run(B, _tape(n, 4, n))
  mask = (rs.rand(n) < 0.6).astype(np.uint8)
  mask[:2] = 1, 0
  rows = _dev(np.nonzero(mask)[0], B, np.int64)
  rest = _dev(np.nonzero(mask == 0)[0], B, np.int64)
  rec_before, obs_before = B.state['rec'].clone(), B.obs.clone()
  B.reset(_dev(mask, B, np.uint8), seeds=S, episodes=E.tolist())
  assert torch.equal(B.obs[rows], A.obs[rows])
  assert torch.equal(B.state['rec'][rest], rec_before[rest]) and torch.equal(B.obs[rest], obs_before[rest])
  assert B.records()['episode'][mask != 0].tolist() == E[mask != 0].tolist()
  _follow([(B, A, rows)], _tape(n + 1, 14, n))   # (4 + 14 steps: no row runs into `length`, where a batch without auto-reset stops)
  _assert_rows_equal(B, A, np.nonzero(mask)[0])
  # episodes alone: the rows restart at an episode of the seeds they have
  B.reset(_dev(mask, B, np.uint8), episodes=2)
  A.reset(_dev(mask, A, np.uint8), seeds=S, episodes=torch.full((n,), 2, dtype=torch.int32, device=A.device))
  assert torch.equal(B.obs[rows], A.obs[rows]) and torch.equal(B.state['rec'][rows], A.state['rec'][rows])
  with pytest.raises(ValueError):
    B.reset(seeds=S[:-1])
  with pytest.raises(ValueError):
    B.reseed(S, episodes=0)
  for e in (A, B):
    e.check_errors()


def test_env_facade_reset_with_seed():
  from crafter_amd import Env
  acts = np.random.RandomState(5).randint(0, 17, size=30)
  e = Env(seed=1, length=LENGTH)
  e.reset()
  for a in acts[:5]:
    e.step(a)
  fresh = Env(seed=7, length=LENGTH)
  assert np.array_equal(e.reset(seed=7), fresh.reset())
  assert (e._seed, e._episode, e._step) == (7, 1, 0)

  def same_step(envs, a):
    outs = [x.step(a) for x in envs]
    for o in outs[1:]:
      assert np.array_equal(o[0], outs[0][0]) and o[1] == outs[0][1] and o[2] == outs[0][2]
      assert o[3]['inventory'] == outs[0][3]['inventory'] and np.array_equal(o[3]['semantic'], outs[0][3]['semantic'])
    return outs[0][2]
  for a in acts[5:12]:
    same_step((e, fresh), a)
  twin = copy.deepcopy(e)
  assert twin._seed == 7 and twin._ctor_args()['seed'] == 7 and twin._episode == 1
  done = False
  for a in acts[12:]:
    done = same_step((e, fresh, twin), a) or done
    if done:
      break
  first = [x.reset() for x in (e, fresh, twin)]   # episode 2 of seed 7 in all three
  assert np.array_equal(first[0], first[1]) and np.array_equal(first[0], first[2]) and e._episode == 2
  # a given episode; and an episode of the seed the env has
  third = Env(seed=7, length=LENGTH)
  for _ in range(3):
    want = third.reset()
  assert np.array_equal(e.reset(seed=7, episode=3), want) and np.array_equal(twin.reset(episode=3), want)
  assert e._episode == twin._episode == 3 and twin._seed == 7


def test_vec_env_view_reseed():
  from crafter_amd.vec import VecEnvView
  v, ctl = (VecEnvView(4, seeds=[1, 2, 3, 4], length=5) for _ in range(2))
  v.reset(), ctl.reset()
  v.reseed(['x', 8], episodes=[1, 2], indices=[1, 3])
  assert v.batch.seeds == [1, 'x', 3, 8]
  for t in range(5):
    got, want = v.step([0, 0, 0, 0]), ctl.step([0, 0, 0, 0])
    assert np.array_equal(got[2], want[2])
    if t < 4:
      assert np.array_equal(got[0], want[0])
  assert got[2].all()   # every env ran into length: step_wait reset them
  ref = _batched(4, seeds=[1, 'x', 3, 8], length=5, auto_reset=False)
  ref.reset(seeds=[1, 'x', 3, 8], episodes=[2, 1, 2, 2])
  assert np.array_equal(got[0], ref.obs.cpu().numpy())
  assert np.array_equal(got[0][[0, 2]], want[0][[0, 2]]) and not np.array_equal(got[0][1], want[0][1])
  assert v.seed() == [None] * 4
  v.batch.check_errors()


# ------------------------------------------------------------------ 7. levels() and the level cache
def test_levels_round_trip_and_level_cache():
  n = 256
  S, other = _seeds(n)
  A = _batched(n, seeds=S)
  A.reset()
  pre = _tape(n, 50, n)
  _run(A, pre[:10])
  A.reset(_dev(np.arange(n) % 3 == 0, A, np.uint8))   # so that the episode numbers differ between rows
  _run(A, pre[10:])
  lanes, episodes = A.levels()
  assert lanes.dtype == torch.int64 and episodes.dtype == torch.int32 and lanes.is_cuda and episodes.is_cuda
  from crafter_amd import state
  assert np.array_equal(lanes.cpu().numpy().view(np.uint64), state.seed_lanes(S))
  assert np.array_equal(episodes.cpu().numpy(), A.records()['episode']) and len(np.unique(episodes.cpu().numpy())) >= 2
  B = _batched(n, seeds=other)
  B.reset()
  B.reset(seeds=lanes, episodes=episodes)
  A.reset(seeds=lanes, episodes=episodes)
  assert B.seeds == [None] * n
  assert torch.equal(A.obs, B.obs)
  assert torch.equal(A.levels()[1], episodes) and torch.equal(B.levels()[0], lanes)
  # the level cache: the start states of rows 0 .. 31, saved once, replayed into other rows at copy cost
  src, dst = np.arange(32), np.arange(100, 132)
  cache = B.save_state(src)
  tape = _tape(n + 1, 30, n)
  seen = []
  _follow([(B, A, None)], tape, on_step=lambda t: seen.append((B.obs[:32].clone(), B.reward[:32].clone(), B.done[:32].clone())))
  _assert_rows_equal(B, A, np.arange(n))
  B.load_state(cache, idx=dst)
  assert torch.equal(B.obs[100:132], A.reset(seeds=lanes, episodes=episodes)[:32])
  again = tape.copy()
  again[:, dst] = tape[:, src]
  for t, a in enumerate(again):
    B.step(_dev(a, B), info=False)
    o, r, d = seen[t]
    assert torch.equal(B.obs[100:132], o) and torch.equal(B.reward[100:132], r) and torch.equal(B.done[100:132], d), t
  assert any(bool(d.any()) for _, _, d in seen)   # across an episode end
  for e in (A, B):
    e.check_errors()
