"""Level sets on the device (BatchedEnv.set_levels / level_ids / levels, crafter_set_levels / crafter_level_ids): a batch B under
a level table is, step for step, a table-free batch R that the existing reseed() puts on the levels the host mirror
(crafter_amd.levels_pick) names -- through step(), rollout(), step_envs() and step(final=True), with the world pool on and
off.  Episodes of 20 steps and tapes of 100: every row passes at least three episode ends, and the pool serves B to the end."""
import ctypes as C

import numpy as np
import pytest
import torch

import crafter_amd
from crafter_amd import state

pytestmark = pytest.mark.gpu

LENGTH, STEPS = 20, 100
KMAX = STEPS + 8                         # no row can enter more episodes than that
TAB = (['lv-a', 2, 977], [3, 1, 2])      # (seeds, episodes) of the table most tests use
KEY = 0x5EED0123456789AB


def _batched(n, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(n, **{**dict(length=LENGTH, seeds=[7 * i + 100001 for i in range(n)]), **k})


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def _tape(seed, n, steps=STEPS):
  return np.random.RandomState(seed).randint(0, 17, (steps, n)).astype(np.int32)


def _mirror(env, seeds, episodes, weights=None, key=0):
  """int [N, KMAX]: the table entry row i plays in its k-th episode, by the host mirror alone.  env: a batch, or its seeds."""
  lanes = state.seed_lanes(getattr(env, 'seeds', env))
  cum = None if weights is None else state.levels_cum(weights)
  return crafter_amd.levels_pick(lanes[:, None], np.arange(KMAX)[None, :], len(seeds), cum, key).astype(np.int64)


class Follower:
  """A table-free batch R with B's seeds, kept on the levels a PLAN names with the existing reseed(): plan = (lanes int64
  [N, KMAX], episodes int32 [N, KMAX]), what row i plays in B's k-th episode.  R is always reseeded one episode ahead -- its
  own automatic or manual reset then starts the planned level -- and k counts B's resets.  Nothing here reads the device back."""

  def __init__(self, B, **kw):
    self.R = _batched(B.num_envs, **kw)
    self.n = B.num_envs
    self.seeds = list(self.R.seeds)   # (R.seeds reads None once lanes came from the device)
    self.k = torch.zeros(self.n, dtype=torch.int64, device=self.R.device)   # the episode B's rows are in
    self.rows = torch.arange(self.n, device=self.R.device)
    self.plan = None

  def table_plan(self, seeds, episodes, weights=None, key=0):
    m = _mirror(self.seeds, seeds, episodes, weights, key)
    lanes = state.seed_lanes(seeds).view(np.int64)[m]
    eps = np.asarray(episodes, np.int32)[m]
    return _dev(lanes, self.R, np.int64), _dev(eps, self.R, np.int32)

  def own_plan(self):
    lanes = np.repeat(state.seed_lanes(self.seeds).view(np.int64)[:, None], KMAX, axis=1)
    eps = np.repeat(np.arange(KMAX, dtype=np.int32)[None, :], self.n, axis=0)
    return _dev(lanes, self.R, np.int64), _dev(eps, self.R, np.int32)

  def follow(self, plan, mask=None):
    """From each (named) row's next reset on, R plays `plan`."""
    self.plan = plan
    self._ahead(mask)

  def _ahead(self, mask):
    nxt = (self.k + 1).clamp(max=KMAX - 1)
    self.R.reseed(self.plan[0][self.rows, nxt].contiguous(), self.plan[1][self.rows, nxt].contiguous(), mask)

  def reset(self, mask=None):
    m = None if mask is None else _dev(mask, self.R, np.uint8)
    obs = self.R.reset(m)
    self.k += 1 if m is None else (m != 0).to(torch.int64)
    self._ahead(m)
    return obs

  def step(self, a):
    obs, reward, done, _ = self.R.step(_dev(a, self.R), info=False)
    self.k += (done != 0).to(torch.int64)
    self._ahead(done)
    return obs, reward, done


MODES = ['step', 'rollout', 'step_envs', 'final']


def _play(B, mode, tape):
  """B through `tape` by `mode` -> (obs [T, N, ...], reward [T, N], done [T, N])."""
  if mode == 'rollout':
    return B.rollout(_dev(tape, B))
  o, r, d = [], [], []
  n = B.num_envs
  halves = [np.arange(0, n, 2), np.arange(1, n, 2)]
  for a in tape:
    if mode == 'step_envs':
      for idx in halves:
        obs, reward, done, _ = B.step_envs(_dev(idx, B), _dev(a[idx], B), info=False)
    else:
      obs, reward, done, _ = B.step(_dev(a, B), info=False, final=(mode == 'final'))
    o.append(obs.clone()), r.append(reward.clone()), d.append(done.clone())
  return torch.stack(o), torch.stack(r), torch.stack(d)


def _assert_states_equal(B, R, where=''):
  """mat, mt and the slot table up to nobj; B's lane and episode count are its own."""
  for name in ('mat', 'mt'):
    assert torch.equal(B.state[name], R.state[name]), f'{where}: {name}'
  nobj = B._rec_i32[:, B._off['nobj']]
  assert torch.equal(nobj, R._rec_i32[:, R._off['nobj']]), f'{where}: nobj'
  live = (torch.arange(B.cfg.max_objects, device=B.device)[None, :] < nobj[:, None])[:, :, None]
  assert torch.equal(B.state['objs'] * live, R.state['objs'] * live), f'{where}: objs'


def _pool_served(B, before, where=''):
  ps = B.pool_status()
  assert ps['state'] == 'running', where
  assert ps['adopted'] > before, f'{where}: no env adopted a pooled world in the last 40 steps'


def _equivalence(n, mode, pool, weights=None):
  gen_period = 0 if pool else -1
  B = _batched(n, gen_period=gen_period)
  B.set_levels(*TAB, weights=weights, key=KEY)
  F = Follower(B, gen_period=gen_period)
  F.follow(F.table_plan(*TAB, weights=weights, key=KEY))
  assert torch.equal(B.reset(), F.reset()), 'first frames'
  tape = _tape(n + (7 if pool else 8), n)
  cut, late = 7, STEPS - 40
  mask = (np.arange(n) % 2 == 0).astype(np.uint8)   # a manual reset of half the rows in mid-episode: the ends fall apart
  ends = torch.zeros(n, dtype=torch.int64, device=B.device)
  adopted = 0
  for lo, hi in ((0, cut), (cut, late), (late, STEPS)):
    if lo == cut:
      named = _dev(np.nonzero(mask)[0], B, np.int64)   # (the other rows of B.obs: rollout() does not keep them current)
      assert torch.equal(B.reset(_dev(mask, B, np.uint8))[named], F.reset(mask)[named]), 'manual reset under a mask'
    if lo == late and pool:
      adopted = B.pool_status()['adopted']
    bo, br, bd = _play(B, mode, tape[lo:hi])
    for t in range(lo, hi):
      ro, rr, rd = F.step(tape[t])
      assert torch.equal(bd[t - lo], rd) and torch.equal(br[t - lo], rr), f'step {t}: reward / done'
      assert torch.equal(bo[t - lo], ro), f'step {t}: obs'
    ends += bd.to(torch.int64).sum(dim=0)
  assert int(ends.min()) >= 3, f'a row passed only {int(ends.min())} episode ends'
  _assert_states_equal(B, F.R, 'at the end')
  rec = B.records()
  assert np.array_equal(rec['seed_lane'], state.seed_lanes(B.seeds))
  want_k = 1 + mask + ends.cpu().numpy()
  assert np.array_equal(rec['episode'], want_k) and np.array_equal(F.k.cpu().numpy(), want_k)
  ids = B.level_ids().cpu().numpy()
  assert np.array_equal(ids, _mirror(B, *TAB, weights=weights, key=KEY)[np.arange(n), want_k])
  if pool:
    _pool_served(B, adopted, mode)
  else:
    assert B.pool_status()['state'] == 'off'
  B.check_errors()
  F.R.check_errors()
  return B, F


# ------------------------------------------------------------------ 1. whole trajectories against the existing feature
@pytest.mark.parametrize('pool', [True, False], ids=['pool', 'inline'])
@pytest.mark.parametrize('mode', MODES)
def test_batch_under_a_table_equals_a_reseeded_batch(mode, pool):
  _equivalence(8, mode, pool)


def test_batch_under_a_table_equals_a_reseeded_batch_64():
  B, _ = _equivalence(64, 'step', True)
  m = _mirror(B, *TAB, key=KEY)[:, 1:5]
  assert set(m.reshape(-1).tolist()) == {0, 1, 2} and len({tuple(r) for r in m.tolist()}) > 8   # the rows draw apart


# ------------------------------------------------------------------ 2. level_ids() and levels()
def test_level_ids_and_levels():
  n = 8
  B = _batched(n)
  B.set_levels(*TAB, key=KEY)
  m = _mirror(B, *TAB, key=KEY)
  B.reset()
  plain = _batched(n, seeds=list(range(n)), auto_reset=False)   # a table-free batch of other seeds
  plain.reset()
  k = np.ones(n, np.int64)
  assert np.array_equal(B.level_ids().cpu().numpy(), m[np.arange(n), k])
  tab_lanes, tab_eps = state.seed_lanes(TAB[0]).view(np.int64), np.asarray(TAB[1], np.int32)
  checked = 0
  out = torch.full((n,), -9, dtype=torch.int32, device=B.device)
  for t, a in enumerate(_tape(21, n)):
    if t == 7:
      half = (np.arange(n) % 2 == 0)
      B.reset(_dev(half, B, np.uint8))
      k += half
    _, _, done, _ = B.step(_dev(a, B), info=False)
    d = done.cpu().numpy() != 0
    k += d
    if not d.any():
      continue
    rows = np.nonzero(d)[0]
    ids = B.level_ids().cpu().numpy()
    assert np.array_equal(ids[rows], m[rows, k[rows]]), t
    # under a mask and into `out`: the other rows keep what they held
    assert B.level_ids(done, out=out) is out
    got = out.cpu().numpy()
    assert np.array_equal(got[rows], ids[rows]) and (got[~d] == -9).all()
    out.fill_(-9)
    lanes, eps = B.levels()
    assert lanes.dtype == torch.int64 and eps.dtype == torch.int32
    assert np.array_equal(lanes.cpu().numpy()[rows], tab_lanes[ids[rows]]) and np.array_equal(eps.cpu().numpy()[rows], tab_eps[ids[rows]])
    first = plain.reset(seeds=lanes, episodes=eps)
    r = _dev(rows, B, np.int64)
    assert torch.equal(first[r], B.obs[r]), f'step {t}: levels() does not replay the first frames'
    checked += len(rows)
  assert checked >= 3 * n and k.min() >= 4
  assert np.array_equal(B.records()['episode'], k)
  B.check_errors()
  plain.check_errors()


# ------------------------------------------------------------------ 3. one level
def test_one_level_every_episode_starts_alike():
  n = 8
  B = _batched(n)
  B.set_levels([31], episodes=2)
  want = _batched(1, seeds=[31], auto_reset=False)
  want.reset(seeds=[31], episodes=2)
  first, mat = want.obs[0], want.state['mat'][0]
  obs = B.reset()
  assert all(torch.equal(obs[i], first) for i in range(n)) and all(torch.equal(B.state['mat'][i], mat) for i in range(n))
  ends = np.zeros(n, np.int64)
  adopted = 0
  for t, a in enumerate(_tape(31, n)):
    if t == STEPS - 40:
      adopted = B.pool_status()['adopted']
    obs, _, done, _ = B.step(_dev(a, B), info=False)
    for i in np.nonzero(done.cpu().numpy())[0]:
      ends[i] += 1
      assert torch.equal(obs[i], first) and torch.equal(B.state['mat'][i], mat), (t, i)
  assert ends.min() >= 3 and (B.level_ids() == 0).all()
  _pool_served(B, adopted)
  B.check_errors()


# ------------------------------------------------------------------ 4. weights
def test_zero_weights_are_never_played_and_skewed_weights_follow_the_mirror():
  n = 8
  seeds, eps = [5, 6, 7], [1, 2, 1]
  B = _batched(n)
  B.set_levels(seeds, eps, weights=[0, 1, 0], key=3)
  want = _batched(1, seeds=[6], auto_reset=False)
  want.reset(seeds=[6], episodes=2)
  first = want.obs[0]
  obs = B.reset()
  assert all(torch.equal(obs[i], first) for i in range(n))
  ends = np.zeros(n, np.int64)
  tape = _tape(41, n)
  for t, a in enumerate(tape[:65]):
    obs, _, done, _ = B.step(_dev(a, B), info=False)
    assert (B.level_ids() == 1).all()
    for i in np.nonzero(done.cpu().numpy())[0]:
      ends[i] += 1
      assert torch.equal(obs[i], first), (t, i)
  assert ends.min() >= 3
  B.check_errors()
  # a skewed vector: the whole trajectory against a batch reseeded by the mirror, ids included
  B, F = _equivalence(n, 'step', True, weights=[5, 0, 2])
  m = _mirror(B, *TAB, weights=[5, 0, 2], key=KEY)
  assert set(m.reshape(-1).tolist()) == {0, 2} and (m == 0).mean() > 0.6


# ------------------------------------------------------------------ 5. replacing the table mid-run
def test_replacing_and_clearing_the_table_mid_run():
  n = 8
  second = ([40, 41, 42, 43, 44], [1, 1, 2, 1, 3])
  B = _batched(n)
  B.set_levels(*TAB, key=KEY)
  F = Follower(B)
  F.follow(F.table_plan(*TAB, key=KEY))
  assert torch.equal(B.reset(), F.reset())
  tape = _tape(51, n, 130)
  ends = {}
  adopted = 0

  def run(lo, hi, what):
    e = torch.zeros(n, dtype=torch.int64, device=B.device)
    for t in range(lo, hi):
      obs, reward, done, _ = B.step(_dev(tape[t], B), info=False)
      ro, rr, rd = F.step(tape[t])
      assert torch.equal(done, rd) and torch.equal(reward, rr) and torch.equal(obs, ro), f'{what}, step {t}'
      e += done.to(torch.int64)
    ends[what] = int(e.min())
  run(0, 7, 'first table')
  half = (np.arange(n) % 2 == 0).astype(np.uint8)
  assert torch.equal(B.reset(_dev(half, B, np.uint8)), F.reset(half))
  run(7, 30, 'first table, rows apart')
  # in mid-episode: the episodes in progress play on, each row's next reset draws from the second table
  rec = B.state['rec'].clone()
  B.set_levels(*second, weights=[1, 1, 1, 1, 4], key=9)
  F.follow(F.table_plan(*second, weights=[1, 1, 1, 1, 4], key=9))
  assert torch.equal(B.state['rec'], rec)
  run(30, 75, 'second table')
  # ... and without a table: the worlds of a fresh batch of B's own seeds at the same k
  B.set_levels(None)
  assert (B.level_ids() == -1).all()
  F.follow(F.own_plan())
  adopted = B.pool_status()['adopted']
  run(75, 130, 'no table')
  assert ends['second table'] >= 2 and ends['no table'] >= 2 and ends['first table, rows apart'] >= 1
  _assert_states_equal(B, F.R, 'at the end')
  assert torch.equal(B.levels()[0], F.R.levels()[0]) and torch.equal(B.levels()[1], F.R.levels()[1])   # R is on (own lane, k) itself now
  _pool_served(B, adopted)
  B.check_errors()
  F.R.check_errors()


# ------------------------------------------------------------------ 6. copies
def test_a_copy_plays_the_levels_its_source_would():
  n = 8
  B = _batched(n)
  B.set_levels(*TAB, key=KEY)
  B.reset()
  tape = _tape(61, n)
  for a in tape[:12]:
    B.step(_dev(a, B), info=False)
  src, dst = [0, 3], [5, 6]
  B.copy_envs(src, dst)
  assert np.array_equal(B.records()['seed_lane'][dst], B.records()['seed_lane'][src])
  ends = np.zeros(2, np.int64)
  adopted = 0
  for t, a in enumerate(tape[12:]):
    if t == STEPS - 12 - 40:
      adopted = B.pool_status()['adopted']
    a = a.copy()
    a[dst] = a[src]
    obs, reward, done, _ = B.step(_dev(a, B), info=False)
    assert torch.equal(obs[dst], obs[src]) and torch.equal(reward[dst], reward[src]) and torch.equal(done[dst], done[src]), t
    ends += done[src].cpu().numpy() != 0
  assert ends.min() >= 3
  ids = B.level_ids().cpu().numpy()
  assert np.array_equal(ids[dst], ids[src])
  _pool_served(B, adopted)
  # a store taken under this table, loaded under another: the rows follow the table in force
  store = B.save_state(src)
  other = ([70, 71], [1, 2])
  B.set_levels(*other, key=1)
  B.load_state(store, idx=dst)
  k = B.records()['episode']
  assert np.array_equal(k[dst], k[src])
  for a in tape[:LENGTH]:
    a = a.copy()
    a[dst] = a[src]
    obs, _, done, _ = B.step(_dev(a, B), info=False)
    assert torch.equal(obs[dst], obs[src]) and torch.equal(done[dst], done[src])
  assert (B.records()['episode'][src] > k[src]).all()
  m = crafter_amd.levels_pick(B.records()['seed_lane'], B.records()['episode'], 2, None, 1)
  assert np.array_equal(B.level_ids().cpu().numpy(), m)
  B.check_errors()


# ------------------------------------------------------------------ 7. no table, errors, facades
def test_without_a_table_ids_read_minus_one():
  B = _batched(8)
  B.reset()
  assert (B.level_ids() == -1).all()
  B.set_levels(None)   # clearing what was never set: nothing happens
  for a in _tape(71, 8, 3):
    B.step(_dev(a, B), info=False)
  assert (B.level_ids() == -1).all()
  lanes, eps = B.levels()
  assert np.array_equal(lanes.cpu().numpy().view(np.uint64), state.seed_lanes(B.seeds)) and (eps == 1).all()
  B.check_errors()


def test_c_errors_and_python_argument_checks():
  B = _batched(8)
  B.reset()
  lanes = torch.zeros(4, dtype=torch.int64, device=B.device)
  eps = torch.ones(4, dtype=torch.int32, device=B.device)
  p = lambda t: C.c_void_p(t.data_ptr())
  from crafter_amd import lib as hiplib
  for args, text in (((p(lanes), p(eps), None, -1, 0), 'n_levels'), ((p(lanes), p(eps), None, 65537, 0), 'n_levels'),
                     ((None, p(eps), None, 4, 0), 'null'), ((p(lanes), None, None, 4, 0), 'null')):
    assert B._lib.crafter_set_levels(B._handle, *args, B._stream()) != 0
    assert text in hiplib.last_error(B._lib, B._handle)
  assert B._lib.crafter_level_ids(B._handle, None, None, B._stream()) != 0
  assert (B.level_ids() == -1).all()   # none of them set a table
  for bad in (dict(seeds=[]), dict(seeds=[1, 2], episodes=[1]), dict(seeds=[1, 2], episodes=0), dict(seeds=[1, 2], weights=[0, 0]),
              dict(seeds=[1, 2], weights=[1, -1]), dict(seeds=list(range(65537))), dict(seeds=None, weights=[1]),
              dict(seeds=torch.zeros(3, dtype=torch.int32, device=B.device)),
              dict(seeds=lanes, episodes=torch.ones(3, dtype=torch.int32, device=B.device))):
    with pytest.raises(ValueError):
      B.set_levels(**bad)
  with pytest.raises(ValueError):
    B.level_ids(out=torch.zeros(8, dtype=torch.int64, device=B.device))
  assert (B.level_ids() == -1).all()
  # lanes and episodes on the device: levels() of a table-free batch is a table
  src = _batched(3, seeds=['x', 5, 6])
  src.reset()
  B.check_errors()
  dev, ref = _batched(8), _batched(8)
  dev.set_levels(*src.levels())
  ref.set_levels(['x', 5, 6])
  assert torch.equal(dev.reset(), ref.reset())
  assert torch.equal(dev.level_ids(), ref.level_ids()) and len(set(dev.level_ids().tolist())) > 1
  dev.check_errors()


def test_facades_set_levels():
  from crafter_amd import Env
  from crafter_amd.vec import VecEnvView
  want = _batched(1, seeds=[77], auto_reset=False)
  first = want.reset(seeds=[77], episodes=2)[0].cpu().numpy()
  e = Env(seed=1, length=LENGTH)
  e.set_levels([77], episodes=2)
  assert np.array_equal(e.reset(), first) and np.array_equal(e.reset(), first) and e._episode == 2 and e._seed == 1
  e.set_levels(None)
  assert not np.array_equal(e.reset(), first)
  v = VecEnvView(4, seeds=[1, 2, 3, 4], length=5)
  v.env_method('set_levels', [77], episodes=2)
  assert all(np.array_equal(o, first) for o in v.reset())
  for _ in range(5):
    obs, _, done, _ = v.step([0, 0, 0, 0])
  assert done.all() and all(np.array_equal(o, first) for o in obs)
  v.set_levels(None)
  v.batch.check_errors()
