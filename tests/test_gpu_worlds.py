"""BatchedEnv.reset(worlds=...) / crafter_reset_worlds on the device: authored worlds against the oracle whose world function is
the authored one (tests/worlds_ref.py; tied to the real reference by tests/test_worlds_golden.py) through a night, on the
LDS-resident and the global-memory layouts, under auto-reset with the world pool running, masked into the middle of a run next
to a twin batch that never made the call, with world ids on the device and absent, and the device-side validation."""
import numpy as np
import pytest
import torch

from tests import worlds_cases as wc
from tests.parity import assert_same
from tests.worlds_ref import AuthoredOracle, clean_world

pytestmark = pytest.mark.gpu

STATE = ('mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census')


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env):
  return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(env.device)


def _rows(env, names=STATE):
  return {k: env.state[k].cpu().numpy() for k in names}


def test_parity_four_envs_through_a_night():
  """The CPU parity case at N = 4 (world ids absent: env % 3, so env 3 plays the meadow under another seed): state, frame,
  reward and done at every one of 180 steps."""
  seeds = [31, 32, 33, 34]
  runs = [wc.oracle_run(i, s) for i, s in enumerate(seeds)]
  assert max(r.balance[-1] for r in runs) >= 1
  env = _batched(4, seeds=seeds, auto_reset=False)
  obs = env.reset(worlds=wc.bank_of(env, range(3))).cpu().numpy()
  for i, r in enumerate(runs):
    assert np.array_equal(obs[i], r.frames[0]), f'env {i}: first frame'
    assert_same(env.snapshot(i), r.snapshots[0], f'env {i} reset')
  tapes = np.stack([wc.tape(i) for i in range(4)], 1)
  for t in range(wc.T):
    obs, rew, done, _ = env.step(_dev(tapes[t], env))
    obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    for i, r in enumerate(runs):
      assert np.array_equal(obs[i], r.frames[t + 1]), f'env {i} step {t + 1}: pixels'
      assert rew[i] == np.float32(r.rewards[t]) and bool(done[i]) == r.dones[t], f'env {i} step {t + 1}: reward / done'
      assert_same(env.snapshot(i), r.snapshots[t + 1], f'env {i} step {t + 1}')
  env.check_errors()


@pytest.mark.parametrize('area,view,size', [((42, 30), (7, 9), (84, 72)), ((256, 256), (9, 9), (64, 64))], ids=['42x30-lds', '256x256-global'])
def test_other_geometries(area, view, size):
  from crafter_amd import WorldBank
  env = _batched(2, area=area, view=view, size=size, seeds=[81, 82], auto_reset=False)
  assert env.slot_map_derived == (area[0] < 256)
  env.reset()
  world = wc.small_world(area)
  bank = WorldBank(env, world['mat'][None], [world['objects']], [world['inventory']])
  obs = env.reset(worlds=bank, world_ids=[0, 0]).cpu().numpy()
  orcs = []
  for i in range(2):
    o = AuthoredOracle(seed=81 + i, area=area, view=view, size=size)
    o.reset()
    o.world = world
    assert np.array_equal(obs[i], o.reset())
    assert_same(env.snapshot(i), o.snapshot(), f'env {i} reset')
    orcs.append(o)
  tape = np.random.RandomState(9).randint(0, 17, size=30)
  for t in range(30):
    obs = env.step(_dev(np.full(2, tape[t]), env))[0].cpu().numpy()
    for i, o in enumerate(orcs):
      assert np.array_equal(obs[i], o.step(int(tape[t]))[0]), (t, i)
  for i, o in enumerate(orcs):
    assert_same(env.snapshot(i), o.snapshot(), f'env {i} step 30')
  env.check_errors()


def test_auto_reset_follows_an_authored_episode_with_the_generated_one():
  """auto_reset, pool on, length 12: the authored episode (number 2) ends by length, and what follows is episode 3 of each
  env's seed -- state and first frame of a plain batch restarted at that episode -- and then episode 4, the pool still running."""
  seeds, length = [21, 22, 23, 24], 12
  a, b = _batched(4, seeds=seeds, length=length), _batched(4, seeds=seeds, length=length)
  a.reset()
  a.reset(worlds=wc.bank_of(a, range(3)))
  runs = [wc.oracle_run(i, s, steps=length, first_episode=2, length=length) for i, s in enumerate(seeds)]
  for i, r in enumerate(runs):
    assert_same(a.snapshot(i), r.snapshots[0], f'env {i}: the authored reset')
  assert all(r.dones == [False] * (length - 1) + [True] for r in runs), 'the authored episodes must end by length, all at once'
  tapes = np.stack([wc.tape(i, length) for i in range(4)], 1)
  for t in range(length):
    obs, _, done, _ = a.step(_dev(tapes[t], a))
    assert bool(done.all()) == (t == length - 1)
    if t < length - 1:
      assert all(np.array_equal(obs[i].cpu().numpy(), r.frames[t + 1]) for i, r in enumerate(runs))
  first = b.reset(episodes=3).cpu().numpy()
  assert np.array_equal(a.obs.cpu().numpy(), first)
  for i in range(4):
    assert_same(a.snapshot(i), b.snapshot(i), f'env {i}: the episode after the authored one')
    assert a.snapshot(i)['episode'] == 3
  acts = np.random.RandomState(4).randint(0, 17, size=(length + 3, 4))
  for t in range(length + 3):
    oa, ob = a.step(_dev(acts[t], a))[0], b.step(_dev(acts[t], b))[0]
    assert torch.equal(oa, ob), t
  for i in range(4):
    assert_same(a.snapshot(i), b.snapshot(i), f'env {i}: episode 4')
    assert a.snapshot(i)['episode'] == 4
  assert a.pool_status()['state'] == 'running'
  a.check_errors()


def test_masked_reset_in_the_middle_of_a_run_leaves_the_other_rows_alone():
  """8 envs stepped by step / step_envs / rollout / copy_envs, a twin doing the same; one of them resets rows 1, 4, 6 into
  authored worlds (ids on the device, garbage in the unnamed rows) and both go on: the named rows are the oracle's, every other
  row is bit-identical to the twin's in every state buffer and in obs / reward / done."""
  seeds = [100 + i for i in range(8)]
  named, ids = [1, 4, 6], np.array([77, 2, -5, 1 << 30, 0, 9, 1, 3], np.int32)
  rs = np.random.RandomState(12)
  script = [('step', rs.randint(0, 17, 8)) for _ in range(4)] + [('envs', [7, 1, 4], rs.randint(0, 17, 3)), ('rollout', rs.randint(0, 17, (6, 8))),
            ('copy', [0], [5]), ('worlds',), ('step', rs.randint(0, 17, 8)), ('envs', [6, 2, 1], rs.randint(0, 17, 3)),
            ('rollout', rs.randint(0, 17, (5, 8))), ('step', rs.randint(0, 17, 8)), ('copy', [3], [7])]
  a, b = _batched(8, seeds=seeds), _batched(8, seeds=seeds)
  bank = wc.bank_of(a, range(3))
  worlds = {1: 2, 4: 0, 6: 1}
  orcs = {}
  for env in (a, b):
    env.reset()
    for op in script:
      if op[0] == 'step':
        env.step(_dev(op[1], env))
      elif op[0] == 'envs':
        env.step_envs(op[1], _dev(op[2], env))
      elif op[0] == 'rollout':
        env.rollout(_dev(op[1], env))
      elif op[0] == 'copy':
        env.copy_envs(op[1], op[2])
      elif env is a:
        mask = torch.zeros(8, dtype=torch.uint8, device=a.device)
        mask[named] = 1
        obs = a.reset(mask=mask, worlds=bank, world_ids=_dev(ids, a)).cpu().numpy()
        for i in named:
          o = AuthoredOracle(seed=seeds[i])
          o.reset()
          o.world = wc.WORLDS[worlds[i]]()
          assert np.array_equal(obs[i], o.reset()), f'env {i}: first frame'
          assert_same(a.snapshot(i), o.snapshot(), f'env {i}: the authored reset')
          orcs[i] = o
  for op in script[[op[0] for op in script].index('worlds') + 1:]:   # the oracle's side of what followed the call
    for i, o in orcs.items():
      if op[0] == 'step':
        o.step(int(op[1][i]))
      elif op[0] == 'envs' and i in op[1]:
        o.step(int(op[2][op[1].index(i)]))
      elif op[0] == 'rollout':
        for t in range(len(op[1])):
          o.step(int(op[1][t][i]))
  for i, o in orcs.items():
    assert_same(a.snapshot(i), o.snapshot(), f'env {i}: after the run')
  ra, rb = _rows(a), _rows(b)
  others = [i for i in range(8) if i not in named]
  for k in STATE:
    assert np.array_equal(ra[k][others], rb[k][others]), k
    assert not np.array_equal(ra[k][named], rb[k][named]), k
  for k in ('obs', 'reward', 'done'):
    assert torch.equal(getattr(a, k)[others], getattr(b, k)[others]), k
  a.check_errors()
  b.check_errors()


def test_validation_through_check_errors():
  """Every flagged case in one batch (one env each, the last env a clean world): ST_BAD_WORLD in exactly the flagged rows,
  check_errors raises naming it, each row is the oracle's on the cleaned input; a world id outside the bank leaves its row as
  it was; host-side values raise ValueError before anything runs."""
  from crafter_amd import CrafterDeviceError, WorldBank, abi
  names = sorted(wc.bad_cases())
  worlds = [wc.edited_garden(wc.bad_cases()[n]) for n in names] + [wc.edited_garden(lambda w: None)]
  n = len(worlds)
  env = _batched(n, seed=300, auto_reset=False)
  bank = WorldBank(env, np.stack([w['mat'] for w in worlds]), [w['objects'] for w in worlds], [w['inventory'] for w in worlds], validate=False)
  obs = env.reset(worlds=bank, world_ids=_dev(np.arange(n), env)).cpu().numpy()
  assert list(env.records()['status']) == [abi.STATUS_BAD_WORLD] * (n - 1) + [0]
  with pytest.raises(CrafterDeviceError, match='ST_BAD_WORLD'):
    env.check_errors()
  for i, w in enumerate(worlds):
    mat, objs, flagged = clean_world(w, (64, 64), len(wc.MAT), wc.MAT['grass'])
    assert flagged == (i < n - 1)
    o = AuthoredOracle(seed=300 + i, world=dict(mat=mat, objects=objs, inventory=w['inventory']))
    assert np.array_equal(obs[i], o.reset()), names[i] if i < n - 1 else 'clean'
    assert_same(env.snapshot(i), o.snapshot(), names[i] if i < n - 1 else 'clean')
  # a world id outside the bank, given on the device: the row stays, the bit is set; on the host it is a ValueError
  env2 = _batched(3, seed=400, auto_reset=False)
  env2.reset()
  before = _rows(env2)
  good = wc.bank_of(env2, [1])
  env2.reset(worlds=good, world_ids=_dev([0, 1, -1], env2))
  after = _rows(env2)
  rec = env2.records()
  assert list(rec['status']) == [0, abi.STATUS_BAD_WORLD, abi.STATUS_BAD_WORLD] and list(rec['episode']) == [2, 1, 1]
  for k in STATE:
    if k != 'rec':
      assert np.array_equal(after[k][1:], before[k][1:]), k
  with pytest.raises(ValueError):
    env2.reset(worlds=good, world_ids=[0, 1, 0])
  with pytest.raises(ValueError):
    env2.reset(worlds=wc.bank_of(dict(area=(32, 32)), [1], area=(32, 32)))
  with pytest.raises(ValueError):
    env2.reset(world_ids=[0, 0, 0])


def test_slot_table_grows_for_a_long_world_and_export_round_trips():
  """A world of 250 objects does not fit three quarters of the default 256 slots: the table grows first.  export_worlds ->
  WorldBank -> reset into another row reproduces map, objects in compacted slot order and inventory."""
  from crafter_amd import WorldBank
  env = _batched(3, seed=500, auto_reset=False, grow_objects=True)
  mat = np.full((1, 64, 64), wc.MAT['grass'], np.uint8)
  objs = [(wc.PLANT, 2 + (k % 30) * 2, 2 + (k // 30) * 2, 1, (0, 0), 0) for k in range(250)]
  with pytest.warns(RuntimeWarning):
    env.reset(worlds=WorldBank(env, mat, [objs]))
  assert env.cfg.max_objects >= 512 and list(env.records()['nobj']) == [252] * 3
  env.check_errors()
  for t in range(6):
    env.step(_dev([5, 2, 4], env))
  w = env.export_worlds([0])
  assert w['objects'][0][0][0] == wc.PLAYER and len(w['objects'][0]) == 251
  env.reset(mask=[0, 1, 0], worlds=WorldBank(env, **w))
  back = env.export_worlds([1])
  assert np.array_equal(back['mat'], w['mat']) and back['objects'] == w['objects'] and np.array_equal(back['inventory'], w['inventory'])
  o = AuthoredOracle(seed=501, world=None)
  o.reset()
  o.world = dict(mat=w['mat'][0], objects=w['objects'][0], inventory=w['inventory'][0])
  o.reset()
  assert_same(env.snapshot(1), o.snapshot(), 'the copy')


def test_env_facade_and_run_random_play_authored_worlds(tmp_path, capsys):
  from crafter_amd import Env, run_random
  env = Env(seed=7)
  world = wc.garden()
  obs = env.reset(world=dict(mat=world['mat'], objects=world['objects']))
  o = AuthoredOracle(seed=7, world=world)
  assert np.array_equal(obs, o.reset())
  got = env.export_world()
  assert np.array_equal(got['mat'], world['mat']) and got['objects'][1:] == world['objects']
  with pytest.raises(ValueError):
    env.reset(world=dict(mat=world['mat'], objects=[('cow', 64, 0)]))
  assert np.array_equal(env.reset(), o.reset())   # the next episode is generated again: episode 2 of the seed
  o9 = AuthoredOracle(seed=9)   # worlds= together with seeds= / episodes=: reseeded first, then the authored reset
  o9.reset()
  o9.world = world
  assert np.array_equal(env.reset(seed=9, episode=2, world=dict(mat=world['mat'], objects=world['objects'])), o9.reset())
  assert_same(env._batch.snapshot(0), o9.snapshot(), 'reseeded and authored')
  wc.bank_of(dict(area=(64, 64)), range(3)).save(tmp_path / 'bank.npz')
  run_random.main(['--worlds', str(tmp_path / 'bank.npz'), '--envs', '4', '--length', '10', '--episodes', '1', '--seed', '3'])
  assert 'authored worlds' in capsys.readouterr().out
