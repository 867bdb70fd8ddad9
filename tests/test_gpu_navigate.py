"""BatchedEnv.navigate() / crafter_navigate on the device: against the Python mirror of snapshot(i) (crafter_amd.navigate_host) on
generated worlds of both geometries and both object paths, the authored worlds of tests/navigate_cases.py against their literal
values, that the query changes nothing, the cross-check with legal_actions(), mask / out / the ValueErrors / Env.navigate, and the
worked example: a scripted woodcutter."""
import numpy as np
import pytest
import torch

import crafter_amd
from crafter_amd import abi, state
from tests import navigate_cases as nc

pytestmark = pytest.mark.gpu


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def _mirror(env, targets, passable=None):
  sets, walk = env._check_targets(env.symbolic_names['classes'], nc.N_MATERIALS, nc.WALKABLE, targets, passable)
  moves = [env.action_names.index(f'move_{d}') for d in ('left', 'right', 'up', 'down')]
  got = [state.navigate_host(env.snapshot(i), nc.N_MATERIALS, sets, walk, moves) for i in range(env.num_envs)]
  return tuple(np.array([g[j] for g in got]).astype(dt) for j, dt in enumerate((np.int32, np.int32, np.uint8)))


def _assert_equal(got, want, what):
  for name, g, w in zip(('dist', 'first', 'facing'), got, want):
    g = g.cpu().numpy() if torch.is_tensor(g) else g
    bad = np.argwhere(g != w)
    assert not len(bad), f'{what}: {name} differs at (env, target) {bad[:6].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}'


def _no_sleep_actions(rs, shape):
  a = rs.randint(0, 16, size=shape)
  return (a + (a >= 6)).astype(np.int32)   # every action but sleep: the rows stay awake


# ------------------------------------------------------------------ 1. the mirror, generated worlds
@pytest.mark.parametrize('n,area', [(32, (64, 64)), (8, (48, 40)), (4, (80, 72)), (4, (144, 144)), (4, (256, 256))],
                         ids=['64x64', '48x40', '80x72-lds', '144x144-lds', '256x256-lds'])
def test_equals_the_mirror_of_snapshot(n, area):
  """After reset and after a 40-step rollout with episodes of 16 steps (some rows are fresh episodes): K = 16 and K = 1 equal the
  mirror of snapshot(i) for every row.  64 x 64 and 48 x 40 run in registers; the others in LDS, 80 x 72 through the slot table,
  the larger ones through objmap.  The compared pairs hold a -1, a walk of more than 20 steps and a faced target."""
  env = _batched(n, area=area, seeds=list(range(500, 500 + n)), length=16, auto_reset=True)
  assert env.slot_map_derived == (area[0] < 144)
  env.reset()
  seen = []
  for stage in range(2):
    got = env.navigate(nc.TARGETS16)
    assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.uint8] and all(tuple(t.shape) == (n, 16) for t in got)
    _assert_equal(got, _mirror(env, nc.TARGETS16), f'stage {stage}, K = 16')
    one = env.navigate(['tree'])
    assert all(torch.equal(o[:, 0], g[:, 5]) for o, g in zip(one, got))
    seen.append([t.cpu().numpy() for t in got])
    if stage == 0:
      env.rollout(_dev(np.random.RandomState(9).randint(0, 17, size=(40, n)), env), obs=False)
      assert int(env.records()['episode'].min()) >= 3
  dist = np.concatenate([g[0] for g in seen])
  facing = np.concatenate([g[2] for g in seen])
  assert (dist == -1).any() and (dist > 20).any() and (facing == 1).any() and (dist != 0).all()
  assert (dist[:, nc.TARGETS16.index('player')] == -1).all()
  env.check_errors()


# ------------------------------------------------------------------ 2. authored worlds
@pytest.mark.parametrize('geo', [dict(area=(64, 64)), dict(area=(42, 30), view=(7, 9), size=(84, 72)), dict(area=(80, 72))],
                         ids=['64x64', '42x30', '80x72-lds'])
def test_authored_worlds(geo):
  """The cases (a) .. (g) of tests/navigate_cases.py through reset(worlds=...): the literal values."""
  W, H = geo['area']
  cases = nc.cases(W, H)
  env = _batched(len(cases), seeds=[0] * len(cases), auto_reset=False, **geo)
  bank = crafter_amd.WorldBank(env, np.stack([c['mat'] for c in cases]), [c['objects'] for c in cases])
  env.reset(worlds=bank, world_ids=list(range(len(cases))))
  env.check_errors()
  queries = {}
  for i, c in enumerate(cases):
    queries.setdefault((tuple(map(str, c['targets'])), str(c['passable'])), (c['targets'], c['passable'], []))[2].append(i)
  for targets, passable, rows in queries.values():
    got = [t.cpu().numpy() for t in env.navigate(targets, passable)]
    for i in rows:
      assert [tuple(int(g[i, k]) for g in got) for k in range(len(targets))] == [tuple(e) for e in cases[i]['expect']], cases[i]['name']
  assert cases[0]['expect'][0][0] == len(range(0, W, 2)) * (H + 1) - 2   # the serpentine's length: 2078 at 64 x 64


# ------------------------------------------------------------------ 3. read-only
def test_changes_nothing():
  """fingerprint(FP_ALL), obs and the rec bytes are identical before and after a call; of two copies of a batch, the one that
  calls navigate() between its steps stays bit-identical to the other over 50 steps."""
  seeds = list(range(700, 708))
  a, b = _batched(8, seeds=seeds, length=20), _batched(8, seeds=seeds, length=20)
  a.reset()
  b.reset()
  acts = np.random.RandomState(2).randint(0, 17, size=(50, 8)).astype(np.int32)
  for t in range(50):
    if t % 10 == 0:
      before = a.fingerprint(abi.FP_ALL).clone(), a.obs.clone(), a.state['rec'].clone(), a.state['objs'].clone(), a.state['mat'].clone()
      a.navigate(nc.TARGETS16)
      after = a.fingerprint(abi.FP_ALL), a.obs, a.state['rec'], a.state['objs'], a.state['mat']
      assert all(torch.equal(x, y) for x, y in zip(before, after)), t
    else:
      a.navigate(['tree', 'cow'])
    ao, ar, ad = (x.clone() for x in a.step(_dev(acts[t], a), info=False)[:3])
    bo, br, bd = b.step(_dev(acts[t], b), info=False)[:3]
    assert torch.equal(ao, bo) and torch.equal(ar, br) and torch.equal(ad, bd), t
  assert torch.equal(a.fingerprint(abi.FP_ALL), b.fingerprint(abi.FP_ALL))
  assert torch.equal(a.state['rec'], b.state['rec']) and torch.equal(a.state['mt'], b.state['mt'])
  a.check_errors()


# ------------------------------------------------------------------ 4. the cross-check with legal_actions()
def test_first_move_is_a_legal_action():
  """Wherever dist > 1, legal_actions()[e, first] == 1: a legal move is one that changes the cell, and the first step of a walk
  goes onto a free walkable cell.  (The query ignores sleeping, the mask does not: the rows are kept awake.)"""
  env = _batched(32, seeds=list(range(800, 832)))
  env.reset()
  rs = np.random.RandomState(12)
  checked = 0
  for stage in range(3):
    dist, first, _ = env.navigate(nc.TARGETS16)
    legal = env.legal_actions()
    assert not env.symbolic()[1][:, env.symbolic_names['stats'].index('sleeping')].any()
    far = dist > 1
    assert bool(torch.gather(legal, 1, first.clamp(min=0).long())[far].all())
    assert bool((first[dist < 0] == -1).all()) and bool((first[dist > 0] >= 1).all())
    checked += int(far.sum())
    env.rollout(_dev(_no_sleep_actions(rs, (25, 32)), env), obs=False)
  assert checked > 500


# ------------------------------------------------------------------ 5. mask, out, arguments, Env
def test_mask_out_and_arguments():
  """Five envs (four to a workgroup), a mask naming rows {0, 3}, out= pre-filled with a sentinel: the other rows stay untouched.
  Bad targets, out and mask raise ValueError before anything is enqueued."""
  env = _batched(5, seeds=[31, 32, 33, 34, 35])
  env.reset()
  targets = ['tree', ['water', 'cow'], 'stone']
  full = env.navigate(targets)
  out = tuple(torch.full((5, 3), 0x5E, dtype=dt, device=env.device) for dt in (torch.int32, torch.int32, torch.uint8))
  mask = np.array([1, 0, 0, 1, 0], np.uint8)
  got = env.navigate(targets, mask=mask, out=out)
  assert all(g is o for g, o in zip(got, out))
  keep = torch.from_numpy(mask.astype(bool)).to(env.device)
  for o, f in zip(out, full):
    assert torch.equal(o[keep], f[keep]) and bool((o[~keep] == 0x5E).all())
  assert env.class_mask('tree') == 1 << 6 and env.class_mask(['coal', 9, 'zombie']) == (1 << 8 | 1 << 9 | 1 << 15)
  ids = env.navigate([6, [1, 14], env.symbolic_names['classes'].index('stone')])
  assert all(torch.equal(i, f) for i, f in zip(ids, full))
  lava = env.navigate(targets, passable=['grass', 'sand', 'path', 'lava'])
  assert bool((lava[0][full[0] > 0] <= full[0][full[0] > 0]).all())
  for bad in ([], ['tree'] * 17, ['wood'], ['none'], [0], [19], 'tree'):
    with pytest.raises(ValueError):
      env.navigate(bad)
  with pytest.raises(ValueError):
    env.navigate(targets, passable=['cow'])
  with pytest.raises(ValueError):
    env.navigate(targets, out=out[:2])
  with pytest.raises(ValueError):
    env.navigate(targets, out=(out[0], out[1].to(torch.int64), out[2]))
  with pytest.raises(ValueError):
    env.navigate(targets, out=tuple(o[:, :2] for o in out))
  with pytest.raises(ValueError):
    env.navigate(targets, mask=np.ones(4, np.uint8))
  from crafter_amd import lib as hiplib
  fn = hiplib.load().crafter_navigate   # the C boundary's own refusals, with a message that names the argument
  host = (hiplib.C.c_uint32 * 2)(1 << 6, 1 << 19)
  args = lambda k, passable, d: (env._native.ptr, None, hiplib.C.cast(host, hiplib.C.c_void_p), k, passable, d, full[1].data_ptr(), None, None)
  for call, word in ((args(0, 4, full[0].data_ptr()), 'k'), (args(2, 4, full[0].data_ptr()), 'targets'), (args(1, 5, full[0].data_ptr()), 'passable'),
                     (args(1, 4, None), 'dist')):
    assert fn(*call) != 0 and word in hiplib.last_error(hiplib.load(), env._native.ptr)
  env.check_errors()


def test_env_navigate():
  env = crafter_amd.Env(seed=7)
  env.reset()
  dist, first, facing = env.navigate(['tree', 'water', 'player'])
  assert dist.shape == first.shape == facing.shape == (3,) and dist.dtype == np.int32 and facing.dtype == bool
  want = _mirror(env._batch, ['tree', 'water', 'player'])
  assert dist.tolist() == want[0][0].tolist() and first.tolist() == want[1][0].tolist() and facing.tolist() == want[2][0].astype(bool).tolist()
  assert dist[2] == -1 and first[2] == -1


# ------------------------------------------------------------------ 6. the worked example
def test_scripted_woodcutter():
  """Sixteen authored worlds of sand, stone, water and trees, the player the only object: nothing ever spawns, the worlds are
  deterministic.  Following `first`, dist falls by exactly one per step down to 1; after dist0 steps the player faces a tree; the
  next `do` adds one wood and unlocks collect_wood -- in every env."""
  n = 16
  env = _batched(n, seeds=list(range(n)), auto_reset=False)
  mats, objects = nc.woodcutter_worlds(64, 64, n, seed=4)
  env.reset(worlds=crafter_amd.WorldBank(env, np.stack(mats), objects), world_ids=list(range(n)))
  do, noop = env.action_names.index('do'), env.action_names.index('noop')
  wood, unlocked = env.item_names.index('wood'), env.achievement_names.index('collect_wood')
  dist0 = env.navigate(['tree'])[0][:, 0].clone()
  assert bool((dist0 >= 1).all()) and int(dist0.max()) <= 40 and int(dist0.max()) >= 4
  for t in range(int(dist0.max()) + 1):
    dist, first, facing = (x[:, 0] for x in env.navigate(['tree']))
    walking, arrived = t < dist0, t == dist0
    assert torch.equal(dist[walking], (dist0 - t).clamp(min=1)[walking]), t
    assert bool((facing[arrived] == 1).all()) and bool((dist[arrived] == 1).all()), t
    inv_before = env.info()['inventory'][:, wood].clone()
    action = torch.where(walking, first, torch.where(arrived, torch.full_like(first, do), torch.full_like(first, noop)))
    assert bool((action >= 0).all())
    env.step(action.to(torch.int32), info=False)
    info = env.info()
    assert torch.equal(info['inventory'][:, wood] - inv_before, arrived.to(inv_before.dtype)), t
    assert bool((info['achievements'][arrived, unlocked] >= 1).all()), t
  info = env.info()
  assert bool((info['inventory'][:, wood] == 1).all()) and bool((info['achievements'][:, unlocked] >= 1).all())
  assert len(env.snapshot(0)['objects']) == 1   # the player, still alone
  env.check_errors()
