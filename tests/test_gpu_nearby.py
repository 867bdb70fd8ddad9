"""BatchedEnv.nearby() / crafter_nearby on the device: against the numpy mirror of snapshot(i) (crafter_amd.nearby_host) on both
kernel instances, after reset, steps and a rollout; the states of the reference fixture reached by seed and tape against what
the untouched reference answered; masked rows and out=; that the query changes nothing; count(), Env.nearby and the ValueErrors;
and the two worked examples: screening levels, and a policy driven from the entity list alone."""
import numpy as np
import pytest
import torch

import crafter_amd
from crafter_amd import abi, state
from tests import nearby_cases as nc

pytestmark = pytest.mark.gpu


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def _mirror(env, distance, k, classes, numpy_slices):
  got = [state.nearby_host(env.snapshot(i), nc.N_MATERIALS, distance, k, classes, numpy_slices) for i in range(env.num_envs)]
  return np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), np.array([g[2] for g in got], np.int32)


def _assert_equal(got, want, what):
  for name, g, w in zip(('counts', 'ents', 'n'), got, want):
    g = g.cpu().numpy() if torch.is_tensor(g) else g
    assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.argwhere(g != w)
    assert not len(bad), f'{what}: {name} differs at {bad[:6].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}'


# ------------------------------------------------------------------ 1. the mirror, generated worlds
@pytest.mark.parametrize('n,area', [(8, (64, 64)), (4, (256, 256))], ids=['64x64-wave', '256x256-workgroup'])
def test_equals_the_mirror_of_snapshot(n, area):
  """After reset, after 40 step()s and after a rollout() with episodes of 16 steps (some rows are fresh episodes): K = 16 and K = 32,
  both window rules, a short window and a long one, equal the mirror of snapshot(i) for every row.  64 x 64 runs one wave per env
  over the slot table, 256 x 256 one workgroup per env, over objmap where the window is short."""
  env = _batched(n, area=area, seeds=list(range(500, 500 + n)), length=16, auto_reset=True)
  assert env.slot_map_derived == (area[0] == 64)
  env.reset()
  acts = np.random.RandomState(9).randint(0, 17, size=(80, n))
  total = 0
  for stage in ('reset', 'steps', 'rollout'):
    if stage == 'steps':
      for t in range(40):
        env.step(_dev(acts[t], env), info=False)
    if stage == 'rollout':
      env.rollout(_dev(acts[40:], env), obs=False)
      assert int(env.records()['episode'].min()) >= 4
    for k in (16, 32):
      for d, rule in ((4, False), (None, False), (4, True), (area[0] + 6, True)):
        got = env.nearby(d, k, nc.OBJECT_NAMES, numpy_slices=rule)
        assert [t.dtype for t in got] == [torch.int32, torch.int16, torch.int32]
        assert [tuple(t.shape) for t in got] == [(n, nc.N_CLASSES), (n, k, 6), (n,)]
        _assert_equal(got, _mirror(env, d, k, nc.ALL_OBJECTS, rule), f'{stage} k={k} d={d} numpy={rule}')
        total += int(got[2].sum())
    whole = env.nearby(None, k=0)[0]
    assert bool((whole[:, 0] == area[0] * area[1]).all()) and bool((whole[:, 1: nc.N_MATERIALS + 1].sum(1) == area[0] * area[1]).all())
    assert torch.equal(env.count('diamond'), whole[:, nc.CLASSES.index('diamond')]) and torch.equal(env.count(2), whole[:, 2])
  assert total > 100
  env.check_errors()


# ------------------------------------------------------------------ 2. the reference fixture
@pytest.mark.parametrize('area', [(64, 64), (42, 30)], ids=['64x64', '42x30'])
def test_fixture_states_on_the_device(area):
  """The recorded runs by seed and tape, one env each: at every recorded state the device's NUMPY windows give the material sets,
  class counts and object rows the untouched reference gave, and count() its World.count.  Then the poked states."""
  fix = nc.load_fixture()
  seeds = [s for a, s in nc.RUNS if a == area]
  entries = [fix[nc.run_key(area, s)] for s in seeds]
  env = _batched(len(seeds), area=area, seeds=seeds, auto_reset=False)
  env.reset()
  tapes = np.stack([nc.tape(s) for s in seeds], 1)

  def check(env, entries, states, what):
    got = [tuple(t.cpu().numpy() for t in env.nearby(d, 32, nc.OBJECT_NAMES, numpy_slices=True)) for d in nc.DISTANCES]
    whole = env.nearby(None, k=0)[0].cpu().numpy()
    for i, (entry, s) in enumerate(zip(entries, states)):
      assert whole[i, 1: nc.N_MATERIALS + 1].tolist() == entry['count'][s][1:].tolist(), (what, i)
      for di, d in enumerate(nc.DISTANCES):
        mats, by_type, rows, cells = nc.expected(entry, s, di, area)
        c, e, n = (g[i] for g in got[di])
        assert sum(1 << m for m in range(1, nc.N_MATERIALS + 1) if c[m]) == mats and c[0] == cells, (what, i, d)
        assert c[nc.N_MATERIALS + 1:].tolist() == by_type and n == len(rows), (what, i, d)
        assert [tuple(r) for r in e[:min(n, 32)].tolist()] == rows[:32] and not e[min(n, 32):].any(), (what, i, d)

  check(env, entries, [0] * len(seeds), 'reset')
  for t in range(nc.STEPS):
    env.step(_dev(tapes[t], env), info=False)
    if (t + 1) % nc.EVERY == 0:
      check(env, entries, [(t + 1) // nc.EVERY] * len(seeds), f'step {t + 1}')
  env.check_errors()
  positions = nc.poke_positions(area)
  poked = _batched(len(positions), area=area, seeds=[nc.POKE_SEED] * len(positions), auto_reset=False)
  poked.reset()
  xy = torch.tensor(positions, dtype=torch.int16, device=poked.device)
  poked.state['objs'][:, 1, 4:8] = xy.view(torch.uint8).reshape(len(positions), 4)   # the players' x, y (slot 1)
  entry = fix[f'{area[0]}x{area[1]}/poke']
  check(poked, [entry] * len(positions), list(range(len(positions))), 'poked')
  assert any(entry['mats'][s][di] == 0 for s in range(len(positions)) for di in range(len(nc.DISTANCES)))


# ------------------------------------------------------------------ 3. mask and out
def test_masked_rows_and_out():
  """Five envs, a mask naming rows {0, 3}, out= filled with poison: untouched rows keep it, rows beyond min(n, K) of a written row
  are zeros.  Bad arguments raise ValueError before anything is enqueued; the C boundary refuses what its header lists."""
  env = _batched(5, seeds=[31, 32, 33, 34, 35])
  env.reset()
  K = 12
  full = env.nearby(5, K)
  shapes = ((5, nc.N_CLASSES), torch.int32, 0x5E5E5E5E), ((5, K, 6), torch.int16, 0x5E5E), ((5,), torch.int32, 0x5E5E5E5E)
  out = tuple(torch.full(shape, fill, dtype=dt, device=env.device) for shape, dt, fill in shapes)
  mask = np.array([1, 0, 0, 1, 0], np.uint8)
  got = env.nearby(5, K, mask=mask, out=out)
  assert all(g is o for g, o in zip(got, out))
  keep = torch.from_numpy(mask.astype(bool)).to(env.device)
  for o, f, (_, _, fill) in zip(out, full, shapes):
    assert torch.equal(o[keep], f[keep]) and bool((o[~keep] == fill).all())
  counts, ents, n = (t.cpu().numpy() for t in out)
  for i in (0, 3):
    assert n[i] < K and not ents[i, n[i]:].any() and (ents[i, :n[i], 0] > nc.N_MATERIALS + 1).all()
  _assert_equal(tuple(t[keep] for t in out), tuple(w[[0, 3]] for w in _mirror(env, 5, K, nc.NOT_PLAYER, False)), 'masked rows')
  for kw in (dict(k=33), dict(k=-1), dict(classes=['tree']), dict(classes=['wood']), dict(distance=None, numpy_slices=True), dict(distance=1.5),
             dict(out=out[:2]), dict(out=(out[0], out[1].to(torch.int32), out[2])), dict(out=(out[0], out[1][:, :3], out[2])),
             dict(mask=np.ones(4, np.uint8))):
    with pytest.raises(ValueError):
      env.nearby(**{**dict(distance=5, k=K), **kw})
  with pytest.raises(ValueError):
    env.count('cow')
  with pytest.raises(ValueError):
    env.count(['coal', 'iron'])
  for o, f, (_, _, fill) in zip(out, full, shapes):   # nothing of the refused calls was written
    assert torch.equal(o[keep], f[keep]) and bool((o[~keep] == fill).all())
  from crafter_amd import lib as hiplib
  fn = hiplib.load().crafter_nearby
  c, e, m = (t.data_ptr() for t in out)
  for args, word in (((5, 0, nc.NOT_PLAYER, 33, c, e, m), 'k'), ((5, 2, nc.NOT_PLAYER, K, c, e, m), 'flags'), ((5, 0, 1 << 6, K, c, e, m), 'classes'),
                     ((-1, 1, nc.NOT_PLAYER, K, c, e, m), 'distance'), ((5, 0, nc.NOT_PLAYER, K, None, e, m), 'counts'),
                     ((5, 0, nc.NOT_PLAYER, K, c, None, m), 'ents or n'), ((5, 0, nc.NOT_PLAYER, K, c, e, None), 'ents or n')):
    assert fn(env._native.ptr, None, *args, None) != 0 and word in hiplib.last_error(hiplib.load(), env._native.ptr), word
  env.check_errors()


# ------------------------------------------------------------------ 4. read-only
def test_changes_nothing():
  """fingerprint(FP_ALL), obs and the state rows are identical before and after a call; of two copies of a batch, the one that
  queries between its steps stays bit-identical to the other over 40 steps."""
  seeds = list(range(700, 708))
  a, b = _batched(8, seeds=seeds, length=20), _batched(8, seeds=seeds, length=20)
  a.reset()
  b.reset()
  acts = np.random.RandomState(2).randint(0, 17, size=(40, 8)).astype(np.int32)
  for t in range(40):
    if t % 10 == 0:
      before = a.fingerprint(abi.FP_ALL).clone(), a.obs.clone(), a.state['rec'].clone(), a.state['objs'].clone(), a.state['mat'].clone()
      a.nearby(None, 32, nc.OBJECT_NAMES)
      a.nearby(3, 16, numpy_slices=True)
      after = a.fingerprint(abi.FP_ALL), a.obs, a.state['rec'], a.state['objs'], a.state['mat']
      assert all(torch.equal(x, y) for x, y in zip(before, after)), t
    else:
      a.nearby(6, 4, ['zombie'])
    ao, ar, ad = (x.clone() for x in a.step(_dev(acts[t], a), info=False)[:3])
    bo, br, bd = b.step(_dev(acts[t], b), info=False)[:3]
    assert torch.equal(ao, bo) and torch.equal(ar, br) and torch.equal(ad, bd), t
  assert torch.equal(a.fingerprint(abi.FP_ALL), b.fingerprint(abi.FP_ALL))
  assert torch.equal(a.state['rec'], b.state['rec']) and torch.equal(a.state['mt'], b.state['mt'])
  a.check_errors()


def test_env_nearby():
  env = crafter_amd.Env(seed=7)
  env.reset()
  counts, ents, n, by_name = env.nearby(7, 8)
  want = state.nearby_host(env._batch.snapshot(0), nc.N_MATERIALS, 7, 8)
  assert isinstance(n, int) and counts.dtype == np.int32 and ents.dtype == np.int16 and ents.shape == (8, 6)
  assert np.array_equal(counts, want[0]) and np.array_equal(ents, want[1]) and n == want[2]
  assert by_name['none'] == 225 and by_name['player'] == 1 and list(by_name) == nc.CLASSES and by_name['grass'] == counts[2]
  assert int(env._batch.count('coal')[0]) == env._world.count('coal')


def test_run_random_census(capsys):
  """run_random --census prints the reference's three "exist" lines for every env after the reset, from one call: the numbers
  are World.count of a batch with the same seed; with one env they repeat the lines the reference's script prints."""
  from crafter_amd import run_random
  run_random.main(['--envs', '3', '--episodes', '1', '--length', '20', '--seed', '2', '--census'])
  out = capsys.readouterr().out
  env = _batched(3, seed=2, length=20)
  env.reset()
  labels = (('Coal exist:    ', 'coal'), ('Iron exist:    ', 'iron'), ('Diamonds exist:', 'diamond'))   # (run_random.py:31-33)
  want = ''.join(f'Env {e}:\n' + ''.join(f'{label} {int(env.count(name)[e])}\n' for label, name in labels) for e in range(3))
  assert want in out and 'Episodes finished:' in out, out
  run_random.main(['--episodes', '1', '--length', '10', '--seed', '2', '--census'])
  lines = [line for line in capsys.readouterr().out.splitlines() if 'exist' in line]
  assert len(lines) == 6 and lines[:3] == lines[3:], lines


# ------------------------------------------------------------------ 5. the worked examples
def test_level_screen():
  """Screening levels for a curriculum: 64 seeds at once, one whole-world census and one zombie query pick the levels that hold a
  diamond and have no zombie within six cells of the start.  The choice equals the one computed from host snapshots.  (The
  generator keeps zombies farther than six cells from the start, so that screen turns on the diamonds; a second one -- two
  diamonds, no zombie within ten cells -- turns on both.)"""
  seeds = list(range(3000, 3064))
  env = _batched(64, auto_reset=False)
  env.reset(seeds=seeds)
  diamonds = env.nearby(None, k=0)[0][:, env.symbolic_names['classes'].index('diamond')]
  chosen = {6: (diamonds >= 1) & (env.nearby(6, k=1, classes=['zombie'])[2] == 0),
            10: (diamonds >= 2) & (env.nearby(10, k=1, classes=['zombie'])[2] == 0)}
  want = {6: [], 10: []}
  for i in range(64):
    snap = env.snapshot(i)
    _, px, py = snap['objects'][0][:3]
    found = int((snap['mat'] == 1 + nc.MATERIALS.index('diamond')).sum())
    for r, least in ((6, 1), (10, 2)):
      near = [o for o in snap['objects'] if o[0] == abi.T_ZOMBIE and abs(o[1] - px) <= r and abs(o[2] - py) <= r]
      want[r].append(found >= least and not near)
  assert chosen[6].cpu().tolist() == want[6] and chosen[10].cpu().tolist() == want[10]
  assert 0 < sum(want[6]) < 64 and 8 <= sum(want[10]) <= 56 and sum(want[10]) < sum(want[6]), (sum(want[6]), sum(want[10]))
  env.check_errors()


def _flee(ents, n, t, moves):
  """The policy, on tensors or arrays alike: one step away from the nearest zombie, along the axis on which it is farther off;
  with none in sight a stroll in a square."""
  dx, dy = ents[:, 0, 1], ents[:, 0, 2]
  along_x = abs(dx) >= abs(dy)
  away = (along_x * ((dx < 0) * moves['right'] + (dx >= 0) * moves['left']) +
          (~along_x) * ((dy < 0) * moves['down'] + (dy >= 0) * moves['up']))
  stroll = moves[('left', 'up', 'right', 'down')[t // 3 % 4]]
  return (n > 0) * away + (n == 0) * stroll


def test_entity_policy_step():
  """A flee-from-the-nearest-zombie policy driven from `ents` alone runs 50 steps with no host read, and ends in the states the same
  policy reaches when it is driven from nearby_host over downloaded snapshots."""
  seeds = list(range(900, 916))
  a, b = _batched(16, seeds=seeds, length=10000), _batched(16, seeds=seeds, length=10000)
  a.reset()
  b.reset()
  moves = {d: a.action_names.index(f'move_{d}') for d in ('left', 'right', 'up', 'down')}
  zombie = 1 << (nc.N_MATERIALS + nc.ZOMBIE)
  seen = torch.zeros(16, dtype=torch.int32, device=a.device)
  out = a.nearby(9, 1, ['zombie'])
  for t in range(50):
    _, ents, n = a.nearby(9, 1, ['zombie'], out=out)
    seen += (n > 0).to(torch.int32)
    a.step(_flee(ents.to(torch.int32), n, t, moves).to(torch.int32), info=False)
    host = [state.nearby_host(b.snapshot(i), nc.N_MATERIALS, 9, 1, zombie) for i in range(16)]
    acts = _flee(np.stack([h[1] for h in host]).astype(np.int32), np.array([h[2] for h in host]), t, moves)
    b.step(_dev(acts, b), info=False)
  assert torch.equal(a.fingerprint(abi.FP_ALL), b.fingerprint(abi.FP_ALL)) and torch.equal(a.state['objs'], b.state['objs'])
  assert int((seen > 0).sum()) >= 4 and int(seen.sum()) >= 20, seen.tolist()
  a.check_errors()
