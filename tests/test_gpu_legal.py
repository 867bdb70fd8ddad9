"""BatchedEnv.legal_actions() / crafter_legal_actions on the device against the oracle's restatement (tests/legal_ref.py), byte
for byte: the default instance with gifts, a small world with its border and the poked edge states, a generic view geometry,
the objmap path of the global-memory instance, mask / out and the batch tail, read-only-ness, auto-reset; what the mask means
on the whole path, with no restatement (copies of a state stepped with every action); the facades and run_random's flag."""
import functools

import numpy as np
import pytest
import torch

from crafter_amd import state
from tests import legal_ref as lr
from tests import symbolic_ref as sr

pytestmark = pytest.mark.gpu
GENERIC = dict(view=(7, 9), size=(84, 72), area=(32, 32))


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


@functools.lru_cache(None)
def oracle_trace(case, area=None, view=(9, 9), size=(64, 64)):
  return lr.oracle_trace(case, area=area, view=view, size=size)


def assert_rows(got, want, what):
  g = got.cpu().numpy() if torch.is_tensor(got) else got
  assert g.dtype == np.uint8 and g.shape == want.shape, what
  bad = np.argwhere(g != want)
  assert not len(bad), f'{what}: differs, first at {bad[:3].tolist()}: {g[tuple(bad[0][:-1])].tolist()} != {want[tuple(bad[0][:-1])].tolist()}'


def _run_cases(cases, n_steps, **geo):
  """One batch with one env per entry of `cases`, each playing its case's tape (noop behind its end) with its gifts written
  into the batch's own state rows and its plants poked there; -> (env, legal [T + 1, N, n_actions]) taken through out= after
  reset and after every step."""
  tapes = [lr.tape(c) for c in cases]
  n = len(cases)
  env = _batched(n, seeds=[t[2] for t in tapes], auto_reset=False, **geo)
  items = list(env.item_names)
  inv0 = env._off['inv']
  L = torch.zeros((n_steps + 1, n, env.num_actions), dtype=torch.uint8, device=env.device)
  env.reset()
  env.legal_actions(out=L[0])
  for t in range(n_steps):
    acts = np.zeros(n, np.int32)
    for i, (a, gifts, _, _, poke) in enumerate(tapes):
      if t >= len(a):
        continue
      acts[i] = a[t]
      for item, amount in gifts.get(t, {}).items():
        env._rec_i32[i, inv0 + items.index(item)] = amount
      if t in poke:
        objs = state.objs_view(env.state['objs'][i:i + 1].cpu().numpy())
        sr.poke_objs(objs[0], env.records()['nobj'][i])
        env.state['objs'][i:i + 1].copy_(torch.from_numpy(objs.view(np.uint8).reshape(1, -1, 16)))
    env.step(_dev(acts, env), info=False)
    env.legal_actions(out=L[t + 1])
  env.check_errors()
  return env, L.cpu().numpy()


def _check_cases(cases, L, **geo):
  for i, case in enumerate(cases):
    want = oracle_trace(case, **geo)
    assert_rows(L[:want.shape[0], i], want, f'env {i} ({case})')


def test_default_instance_three_tapes_twice():
  cases = ['builder', 'sleeper', 'fighter'] * 2
  env, L = _run_cases(cases, 400)
  assert env.step_instance == 'crafter_step_kernel<1, 1, 1>' and env.slot_map_derived
  _check_cases(cases, L, area=(64, 64))
  assert L[:, 0].min(axis=0).tolist()[1:] == [0] * 16 and L[:, 0].max(axis=0).tolist() == [1] * 17   # builder: every action both ways


def test_small_world_and_its_border():
  cases = ['fighter', 'builder']
  env, L = _run_cases(cases, 400, area=(16, 16))
  _check_cases(cases, L, area=(16, 16))


def test_poked_edge_states():
  """Copies of the reset state made with copy_envs, poked and observed, never stepped."""
  edges = lr.edge_states()
  n = 1 + len(edges)
  env = _batched(n, seeds=[lr.EDGE_SEED] * n, area=lr.EDGE_AREA, auto_reset=False)
  assert env.slot_map_derived
  env.reset()
  env.copy_envs([0] * len(edges), list(range(1, n)))
  W, H = lr.EDGE_AREA
  inv0 = env._off['inv']
  for k, edge in enumerate(edges):
    i = k + 1
    mat = env.state['mat'][i].cpu().numpy().reshape(W, H).copy()
    objs = state.objs_view(env.state['objs'][i:i + 1].cpu().numpy())
    inv = env._rec_i32[i, inv0: inv0 + len(env.item_names)].cpu().numpy()
    lr.edge_arrays(edge, env.rules, mat, objs[0], inv)
    env.state['mat'][i].copy_(torch.from_numpy(mat.reshape(-1)))
    env.state['objs'][i:i + 1].copy_(torch.from_numpy(objs.view(np.uint8).reshape(1, -1, 16)))
    env._rec_i32[i, inv0: inv0 + len(inv)] = torch.from_numpy(inv).to(env.device)
  got = env.legal_actions().cpu().numpy()
  want = lr.edge_trace()
  assert_rows(got[1:], want, 'edge states')
  makes = [a for a, name in enumerate(env.action_names) if name.startswith('make_')]
  for row, e in zip(got[1:], edges):
    assert (row[makes] == (0 if 0 in e['pos'] else 1)).all(), (e, row.tolist())


def test_generic_geometry():
  cases = ['builder', 'fighter']
  env, L = _run_cases(cases, 200, **GENERIC)
  assert env.step_instance != 'crafter_step_kernel<1, 1, 1>'
  for i, case in enumerate(cases):
    assert_rows(L[:201, i], oracle_trace(case, **GENERIC)[:201], f'env {i} ({case})')


def test_objmap_path_large_world():
  """area (256, 256): the global-memory instance, objmap is state."""
  import copy
  from oracle.crafter_oracle import OracleEnv
  env = _batched(2, area=(256, 256), seeds=[3, 3], auto_reset=False)
  assert not env.slot_map_derived
  orcs = [OracleEnv(area=(256, 256), seed=3)]
  orcs[0].reset()
  orcs.append(copy.deepcopy(orcs[0]))
  env.reset()
  acts = np.random.RandomState(9).randint(0, 17, size=(40, 2)).astype(np.int32)
  for t in range(-1, 40):
    if t >= 0:
      env.step(_dev(acts[t], env), info=False)
      for i, o in enumerate(orcs):
        o.step(int(acts[t, i]))
    assert_rows(env.legal_actions(), np.stack([lr.legal_of(o) for o in orcs]), f'step {t}')
  env.check_errors()


def test_batch_tail_mask_and_out():
  """Five envs (four per workgroup), a row mask, out= pre-filled with 0xFF; out must be exactly right."""
  seeds = [31, 32, 33, 34, 35]
  env = _batched(5, seeds=seeds)
  env.reset()
  acts = np.random.RandomState(4).randint(0, 17, size=(20, 5)).astype(np.int32)
  for t in range(20):
    env.step(_dev(acts[t], env), info=False)
  full = env.legal_actions()
  assert full.dtype == torch.uint8 and tuple(full.shape) == (5, 17) and bool((full[:, 0] == 1).all()) and int(full.max()) == 1
  L = torch.full((5, 17), 0xFF, dtype=torch.uint8, device=env.device)
  mask = np.array([1, 0, 1, 1, 0], np.uint8)
  assert env.legal_actions(mask=mask, out=L) is L
  keep = torch.from_numpy(mask.astype(bool)).to(env.device)
  assert torch.equal(L[keep], full[keep]) and bool((L[~keep] == 0xFF).all())
  good = torch.zeros_like(full)
  wide = torch.zeros((5, 34), dtype=torch.uint8, device=env.device)
  for bad in (good.to(torch.int8), good.to(torch.bool), good[:4], good[:, :-1], wide[:, ::2], good.cpu(), good.cpu().numpy()):
    with pytest.raises(ValueError):
      env.legal_actions(out=bad)
  with pytest.raises(ValueError):
    env.legal_actions(mask=np.ones(4, np.uint8))


def test_read_only():
  """save_state() before and after three calls is byte-identical; twins, one asked for its mask after every step, stay equal in
  every output and every byte of state."""
  seeds = [7, 8, 9, 10]
  a, b = _batched(4, seeds=seeds), _batched(4, seeds=seeds)
  a.reset()
  b.reset()
  acts = np.random.RandomState(1234 + 7).choice([0, 0, 6, 1, 2, 3, 4, 5, 5], size=(120, 4)).astype(np.int32)
  for t in range(120):
    a.step(_dev(acts[t], a), info=False)
    b.step(_dev(acts[t], b), info=False)
    a.legal_actions()
  before = a.save_state()
  for _ in range(3):
    a.legal_actions()
  after = a.save_state()
  assert set(before.tensors) == set(after.tensors)
  for name in before.tensors:
    assert torch.equal(before.tensors[name], after.tensors[name]), name
  assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done)
  for name in ('mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census'):
    assert torch.equal(a.state[name], b.state[name]), name


def test_auto_reset_describes_the_new_episode():
  from oracle.crafter_oracle import OracleEnv
  seeds = [21, 22, 23, 24]
  env = _batched(4, seeds=seeds, length=30, auto_reset=True)
  orcs = [OracleEnv(seed=s, length=30) for s in seeds]
  for o in orcs:
    o.reset()
  env.reset()
  acts = np.random.RandomState(2).randint(0, 17, size=(100, 4)).astype(np.int32)
  resets = 0
  for t in range(100):
    _, _, done, _ = env.step(_dev(acts[t], env), info=False)
    legal = env.legal_actions()
    for i, o in enumerate(orcs):
      if o.step(int(acts[t, i]))[2]:
        o.reset()
        resets += 1
        assert bool(done[i])
    assert_rows(legal, np.stack([lr.legal_of(o) for o in orcs]), f'step {t}')
  assert resets >= 12
  ps = env.pool_status()
  assert ps['state'] == 'running' and ps['adopted'] > 0, ps
  env.check_errors()


@pytest.mark.parametrize('case', ['builder', 'sleeper'])
def test_behaviour_whole_path(case):
  """What the mask means, with no restatement: at every 10th state of the tape, row 0 is copied into rows 1 .. 17, which are
  then stepped with actions 0 .. 16.  A non-move action with legal == 0 leaves its row byte-identical to the noop row (every
  saved byte of state, obs, reward, done); a move is legal iff the player's position changed; a legal non-move action's row
  differs from the noop row -- except `do` on a creature (the same step's balancing may despawn the zombie that was hit: 1 in
  3,854 legal non-move cases on the reference), allowed in at most 1 % of the `do`-on-a-creature rows."""
  acts, gifts, seed, area, _ = lr.tape(case)
  env = _batched(18, seeds=[seed] * 18, area=area, auto_reset=False)
  names = list(env.action_names)
  assert len(names) == 17
  moves = [a for a, n in enumerate(names) if n.startswith('move_')]
  do = names.index('do')
  items, inv0 = list(env.item_names), env._off['inv']
  gw, gh = env.symbolic_shape[0][1:]
  creatures = [env.symbolic_names['classes'].index(n) for n in ('cow', 'zombie', 'skeleton')]
  env.reset()
  rows = list(range(1, 18))
  checked = dict(illegal=0, legal=0, moves=0, creature_rows=0, creature_same=0)
  for t, a in enumerate(acts):
    for item, amount in gifts.get(t, {}).items():
      env._rec_i32[0, inv0 + items.index(item)] = amount
    step_acts = np.zeros(18, np.int32)
    step_acts[0] = a
    sample = t % 10 == 0
    if sample:
      env.copy_envs([0] * 17, rows)
      legal = env.legal_actions().cpu().numpy()
      assert (legal[1:] == legal[0]).all()
      legal = legal[0]
      local, stats = (x[0].cpu().numpy() for x in env.symbolic())
      fx, fy = int(stats[len(items)]), int(stats[len(items) + 1])
      on_creature = int(local[0, gw // 2 + fx, gh // 2 + fy]) in creatures
      pos = env.info()['player_pos'].cpu().numpy().copy()
      step_acts[1:] = np.arange(17)
    env.step(_dev(step_acts, env), info=False)
    if not sample:
      continue
    store = env.save_state(rows)
    tensors = {k: v.cpu().numpy().reshape(17, -1) for k, v in store.tensors.items()}
    same = np.array([all(np.array_equal(v[b], v[0]) for v in tensors.values()) for b in range(17)])
    moved = (env.info()['player_pos'].cpu().numpy()[1:] != pos[1:]).any(axis=1)
    for b in range(1, 17):
      if b in moves:
        assert bool(legal[b]) == bool(moved[b]), (t, names[b], legal.tolist())
        checked['moves'] += 1
      elif not legal[b]:
        assert same[b], (t, names[b], [k for k, v in tensors.items() if not np.array_equal(v[b], v[0])])
        checked['illegal'] += 1
      else:
        checked['legal'] += 1
        if b == do and on_creature:
          checked['creature_rows'] += 1
          checked['creature_same'] += int(same[b])
        else:
          assert not same[b], (t, names[b], legal.tolist())
  env.check_errors()
  print(case, checked)
  assert checked['illegal'] > 100 and checked['legal'] > 20 and checked['moves'] == 4 * ((len(acts) + 9) // 10)
  assert checked['creature_same'] <= 0.01 * checked['creature_rows'], checked


def test_facades(monkeypatch, capsys):
  from crafter_amd import BatchedEnv, Env, VecEnvView, run_random
  from oracle.crafter_oracle import OracleEnv
  e, orc = Env(seed=51), OracleEnv(seed=51)
  e.reset()
  orc.reset()
  for a in (2, 2, 5, 6, 3):
    e.step(a)
    orc.step(a)
    legal = e.legal_actions()
    assert isinstance(legal, np.ndarray) and legal.dtype == bool and legal.shape == (17,)
    assert legal.tolist() == lr.legal_of(orc).astype(bool).tolist(), a
  seeds = [52, 53, 54]
  vec = VecEnvView(3, seeds=seeds)
  orcs = [OracleEnv(seed=s) for s in seeds]
  for o in orcs:
    o.reset()
  vec.reset()
  for t in range(5):
    acts = [(t + i) % 17 for i in range(3)]
    vec.step(np.array(acts))
    for o, a in zip(orcs, acts):
      o.step(a)
  masks = vec.action_masks()
  want = np.stack([lr.legal_of(o) for o in orcs]).astype(bool)
  assert isinstance(masks, np.ndarray) and masks.dtype == bool and np.array_equal(masks, want)
  listed = vec.env_method('action_masks')
  assert isinstance(listed, list) and len(listed) == 3 and np.array_equal(np.stack(listed), want)
  assert np.array_equal(np.stack(vec.env_method('action_masks', indices=[2, 0])), want[[2, 0]])
  assert np.array_equal(vec.env_method('action_masks', indices=1)[0], want[1])
  for name in ('get_wrapper_attr', 'render', 'action_mask'):
    with pytest.raises(AttributeError):
      vec.env_method(name)
  # run_random --legal: every action it emits had its mask byte set
  seen = dict(steps=0, actions=set())
  step = BatchedEnv.step

  def checked_step(self, actions, *a, **k):
    legal = self.legal_actions()
    assert bool(legal.gather(1, actions.to(torch.int64).reshape(-1, 1)).all()), (actions.tolist(), legal.tolist())
    seen['steps'] += 1
    seen['actions'] |= set(actions.tolist())
    return step(self, actions, *a, **k)
  monkeypatch.setattr(BatchedEnv, 'step', checked_step)
  run_random.main(['--envs', '4', '--seed', '3', '--length', '60', '--legal'])
  assert seen['steps'] >= 60 and len(seen['actions']) > 6, seen
  assert 'Episodes finished: 4' in capsys.readouterr().out
  # ... and with one env, through the Env facade (whose step() goes through the checked BatchedEnv.step)
  seen.update(steps=0, actions=set())
  run_random.main(['--seed', '3', '--length', '40', '--legal'])
  out = capsys.readouterr().out
  assert f"Episode length: {seen['steps']}" in out and 5 <= seen['steps'] <= 40 and len(seen['actions']) > 1, (seen, out)
