"""BatchedEnv.symbolic() / crafter_symbolic on the device against the oracle's restatement (tests/symbolic_ref.py), bit for
bit (floats compared as words): the default instance with gifts and the plant poke, cells outside a small world, a generic
view geometry, the objmap path of the global-memory instance, auto-reset, read-only-ness, mask / out, batch tails, the
facade and rollout()."""
import copy
import functools

import numpy as np
import pytest
import torch

from crafter_amd import state
from tests import symbolic_ref as sr
from tests.parity import assert_same

pytestmark = pytest.mark.gpu
GENERIC = dict(view=(7, 9), size=(84, 72), area=(32, 32))


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


@functools.lru_cache(None)
def oracle_trace(case, area=None, view=(9, 9), size=(64, 64)):
  return sr.oracle_trace(case, area=area, view=view, size=size)


def assert_rows(local, stats, want_local, want_stats, what):
  """local / stats: device tensors or numpy arrays of any leading shape, against numpy arrays of the same shape."""
  l = local.cpu().numpy() if torch.is_tensor(local) else local
  s = stats.cpu().numpy() if torch.is_tensor(stats) else stats
  assert l.dtype == np.uint8 and s.dtype == np.float32 and l.shape == want_local.shape and s.shape == want_stats.shape, what
  bad = np.argwhere(l != want_local)
  assert not len(bad), f'{what}: local differs, first at {bad[:3].tolist()}'
  bad = np.argwhere(s.view(np.uint32) != want_stats.view(np.uint32))
  assert not len(bad), f'{what}: stats differ, first at {bad[:3].tolist()}'


def _run_cases(cases, n_steps, **geo):
  """One batch with one env per entry of `cases`, each playing its case's tape (noop behind its end) with its gifts written
  into the batch's own state rows and its plants poked there; -> (env, locals [T + 1, N, ...], stats [T + 1, N, ...]) taken
  through out= after reset and after every step."""
  tapes = [sr.tape(c) for c in cases]
  n = len(cases)
  env = _batched(n, seeds=[t[2] for t in tapes], auto_reset=False, **geo)
  items = list(env.item_names)
  inv0 = env._off['inv']
  ls, ss = env.symbolic_shape
  L = torch.zeros((n_steps + 1, n) + ls, dtype=torch.uint8, device=env.device)
  S = torch.zeros((n_steps + 1, n) + ss, dtype=torch.float32, device=env.device)
  env.reset()
  env.symbolic(out=(L[0], S[0]))
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
    env.symbolic(out=(L[t + 1], S[t + 1]))
  env.check_errors()
  return env, L.cpu().numpy(), S.cpu().numpy()


def _check_cases(cases, L, S, **geo):
  for i, case in enumerate(cases):
    want_local, want_stats = oracle_trace(case, **geo)
    rows = want_local.shape[0]
    assert_rows(L[:rows, i], S[:rows, i], want_local, want_stats, f'env {i} ({case})')


def test_default_instance_three_tapes_twice():
  cases = ['sleeper', 'fighter', 'planter'] * 2
  env, L, S = _run_cases(cases, 400)
  assert env.step_instance == 'crafter_step_kernel<1, 1, 1>' and env.slot_map_derived
  _check_cases(cases, L, S, area=(64, 64))
  assert ((L[:, 2, 0] == 18) & (L[:, 2, 1] == 1)).any(), 'the poke must show a ripe plant'


def test_cells_outside_the_world():
  env, L, S = _run_cases(['fighter'], 200, area=(16, 16))
  _check_cases(['fighter'], L, S, area=(16, 16))
  assert sum(1 for t in range(1, 201) if (L[t, 0, 0] == 0).any()) >= 100


def test_generic_geometry():
  env, L, S = _run_cases(['fighter'], 200, **GENERIC)
  assert env.symbolic_shape == ((2, 7, 6), (20,))
  _check_cases(['fighter'], L, S, **GENERIC)


def test_objmap_path_large_world():
  """area (256, 256): the global-memory instance, objmap is state."""
  from oracle.crafter_oracle import OracleEnv
  env = _batched(2, area=(256, 256), seeds=[3, 3], auto_reset=False)
  assert not env.slot_map_derived
  orcs = [OracleEnv(area=(256, 256), seed=3)]
  orcs[0].reset()
  orcs.append(copy.deepcopy(orcs[0]))
  env.reset()
  acts = np.random.RandomState(9).randint(0, 17, size=(60, 2)).astype(np.int32)
  for t in range(-1, 60):
    if t >= 0:
      env.step(_dev(acts[t], env), info=False)
      for i, o in enumerate(orcs):
        o.step(int(acts[t, i]))
    want = [sr.symbolic_of(o) for o in orcs]
    local, stats = env.symbolic()
    assert_rows(local, stats, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), f'step {t}')
  env.check_errors()


@pytest.mark.parametrize('gen_period', [0, -1])
def test_auto_reset_describes_the_new_episode(gen_period):
  from oracle.crafter_oracle import OracleEnv
  seeds = [21, 22, 23, 24]
  env = _batched(4, seeds=seeds, length=30, auto_reset=True, gen_period=gen_period)
  orcs = [OracleEnv(seed=s, length=30) for s in seeds]
  for o in orcs:
    o.reset()
  env.reset()
  acts = np.random.RandomState(2).randint(0, 17, size=(100, 4)).astype(np.int32)
  resets = 0
  for t in range(100):
    _, _, done, _ = env.step(_dev(acts[t], env), info=False)
    local, stats = env.symbolic()
    for i, o in enumerate(orcs):
      if o.step(int(acts[t, i]))[2]:
        o.reset()
        resets += 1
        assert bool(done[i])
    want = [sr.symbolic_of(o) for o in orcs]
    assert_rows(local, stats, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), f'step {t}')
  assert resets >= 12
  ps = env.pool_status()
  if gen_period < 0:
    assert ps['state'] == 'off'
  else:
    assert ps['state'] == 'running' and ps['adopted'] > 0, ps
  env.check_errors()


def test_read_only():
  """Twins, one asked for its symbolic observation after every step, through 250 steps into the night (where render()
  would draw noise from the RNG): every byte of every env's state, the RNG included, and obs / reward / done stay equal."""
  seeds = [7, 8, 9, 10]
  a, b = _batched(4, seeds=seeds), _batched(4, seeds=seeds)
  a.reset()
  b.reset()
  acts = np.random.RandomState(1234 + 7).choice([0, 0, 0, 6, 1, 2, 3, 4, 5], size=(250, 4)).astype(np.int32)
  night = False
  for t in range(250):
    a.step(_dev(acts[t], a), info=False)
    b.step(_dev(acts[t], b), info=False)
    _, stats = a.symbolic()
    night = night or bool((stats[:, -1] < 0.5).any())
  assert night
  assert torch.equal(a.obs, b.obs) and torch.equal(a.reward, b.reward) and torch.equal(a.done, b.done)
  for i in range(4):
    assert_same(a.snapshot(i), b.snapshot(i), f'env {i}')
  for name in ('mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census'):
    assert torch.equal(a.state[name], b.state[name]), name


def test_mask_out_and_render_off():
  seeds = [31, 32, 33, 34, 35]
  env, blind = _batched(5, seeds=seeds), _batched(5, seeds=seeds, render=False, semantic=True)
  env.reset()
  blind.reset()
  acts = np.random.RandomState(4).randint(0, 17, size=(20, 5)).astype(np.int32)
  for t in range(20):
    env.step(_dev(acts[t], env), info=False)
    blind.step(_dev(acts[t], blind), info=False)
  local, stats = env.symbolic()
  bl, bs = blind.symbolic()
  assert torch.equal(local, bl) and torch.equal(stats.view(torch.int32), bs.view(torch.int32))
  assert (local[:, 0] == 13).sum() == 5 and not bool(blind.obs.any())
  # masked rows keep what they held
  ls, ss = env.symbolic_shape
  L = torch.full((5,) + ls, 0xFF, dtype=torch.uint8, device=env.device)
  S = torch.full((5,) + ss, -7.0, dtype=torch.float32, device=env.device)
  mask = np.array([1, 0, 1, 0, 1], np.uint8)
  got = env.symbolic(mask=mask, out=(L, S))
  assert got[0] is L and got[1] is S
  keep = torch.from_numpy(mask.astype(bool)).to(env.device)
  assert torch.equal(L[keep], local[keep]) and torch.equal(S[keep], stats[keep])
  assert bool((L[~keep] == 0xFF).all()) and bool((S[~keep] == -7.0).all())
  # out must be exactly right
  good_l, good_s = torch.zeros_like(local), torch.zeros_like(stats)
  wide = torch.zeros((5, 2, ls[1], 2 * ls[2]), dtype=torch.uint8, device=env.device)
  for bad in ((good_l.to(torch.int8), good_s), (good_l, good_s.to(torch.float64)), (good_l[:4], good_s), (good_l, good_s[:, :-1]),
              (wide[..., ::2], good_s), (good_l.cpu(), good_s)):
    with pytest.raises(ValueError):
      env.symbolic(out=bad)
  with pytest.raises(ValueError):
    env.symbolic(mask=np.ones(4, np.uint8))


@pytest.mark.parametrize('n', [5, 257])
def test_batch_tails(n):
  """Batches that do not fill their last workgroup of four envs; seeds cycle over three values, so three oracles serve all rows."""
  from oracle.crafter_oracle import OracleEnv
  seeds = [41 + i % 3 for i in range(n)]
  env = _batched(n, seeds=seeds)
  orcs = [OracleEnv(seed=41 + k) for k in range(3)]
  for o in orcs:
    o.reset()
  env.reset()
  acts = np.random.RandomState(6).randint(0, 17, size=(10, 3)).astype(np.int32)
  for t in range(-1, 10):
    if t >= 0:
      env.step(_dev(acts[t][np.arange(n) % 3], env), info=False)
      for k, o in enumerate(orcs):
        o.step(int(acts[t, k]))
    want = [sr.symbolic_of(o) for o in orcs]
    local, stats = env.symbolic()
    assert_rows(local, stats, np.stack([want[i % 3][0] for i in range(n)]), np.stack([want[i % 3][1] for i in range(n)]), f'step {t}')


def test_facade_and_after_rollout():
  from crafter_amd import Env
  from oracle.crafter_oracle import OracleEnv
  e, orc = Env(seed=51), OracleEnv(seed=51)
  e.reset()
  orc.reset()
  for a in (2, 2, 5, 6, 3):
    e.step(a)
    orc.step(a)
    local, stats = e.symbolic()
    assert isinstance(local, np.ndarray) and isinstance(stats, np.ndarray)
    want = sr.symbolic_of(orc)
    assert_rows(local, stats, want[0], want[1], f'facade after action {a}')
  names = e._batch.symbolic_names
  assert names['classes'] == sr.names(e._batch.rules)[0] and names['stats'] == sr.names(e._batch.rules)[1]
  assert names['classes'][13] == 'player' and names['stats'][:4] == ['health', 'food', 'drink', 'energy']
  # after a rollout: the state behind its last step
  seeds = [52, 53, 54]
  env = _batched(3, seeds=seeds)
  orcs = [OracleEnv(seed=s) for s in seeds]
  for o in orcs:
    o.reset()
  env.reset()
  acts = np.random.RandomState(8).randint(0, 17, size=(16, 3)).astype(np.int32)
  env.rollout(_dev(acts, env))
  for t in range(16):
    for i, o in enumerate(orcs):
      assert not o.step(int(acts[t, i]))[2]
  want = [sr.symbolic_of(o) for o in orcs]
  local, stats = env.symbolic()
  assert_rows(local, stats, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), 'after rollout')
