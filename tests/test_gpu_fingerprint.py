"""BatchedEnv.fingerprint() / fingerprint_parts() / crafter_fingerprint on the device: against the numpy mirror of snapshot(i)
(crafter_amd.fingerprint_host), mask / out and the batch tail, what enters the hash and what does not (state rows edited by
hand), the step paths and the copies, the holes of the large-world instance, and the worked example: transposition pruning."""
import numpy as np
import pytest
import torch

import crafter_amd
from crafter_amd import abi, state

pytestmark = pytest.mark.gpu
P = abi.FP_PARTS


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def _u64(t):
  return t.cpu().numpy().view(np.uint64)


def _lanes(env):
  return env.records()['seed_lane']


def _mirror(env, parts=abi.FP_ALL):
  """-> (keys uint64 [N], part hashes uint64 [N, 7]) from snapshot(i), on the CPU."""
  lanes = _lanes(env)
  rows = [state.fingerprint_host(env.snapshot(i), lanes[i], parts) for i in range(env.num_envs)]
  return np.array([k for k, _ in rows], np.uint64), np.array([h for _, h in rows], np.uint64)


def _assert_parts(got, want, what):
  bad = np.argwhere(got != want)
  assert not len(bad), f'{what}: part hashes differ at (env, part) {bad[:6].tolist()}'


# ------------------------------------------------------------------ 1. the mirror
def test_equals_the_mirror_of_snapshot():
  """Six envs of the default geometry, episodes of 16 steps, 40 random steps: at every 8th step fingerprint_parts() and the keys
  equal the mirror of snapshot(i), for all rows."""
  env = _batched(6, seeds=[61, 62, 63, 64, 65, 66], length=16, auto_reset=True)
  assert env.step_instance == 'crafter_step_kernel<1, 1, 1>' and env.slot_map_derived
  env.reset()
  acts = np.random.RandomState(6).randint(0, 17, size=(40, 6)).astype(np.int32)
  for t in range(41):
    if t % 8 == 0:
      parts = env.fingerprint_parts()
      assert parts.dtype == torch.int64 and tuple(parts.shape) == (6, P)
      wkey, wparts = _mirror(env)
      _assert_parts(_u64(parts), wparts, f'step {t}')
      assert _u64(env.fingerprint(abi.FP_ALL)).tolist() == wkey.tolist(), t
      assert _u64(env.fingerprint()).tolist() == [state.fingerprint_combine(row, abi.FP_DYNAMICS) for row in wparts], t
    if t < 40:
      env.step(_dev(acts[t], env), info=False)
  assert int(env.records()['episode'].min()) >= 3
  env.check_errors()


# ------------------------------------------------------------------ 2. mask, tail, arguments
def test_mask_tail_out_and_arguments():
  """Five envs (four to a workgroup), a mask naming rows {0, 3}, out= pre-filled with a sentinel: the other rows stay untouched.
  Bad `parts` values raise through _check; bad out / mask tensors raise ValueError before anything is enqueued."""
  from crafter_amd import CrafterDeviceError
  env = _batched(5, seeds=[31, 32, 33, 34, 35])
  env.reset()
  acts = np.random.RandomState(4).randint(0, 17, size=(10, 5)).astype(np.int32)
  for t in range(10):
    env.step(_dev(acts[t], env), info=False)
  full_key, full_parts = env.fingerprint(abi.FP_ALL), env.fingerprint_parts()
  wkey, wparts = _mirror(env)
  assert _u64(full_key).tolist() == wkey.tolist()
  _assert_parts(_u64(full_parts), wparts, 'tail')
  sentinel = 0x5E5E5E5E5E5E5E5E
  key = torch.full((5,), sentinel, dtype=torch.int64, device=env.device)
  parts = torch.full((5, P), sentinel, dtype=torch.int64, device=env.device)
  mask = np.array([1, 0, 0, 1, 0], np.uint8)
  assert env.fingerprint(abi.FP_ALL, mask=mask, out=key) is key and env.fingerprint_parts(mask=mask, out=parts) is parts
  keep = torch.from_numpy(mask.astype(bool)).to(env.device)
  assert torch.equal(key[keep], full_key[keep]) and bool((key[~keep] == sentinel).all())
  assert torch.equal(parts[keep], full_parts[keep]) and bool((parts[~keep] == sentinel).all())
  for bad in (0, 128, abi.FP_ALL | 256):
    with pytest.raises(CrafterDeviceError, match='crafter_fingerprint'):
      env.fingerprint(bad)
  assert torch.equal(env.fingerprint(abi.FP_ALL), full_key)   # (a refused call leaves the handle usable)
  good = torch.zeros_like(full_key)
  for bad in (good.to(torch.int32), good[:4], torch.zeros(10, dtype=torch.int64, device=env.device)[::2], good.cpu(), good.cpu().numpy(), full_parts):
    with pytest.raises(ValueError):
      env.fingerprint(out=bad)
  for bad in (full_key, torch.zeros((5, P), dtype=torch.uint8, device=env.device), torch.zeros((5, P + 1), dtype=torch.int64, device=env.device)[:, :P]):
    with pytest.raises(ValueError):
      env.fingerprint_parts(out=bad)
  with pytest.raises(ValueError):
    env.fingerprint(mask=np.ones(4, np.uint8))
  # the facade: an unsigned Python int, the mirror's
  e = crafter_amd.Env(seed=51)
  e.reset()
  e.step(2)
  snap, lane = e._batch.snapshot(0), _lanes(e._batch)[0]
  for which in (abi.FP_DYNAMICS, abi.FP_VISIBLE, abi.FP_ALL):
    k = e.fingerprint(which)
    assert isinstance(k, int) and 0 <= k < 1 << 64 and k == state.fingerprint_host(snap, lane, which)[0]
  assert e.fingerprint() == e.fingerprint(abi.FP_DYNAMICS)


# ------------------------------------------------------------------ 3. what counts and what does not
def test_what_counts_and_what_does_not():
  """Row 1 is made a copy of row 0 (copy_envs), one thing is written into its state tensors by hand, and the two rows' part
  hashes are compared.  No step follows an edit, so the row may be left inconsistent."""
  env = _batched(2, seeds=[71, 71], auto_reset=False)
  assert env.slot_map_derived
  env.reset()
  for a in (2, 2, 4, 5, 1, 1, 5, 3):
    env.step(_dev([a, a], env), info=False)
  st, rec, off = env.state, env._rec_i32, env._off
  base = env.records()[0]
  nobj, nseen = int(base['nobj']), int(base['nchunks_seen'])
  objs = state.objs_view(st['objs'][0:1].cpu().numpy())[0]
  live = [s for s in range(2, nobj) if objs[s]['type'] != abi.T_NONE]
  assert len(live) >= 2 and nobj + 2 < env.cfg.max_objects and nseen >= 2
  s1, s2 = live[0], live[-1]
  assert objs[s1].tobytes()[:12] != objs[s2].tobytes()[:12]
  wood = list(env.item_names).index('wood')
  assert wood != env.tables.rules.item_health
  obj_i32 = st['objs'].view(torch.int32)   # [N, C, 4]: type | health | fx | fy, x | y, aux, pad
  nch = st['chunk_order'].shape[1]

  def swap(t, a, b):
    tmp = t[a].clone()
    t[a] = t[b]
    t[b] = tmp

  def changed(edit):
    env.copy_envs([0], [1])
    edit()
    parts = _u64(env.fingerprint_parts())
    key = _u64(env.fingerprint(abi.FP_ALL))
    differs = (parts[0] != parts[1]).tolist()
    assert (key[0] != key[1]) == any(differs)
    return [abi.FP_NAMES[p] for p in range(P) if differs[p]]

  def bump(t, index, by=1):
    t[index] = t[index] + by

  counts = {
      'one mat byte': (lambda: bump(st['mat'], (1, 1000), 1), 'map'),
      'the last mat byte': (lambda: bump(st['mat'], (1, st['mat'].shape[1] - 1), 1), 'map'),
      "one object's aux": (lambda: bump(obj_i32, (1, s1, 2), 5), 'objects'),
      'two live slots exchanged': (lambda: swap(st['objs'][1], s1, s2), 'objects'),
      'one inventory count': (lambda: bump(rec, (1, off['inv'] + wood), 1), 'player'),
      'one achievement count': (lambda: bump(rec, (1, off['ach'] + 3), 1), 'player'),
      'hunger': (lambda: bump(rec, (1, off['hunger2']), 1), 'player'),
      'one mt word': (lambda: bump(st['mt'], (1, 311), 1), 'rng'),
      'the last mt word': (lambda: bump(st['mt'], (1, abi.MT_N - 1), 1), 'rng'),
      'mt_pos': (lambda: bump(rec, (1, off['mt_pos']), 1), 'rng'),
      'step': (lambda: bump(rec, (1, off['step']), 1), 'clock'),
      'two chunk-order entries exchanged': (lambda: swap(st['chunk_order'][1], 0, nseen - 1), 'chunks'),
      'seed_lane': (lambda: bump(rec, (1, off['seed_lane'] + 1), 1), 'ident'),
      'episode': (lambda: bump(rec, (1, off['episode']), 1), 'ident'),
  }
  for what, (edit, part) in counts.items():
    assert changed(edit) == [part], what
  # the player's health is an inventory count AND what its object record shows (state.live_objects)
  assert changed(lambda: bump(rec, (1, off['inv'] + env.tables.rules.item_health), -1)) == ['objects', 'player']

  def garbage_tail():
    st['objs'][1, nobj:nobj + 2] = 0xAB

  def derived_maps():
    st['objmap'][1] = 7
    st['census'][1] = -3
    st['chunk_seen'][1] = 1 - st['chunk_seen'][1]
    st['chunk_order'][1, nseen:] = 9

  def bookkeeping():
    for name in ('status', 'dhealth', 'new_unlocked', 'dead', 'done', 'needs_reset', 'ep_dhealth', 'ep_unlock_steps', 'env_last_health', 'unlocked'):
      bump(rec, (1, off[name]), 1)

  nothing = {
      'garbage in records >= nobj': garbage_tail,
      'Obj.pad': lambda: bump(obj_i32, (1, s1, 3), 99),
      "the player's Obj.health byte": lambda: bump(st['objs'], (1, 1, 1), 3),
      'objmap, census, chunk_seen, chunk_order behind nchunks_seen': derived_maps,
      'status, dhealth, new_unlocked and the other bookkeeping fields': bookkeeping,
  }
  for what, edit in nothing.items():
    assert changed(edit) == [], what
  assert nch > nseen   # (the chunk-order tail existed)


# ------------------------------------------------------------------ 4. the step paths and the copies
def test_paths_and_copies_agree():
  """The same tape through step x T, rollout(T) and rollout_envs: all seven parts equal (the raw slot tables differ in their free
  tails).  copy_envs and a save_state / load_state round trip keep all seven."""
  seeds, T = [81, 82, 83, 84], 40
  acts = np.random.RandomState(8).randint(0, 17, size=(T, 4)).astype(np.int32)
  envs = [_batched(4, seeds=seeds, length=16, auto_reset=True) for _ in range(3)]
  for e in envs:
    e.reset()
  a, b, c = envs
  for t in range(T):
    a.step(_dev(acts[t], a), info=False)
  b.rollout(_dev(acts, b), obs=False)
  c.rollout_envs([2, 0, 3, 1], _dev(acts[:, [2, 0, 3, 1]], c), obs=False)
  want = _u64(a.fingerprint_parts())
  _assert_parts(want, _mirror(a)[1], 'step')
  _assert_parts(_u64(b.fingerprint_parts()), want, 'rollout')
  _assert_parts(_u64(c.fingerprint_parts()), want, 'rollout_envs')
  assert int(a.records()['episode'].min()) >= 3
  a.copy_envs([0, 1], [3, 2])
  got = _u64(a.fingerprint_parts())
  _assert_parts(got[[3, 2]], want[[0, 1]], 'copy_envs')
  _assert_parts(got[[0, 1]], want[[0, 1]], 'copy_envs sources')
  store = b.save_state([1, 2])
  for t in range(5):
    b.step(_dev(acts[t], b), info=False)
  moved = _u64(b.fingerprint_parts())
  assert (moved[[1, 2]] != want[[1, 2]]).any(axis=1).all()
  b.load_state(store)
  _assert_parts(_u64(b.fingerprint_parts())[[1, 2]], want[[1, 2]], 'load_state')
  b.load_state(store, idx=[0], rows=[1])   # ... and into another row
  assert _u64(b.fingerprint_parts())[0].tolist() == want[2].tolist()
  for e in envs:
    e.check_errors()


# ------------------------------------------------------------------ 5. the large-world instance's holes
def test_large_world_holes_do_not_count():
  """area (256, 256), the smallest geometry of the suite whose slot map is state: two rows in the same state; in row 0 a live
  non-player slot's type is cleared by hand (a hole, as that instance's despawn leaves it), in row 1 the same record is removed
  and the table compacted by hand.  Same keys, and the mirror's."""
  env = _batched(2, area=(256, 256), seeds=[3, 3], auto_reset=False)
  assert not env.slot_map_derived
  env.reset()
  for a in (1, 5, 2):
    env.step(_dev([a, a], env), info=False)
  before = _u64(env.fingerprint_parts())
  assert before[0].tolist()[:6] == before[1].tolist()[:6]
  nobj = int(env.records()['nobj'][0])
  objs = state.objs_view(env.state['objs'][0:1].cpu().numpy())[0]
  live = [s for s in range(2, nobj - 1) if objs[s]['type'] != abi.T_NONE]
  s = live[len(live) // 2]
  assert nobj > 256 and s + 1 < nobj
  env.state['objs'][0, s, 0] = abi.T_NONE
  env.state['objs'][1, s:nobj - 1] = env.state['objs'][1, s + 1:nobj].clone()
  env._rec_i32[1, env._off['nobj']] = nobj - 1
  parts = _u64(env.fingerprint_parts())
  assert parts[0].tolist() == parts[1].tolist()
  assert [p for p in range(P) if parts[0, p] != before[0, p]] == [1]
  key = _u64(env.fingerprint(abi.FP_ALL))
  assert key[0] == key[1]
  wkey, wparts = _mirror(env)
  _assert_parts(parts, wparts, 'mirror')
  assert key.tolist() == wkey.tolist()
  assert env.snapshot(0)['objects'] == env.snapshot(1)['objects']


# ------------------------------------------------------------------ 6. the worked example: transposition pruning
def test_transposition_pruning():
  """A root row (seed 7 after reset and three moves: on the CPU harness its mirror shows eleven illegal non-move actions and six
  legal ones with six distinct keys) is copied into 17 scratch rows, each stepped with one action by step_envs.  Every non-move
  action with legal_actions() == 0 lands on the noop row's DYNAMICS key -- the header's promise for illegal actions -- so a
  search expands that child once; the legal actions give distinct keys."""
  env = _batched(18, seeds=[7] * 18, auto_reset=False)
  names = list(env.action_names)
  assert len(names) == 17 and names[0] == 'noop'
  env.reset()
  for a in (1, 1, 3):
    env.step(_dev([a] * 18, env), info=False)
  rows = list(range(1, 18))
  env.copy_envs([0] * 17, rows)
  legal = env.legal_actions().cpu().numpy()
  assert (legal[1:] == legal[0]).all()
  legal = legal[0]
  root = _u64(env.fingerprint())
  assert len(set(root.tolist())) == 1
  env.step_envs(rows, np.arange(17, dtype=np.int32), info=False)
  key = _u64(env.fingerprint())
  assert key[0] == root[0]   # the root row was not stepped
  child = {names[a]: int(key[1 + a]) for a in range(17)}
  illegal = [n for a, n in enumerate(names) if not legal[a] and not n.startswith('move_')]
  legal_names = [n for a, n in enumerate(names) if legal[a]]
  assert len(illegal) >= 5 and len(legal_names) >= 3
  for n in illegal:
    assert child[n] == child['noop'], n
  assert len({child[n] for n in legal_names}) >= 2 and child['noop'] != int(root[0])
  # what the table saves: 17 children, far fewer distinct ones; and the mirror sees the same partition
  distinct = len(set(child.values()))
  assert distinct <= 17 - len(illegal)
  lanes = _lanes(env)
  mirror = [state.fingerprint_host(env.snapshot(i), lanes[i], abi.FP_DYNAMICS)[0] for i in range(1, 18)]
  assert mirror == [child[n] for n in names]
  env.check_errors()
