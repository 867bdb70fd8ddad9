"""BatchedEnv.edit / crafter_edit_envs on the device: the CPU parity cases against the oracle that executes the reference's
statements (tests/edits_ref.py; tied to the real reference by tests/test_edits_golden.py) through a night, the LDS-resident and
the global-memory layouts, device tapes and device index lists, auto-reset with the world pool running next to a twin batch, the
read-only queries right behind an edit, edits mixed with every other call, Env.edit, and the README's counterfactual."""
import numpy as np
import pytest
import torch

from crafter_amd import abi, edits as E
from tests import edits_cases as ec
from tests import worlds_cases as wc
from tests.edits_ref import EditedOracle
from tests.parity import assert_same

pytestmark = pytest.mark.gpu

STATE = ('mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census')


def _batched(*a, **k):
  from crafter_amd import BatchedEnv
  return BatchedEnv(*a, **k)


def _dev(a, env, dtype=np.int32):
  return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(env.device)


def _rows(env, names=STATE):
  out = {k: env.state[k].cpu().numpy() for k in names}
  if not env.slot_map_derived:
    out['objmap'] = env.state['objmap'].cpu().numpy()
  return out


def _outputs(env):
  return [t.cpu().numpy().copy() for t in (env.obs, env.reward, env.done)]


def _oracle(world, seed, **kw):
  o = EditedOracle(seed=seed, **kw)
  o.world = world
  return o, o.reset()


def test_parity_three_edited_envs_through_a_night():
  """The CPU parity case on the device: state, frame, reward and done at every step, the state right behind every edit too."""
  runs = [ec.oracle_run(k, ec.SEEDS[k]) for k in range(3)]
  env = _batched(3, seeds=list(ec.SEEDS), auto_reset=False)
  obs = env.reset(worlds=ec.bank_of(env, range(3))).cpu().numpy()
  for i, r in enumerate(runs):
    assert np.array_equal(obs[i], r.frames[0]), f'env {i}: first frame'
  tapes = np.stack([ec.tape(i) for i in range(3)], 1)
  for t in range(ec.T):
    named = [i for i in range(3) if t in ec.SCHEDULES[i]]
    if named:
      before = _outputs(env)
      env.edit(named, [ec.SCHEDULES[i][t] for i in named])
      for i in named:
        assert_same(env.snapshot(i), runs[i].edited[t], f'env {i} edited before step {t + 1}')
      assert all(np.array_equal(a, b) for a, b in zip(before, _outputs(env))), 'an edit redraws nothing'
    obs, rew, done, _ = env.step(_dev(tapes[t], env))
    obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
    for i, r in enumerate(runs):
      assert np.array_equal(obs[i], r.frames[t + 1]), f'env {i} step {t + 1}: pixels'
      assert rew[i] == np.float32(r.rewards[t]) and bool(done[i]) == r.dones[t], f'env {i} step {t + 1}: reward / done'
      assert_same(env.snapshot(i), r.snapshots[t + 1], f'env {i} step {t + 1}')
  env.check_errors()


@pytest.mark.parametrize('area,view,size', [((42, 30), (7, 9), (84, 72)), ((132, 132), (9, 9), (64, 64)), ((256, 256), (9, 9), (64, 64))],
                         ids=['42x30-lds', '132x132-lds-beyond-64K', '256x256-global'])
def test_other_geometries(area, view, size):
  """(132 x 132: the edit kernel's LDS exceeds the 64 KB a launch gets without asking; crafter_create allowed it that much.)"""
  from crafter_amd import WorldBank
  env = _batched(2, area=area, view=view, size=size, seeds=[81, 82], auto_reset=False)
  assert env.slot_map_derived == (area[0] < 256)
  world = wc.small_world(area)
  obs = env.reset(worlds=WorldBank(env, world['mat'][None], [world['objects']], [world['inventory']])).cpu().numpy()
  orcs = []
  for i in range(2):
    o, first = _oracle(world, 81 + i, area=area, view=view, size=size)
    assert np.array_equal(obs[i], first)
    orcs.append(o)
  tapes = ec.geometry_edits(area)
  tape = np.random.RandomState(9).randint(0, 17, size=34)
  for t in range(34):
    if t in (0, 4):
      env.edit([1, 0], tapes[t // 4])
      for i, o in enumerate(orcs):
        o.edit(E.encode(env, tapes[t // 4], 1)[0])
        assert_same(env.snapshot(i), o.snapshot(), f'env {i} edited before step {t + 1}')
    obs = env.step(_dev(np.full(2, tape[t]), env))[0].cpu().numpy()
    for i, o in enumerate(orcs):
      assert np.array_equal(obs[i], o.step(int(tape[t]))[0]), (t, i)
  for i, o in enumerate(orcs):
    assert_same(env.snapshot(i), o.snapshot(), f'env {i} step 34')
  env.check_errors()


def test_device_tape_with_bad_ops():
  """A tape built on the device is not read back: its bad ops are met by the kernel -- check_errors() names ST_BAD_EDIT -- and
  the rest of the tape is applied."""
  from crafter_amd import CrafterDeviceError
  names = ['add_occupied', 'unknown_kind', 'clock_at_length', 'item_value_high']
  cases = ec.refusals()
  env = _batched(5, seeds=[100 + j for j in range(5)], auto_reset=False)
  env.reset(worlds=ec.bank_of(env, [1]))
  before = [env.snapshot(j) for j in range(5)]
  tape = torch.zeros((5, 3, 8), dtype=torch.int32, device=env.device)
  tape[:4] = _dev(np.stack([cases[n] for n in names]), env)
  tape[4, 1] = _dev(ec.rows([E.set_item('wood', 2)])[0], env)   # a clean tape between NOPs
  env.edit(torch.arange(5, device=env.device), tape)
  with pytest.raises(CrafterDeviceError, match='ST_BAD_EDIT'):
    env.check_errors()
  status = env.records()['status']
  assert list(status) == [abi.STATUS_BAD_EDIT] * 4 + [0]
  for j, name in enumerate(names):
    clean, flagged = E.clean_edits(env, before[j], cases[name])
    assert flagged
    o, _ = _oracle(ec.garden(), 100 + j)
    o.edit(clean)
    assert_same(env.snapshot(j), o.snapshot(), name)
    assert env.snapshot(j)['mat'][5, 5] == ec.MAT['sand'] and env.snapshot(j)['inventory'][ec.ITEMS.index('wood')] == 3
  assert env.snapshot(4)['inventory'][ec.ITEMS.index('wood')] == 2
  with pytest.raises(ValueError):
    env.edit([0], torch.zeros((1, 3, 7), dtype=torch.int32, device=env.device))
  with pytest.raises(ValueError):
    env.edit([0, 1], torch.zeros((1, 3, 8), dtype=torch.int32, device=env.device))
  with pytest.raises(ValueError):
    env.edit([0], [E.set_cell(64, 0, 'stone')])


def test_bad_index_list_on_the_device_refuses_the_whole_call():
  from crafter_amd import CrafterDeviceError
  env = _batched(4, seeds=[1, 2, 3, 4], auto_reset=False)
  env.reset()
  env.step(_dev([1, 2, 3, 4], env))
  before, outs = _rows(env), _outputs(env)
  for idx, flagged in (([0, 2, 0], [0, 2]), ([3, 4], [3]), ([-1], [0])):
    env.edit(_dev(idx, env), [E.set_item('wood', 5), E.set_clock(300)])
    with pytest.raises(CrafterDeviceError, match='ST_BAD_COPY'):
      env.check_errors()
    status = env.records()['status']
    assert [i for i in range(4) if status[i]] == flagged and all(status[i] == abi.ST_BAD_COPY for i in flagged)
    env._rec_i32[:, env._off['status']] = 0
    after = _rows(env)
    for k in before:
      assert np.array_equal(after[k], before[k]), (idx, k)
    assert all(np.array_equal(a, b) for a, b in zip(outs, _outputs(env)))
  for idx in ([0, 0], [4], [-1], [0.5]):
    with pytest.raises(ValueError):
      env.edit(idx, [E.NOP])
  env.edit([], [E.NOP])   # enqueues nothing
  env.check_errors()


def _free_neighbour(snap):
  x, y = snap['objects'][0][1:3]
  for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
    if 0 <= x + dx < 64 and 0 <= y + dy < 64 and not snap['occupied'][x + dx, y + dy]:
      return x + dx, y + dy
  raise AssertionError('the player is walled in by objects')


def test_auto_reset_pool_and_an_unedited_twin():
  """8 envs under auto-reset with the pool on, two of them edited: the other six stay bit-identical to a twin batch that never
  made the call, over 40 steps; an edited env that dies comes back with the generated next episode of its seed."""
  seeds = [200 + i for i in range(8)]
  a, b = _batched(8, seeds=seeds), _batched(8, seeds=seeds)
  a.reset()
  b.reset()
  rs = np.random.RandomState(21)
  acts = rs.randint(0, 17, size=(40, 8))
  acts[3, 2] = ec.ACT['noop']
  others = [0, 1, 3, 4, 6, 7]
  for t in range(40):
    if t == 3:   # env 2: one health point and a zombie with no cooldown beside the player -- dead at the next step; env 5: a gift
      zx, zy = _free_neighbour(a.snapshot(2))
      a.edit([5, 2], [[E.set_item('wood_pickaxe', 1), E.set_item('stone', 5), E.set_clock(170)],
                      [E.set_item('health', 1), E.add('zombie', zx, zy), E.set_player(sleeping=0)]])
    if t == 20:
      px, py = a.snapshot(5)['objects'][0][1:3]
      a.edit([5], [E.set_cell(px, py, 'path'), E.set_item('health', 9)])
    oa, ra, da, _ = a.step(_dev(acts[t], a))
    ob, rb, db, _ = b.step(_dev(acts[t], b))
    if t == 3:
      assert int(da[2]) == 1 and int(db[2]) == 0, 'the edited env did not die'
      c = _batched(8, seeds=seeds)
      first = c.reset(episodes=2).cpu().numpy()
      assert np.array_equal(oa[2].cpu().numpy(), first[2])
      assert_same(a.snapshot(2), c.snapshot(2), 'the episode after the edited one')
      del c
    ra_, rb_ = _rows(a), _rows(b)
    for k in ra_:
      assert np.array_equal(ra_[k][others], rb_[k][others]), (t, k)
    for x, y in ((oa, ob), (ra, rb), (da, db)):
      assert torch.equal(x[others], y[others]), t
  assert a.pool_status()['state'] == 'running'
  a.check_errors()
  b.check_errors()


def test_queries_see_an_edit_at_once():
  """symbolic(), legal_actions(), navigate() and fingerprint_parts() right behind an edit, with no step in between; a SET_CELL
  changes only the map part of the fingerprint, a SET_ITEM only the player part, a SET_CLOCK only the clock part."""
  env = _batched(2, seeds=[41, 42], auto_reset=False)
  env.reset(worlds=ec.bank_of(env, [1]))
  sleep = ec.ACT['sleep']
  look = lambda: (env.symbolic()[0].cpu().numpy().copy(), env.symbolic()[1].cpu().numpy().copy(), env.legal_actions().cpu().numpy().copy(),
                  env.navigate(['stone'])[0].cpu().numpy().copy(), env.fingerprint_parts().cpu().numpy().copy())
  local0, stats0, legal0, dist0, fp0 = look()
  assert dist0[0, 0] == -1 and not legal0[0, sleep]
  parts = lambda fp, base: [abi.FP_NAMES[p] for p in range(abi.FP_PARTS) if fp[0, p] != base[0, p]]
  env.edit([0], [E.set_cell(33, 32, 'stone')])
  local1, stats1, legal1, dist1, fp1 = look()
  diff = np.argwhere(local1[0] != local0[0])
  assert diff.tolist() == [[0, 5, 3]] and local1[0, 0, 5, 3] == ec.MAT['stone']   # plane 0, one cell right of the player's (4, 3)
  assert dist1[0, 0] == 1 and parts(fp1, fp0) == ['map']
  env.edit([0], [E.set_item('energy', 3)])
  local2, stats2, legal2, dist2, fp2 = look()
  assert legal2[0, sleep] and not legal1[0, sleep] and parts(fp2, fp1) == ['player']
  assert (stats2[0] != stats1[0]).sum() == 1
  env.edit([0], [E.set_clock(200)])
  local3, stats3, legal3, dist3, fp3 = look()
  assert parts(fp3, fp2) == ['clock'] and (stats3[0] != stats2[0]).sum() == 1   # (the daylight entry)
  env.edit([0], [E.add('zombie', 31, 32), E.move(32, 32, 32, 31)])
  local4, _, _, _, fp4 = look()
  assert set(parts(fp4, fp3)) == {'objects'} and not np.array_equal(local4[0], local3[0])
  for x, y in zip(look(), (local0, stats0, legal0, dist0, fp0)):   # env 1 never changed
    assert np.array_equal(x[1], y[1])
  env.check_errors()


def test_edits_mix_with_every_other_call():
  """edit between step_envs, rollout, copy_envs and a save_state / load_state round trip: row 0 and its copy follow the oracle
  that made the same edits; the edit behind the save is undone by the load."""
  seeds = [51, 52, 53, 54]
  env = _batched(4, seeds=seeds, auto_reset=False)
  env.reset(worlds=ec.bank_of(env, [1]))
  o, _ = _oracle(ec.garden(), 51)
  A = [E.set_object(32, 33, aux=400), E.add('cow', 33, 32), E.set_item('sapling', 3)]
  B = [E.set_cell(31, 32, 'sand'), E.set_clock(155), E.remove(33, 32)]
  C = [E.set_item('health', 2), E.set_cell(32, 31, 'lava'), E.set_clock(9)]
  env.edit([0], A)
  o.edit(ec.rows(A))
  env.step_envs([0], _dev([ec.ACT['do']], env))
  o.step(ec.ACT['do'])
  roll = np.random.RandomState(6).randint(0, 5, size=(3, 4))
  env.rollout(_dev(roll, env), obs=False)
  for a in roll[:, 0]:
    o.step(int(a))
  px, py = o.ox[1], o.oy[1]
  assert (px, py) == env.snapshot(0)['objects'][0][1:3]
  B = B[:2] + ([B[2]] if int(o.objmap[33, 32]) > 1 else [])   # (the cow may have walked)
  env.edit([0], B)
  o.edit(ec.rows(B))
  assert_same(env.snapshot(0), o.snapshot(), 'row 0 behind the second edit')
  env.copy_envs([0], [2])
  store = env.save_state([0])
  env.edit([0], C)
  assert env.snapshot(0)['step'] == 9 and env.snapshot(0)['inventory'][0] == 2
  env.step_envs([0], _dev([ec.ACT['noop']], env))
  env.load_state(store, [0])
  assert_same(env.snapshot(0), o.snapshot(), 'row 0 loaded back')
  for a in (ec.ACT['move_up'], ec.ACT['place_plant'], ec.ACT['noop']):
    obs = env.step_envs([2, 0], _dev([a, a], env))[0].cpu().numpy()
    want = o.step(a)[0]
    assert np.array_equal(obs[0], want) and np.array_equal(obs[2], want)
  assert_same(env.snapshot(0), o.snapshot(), 'row 0')
  assert_same(env.snapshot(2), o.snapshot(), 'its copy')
  env.check_errors()


def test_env_edit():
  import crafter_amd
  env = crafter_amd.Env(seed=7)
  world = ec.garden()
  first = env.reset(world=world)
  o, want = _oracle(world, 7)
  assert np.array_equal(first, want)
  tape = [E.set_object(32, 33, aux=400), E.set_clock(160), E.set_item('wood', 1)]
  env.edit(tape)
  o.edit(ec.rows(tape))
  shown = env.render()   # (once: a night frame draws its noise from the env's stream, here as in the reference)
  assert env._step == 160 and np.array_equal(shown, o.render()) and not np.array_equal(shown, first)
  obs, reward, done, info = env.step(ec.ACT['do'])
  wobs, wreward, wdone, winfo = o.step(ec.ACT['do'])
  assert np.array_equal(obs, wobs) and reward == wreward and done == wdone and env._step == 161
  assert info['achievements']['eat_plant'] == 1 and info['inventory'] == winfo['inventory']
  with pytest.raises(crafter_amd.CrafterDeviceError, match='ST_BAD_EDIT'):
    env.edit([E.remove(1, 1), E.set_item('wood', 5)])
  assert env._player.inventory['wood'] == 5
  with pytest.raises(ValueError):
    env.edit([E.set_item('wood', 10)])
  # a refused op and a clock op in one tape: the clock op is applied, and the facade's counter follows it
  short = crafter_amd.Env(seed=8, length=50)
  short.reset()
  with pytest.raises(crafter_amd.CrafterDeviceError, match='ST_BAD_EDIT'):
    short.edit([E.remove(*_free_neighbour(short._batch.snapshot(0))), E.set_clock(48)])
  assert short._step == 48 and short._batch.snapshot(0)['step'] == 48
  short._batch._rec_i32[:, short._batch._off['status']] = 0
  assert not short.step(ec.ACT['noop'])[2] and short._step == 49 and not short._batch.records()[0]['done']
  assert short.step(ec.ACT['noop'])[2] and short._step == 50 and short._batch.records()[0]['done']   # done by length, where the device says so


def test_edit_on_a_batch_without_an_episode_length():
  """length=None: a clock op near the end of the daylight table makes the batch look at the counters again, and the table grows
  before the episode gets there; frames and state follow the oracle across the old table's end."""
  env = _batched(2, seeds=[151, 152], length=None, auto_reset=False)
  obs = env.reset().cpu().numpy()
  n0 = int(env.cfg.n_daylight)
  o = EditedOracle(seed=151, length=None)
  assert np.array_equal(obs[0], o.reset())
  with pytest.raises(ValueError):
    env.edit([0], [E.set_clock(n0)])
  tape = [E.set_clock(n0 - 4), E.set_item('wood', 2)]
  env.edit([0], tape)
  o.edit(E.encode(env, tape, 1)[0])
  for a in (1, 2, 5, 0, 3, 4, 0, 5):
    obs = env.step(_dev([a, 0], env))[0].cpu().numpy()
    assert np.array_equal(obs[0], o.step(a)[0]), a
    env.check_errors()
  assert int(env.cfg.n_daylight) > n0 and env.snapshot(0)['step'] == n0 + 4 and env.snapshot(1)['step'] == 8
  assert_same(env.snapshot(0), o.snapshot(), 'beyond the old table')


def test_counterfactual_zombie():
  """The worked example of the README: the same state with and without the zombie.  Row 0 stands beside a zombie; copy_envs
  makes two scratch rows of it, one loses the zombie by REMOVE, both are rolled out under one tape: the reward traces (a tenth
  of each step's health change) and the health at the end differ exactly as two oracles say."""
  env = _batched(4, seeds=[11, 77, 78, 79], auto_reset=False)
  env.reset(worlds=ec.bank_of(env, [0]))
  setup = [E.add('zombie', 33, 32), E.add('zombie', 31, 32, aux=2)]
  env.edit([0], setup)
  env.copy_envs([0, 0], [1, 2])
  env.edit([2], [E.remove(33, 32)])
  T = 12
  tape = np.full((T, 2), ec.ACT['noop'], np.int32)
  _, reward, done = env.rollout_envs([1, 2], _dev(tape, env), obs=False)
  reward = reward.cpu().numpy()
  health = ec.ITEMS.index('health')
  for row, extra in ((1, []), (2, [E.remove(33, 32)])):
    o, _ = _oracle(ec.quarry(), 11)
    o.edit(ec.rows(setup + extra))
    want = [o.step(ec.ACT['noop'])[1] for _ in range(T)]
    assert reward[:, row - 1].tolist() == [np.float32(r) for r in want], row
    assert_same(env.snapshot(row), o.snapshot(), f'row {row}')
  h1, h2 = env.snapshot(1)['inventory'][health], env.snapshot(2)['inventory'][health]
  assert h1 < h2 < 9, (h1, h2)   # two zombies hurt more than one; one still hurts
  assert env.snapshot(0)['step'] == 0 and env.snapshot(3)['step'] == 0
  env.check_errors()
