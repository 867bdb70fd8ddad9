"""Edits in place on the CPU: the body of crafter_edit_envs (csrc/env_edit.hpp) through WaveHost against the oracle that executes
the reference's statements (tests/edits_ref.py): parity through a night with the derived tables checked on the way, the device's
refusals, unnamed rows, a NOP tape, other geometries, the stand-alone sanitised build, encode()'s errors, the library's side."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import crafter_amd
from crafter_amd import abi, edits as E, state
from crafter_amd.worlds import WorldBank
from tests import edits_cases as ec
from tests import worlds_cases as wc
from tests.edits_ref import EditedOracle
from tests.hostsim import edits_build as eb
from tests.hostsim import worlds_build
from tests.hostsim.driver import HostSimEnv
from tests.parity import assert_same

ROOT = pathlib.Path(__file__).resolve().parent.parent
STATE_BUFFERS = ('mat', 'objmap', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'semantic', 'terminal')   # (tests/test_worlds_host.py's list)


def raw_state(hs):
  return {k: hs.buf[k].copy() for k in STATE_BUFFERS}


def census_of(snap, cfg):
  """The per-chunk census [nchunks][5] -- grass cells, path cells, zombies, skeletons, cows -- counted from a snapshot."""
  nx, ny = cfg.nchunk_x, cfg.nchunk_y
  out = np.zeros((nx * ny, 5), np.int32)
  for col, m in ((0, ec.MAT['grass']), (1, ec.MAT['path'])):
    xs, ys = np.nonzero(snap['mat'] == m)
    np.add.at(out[:, col], (xs // abi.CHUNK) * ny + ys // abi.CHUNK, 1)
  for o in snap['objects']:
    col = {ec.ZOMBIE: 2, ec.SKELETON: 3, ec.COW: 4}.get(o[0])
    if col is not None:
      out[(o[1] // abi.CHUNK) * ny + o[2] // abi.CHUNK, col] += 1
  return out


def check_row(hs, i, snap, what):
  """Row i of the harness against an oracle snapshot, the census included (no snapshot carries it: a wrong count would only
  show ten steps later, in what the balance pass draws)."""
  assert_same(hs.snapshot(i), snap, what)
  assert np.array_equal(hs.buf['census'][i].reshape(-1, 5), census_of(snap, hs.cfg)), f'{what}: census'


# ------------------------------------------------------------------ 1. parity, 2. its preconditions
def test_preconditions_of_the_parity_cases():
  """What the cases must show on the oracle ALONE, or a wrong census / aux / chunk order would pass unnoticed."""
  health = ec.ITEMS.index('health')
  ach = lambda r, t, name: r.snapshots[t]['achievements'][ec.ACHS.index(name)]
  r0, r1, r2 = (ec.oracle_run(k, ec.SEEDS[k]) for k in range(3))
  # the added zombie hit the player (cooldown 0: at once; then it cools down)
  assert r0.snapshots[1]['inventory'][health] == r0.edited[0]['inventory'][health] - 2, 'the added zombie did not hit'
  assert [o for o in r0.snapshots[1]['objects'] if o[0] == ec.ZOMBIE][0][6] == 5
  # a SET_CELL stone blocked a move that succeeds without it ...
  free = ec.oracle_run(0, ec.SEEDS[0], without=(0, 2), steps=3)
  assert free.snapshots[1]['objects'][0][1:3] == (32, 33) and r0.snapshots[1]['objects'][0][1:3] == (32, 32)
  # ... and a SET_ITEM pickaxe made collect_stone succeed
  bare = ec.oracle_run(0, ec.SEEDS[0], without=(0, 3), steps=3)
  assert ach(r0, 2, 'collect_stone') == 1 and r0.snapshots[2]['mat'][32, 33] == ec.MAT['path']
  assert ach(bare, 2, 'collect_stone') == 0 and bare.snapshots[2]['mat'][32, 33] == ec.MAT['stone']
  # a plant ripened by SET_OBJECT was eaten
  unripe = ec.oracle_run(1, ec.SEEDS[1], without=(0, 0), steps=3)
  assert ach(r1, 1, 'eat_plant') == 1 and ach(unripe, 1, 'eat_plant') == 0
  # the removed cow is gone and the despawn / spawn balance ran afterwards
  assert (ec.COW, 50, 50) in [o[:3] for o in r1.snapshots[0]['objects']] and (ec.COW, 50, 50) not in [o[:3] for o in r1.edited[0]['objects']]
  assert r1.balance[-1] > r1.balance[0] and r0.balance[-1] > 0 and r2.balance[-1] > 0, 'no balance spawn or despawn behind the edits'
  # a MOVE across a chunk border appended a new key to chunk_order
  assert r1.edited[0]['chunk_order'] == r1.snapshots[0]['chunk_order'] + [(36, 48, 48, 60)]
  assert r1.edited[9]['chunk_order'][-1] == (36, 48, 36, 48) and r2.edited[4]['chunk_order'][-1] == (0, 12, 0, 12)
  # a SET_CLOCK turned the next frame into a night frame (engine.py:189-196: noise below daylight 0.5)
  assert r1.daylight[4] >= 0.5 and r1.daylight[5] < 0.5 and r1.snapshots[5]['step'] == 161
  assert ec.oracle_run(1, ec.SEEDS[1], without=(4, 0), steps=6).daylight[5] >= 0.5
  # every case runs into the night; the teleported player drank from the cell the edit made water
  assert min(r.daylight[-1] for r in (r0, r1, r2)) < 0.5 and ach(r2, 5, 'collect_drink') == 1


def test_parity_three_edited_envs_through_a_night():
  runs = [ec.oracle_run(k, ec.SEEDS[k]) for k in range(3)]
  hs = HostSimEnv(list(ec.SEEDS), auto_reset=False)
  assert worlds_build.reset_worlds(hs, ec.bank_of(hs, range(3))) == 0
  for i in range(3):
    assert np.array_equal(hs.obs[i], runs[i].frames[0])
  for t in range(ec.T):
    named = [i for i in range(3) if t in ec.SCHEDULES[i]]
    if named:
      obs, rew, done = hs.obs.copy(), hs.reward.copy(), hs.done.copy()
      assert eb.edit(hs, named, [ec.SCHEDULES[i][t] for i in named]) == 0
      for i in named:
        check_row(hs, i, runs[i].edited[t], f'env {i} edited before step {t + 1}')
      assert np.array_equal(hs.obs, obs) and np.array_equal(hs.reward, rew) and np.array_equal(hs.done, done)
    obs, rew, done = hs.step(np.array([ec.tape(i)[t] for i in range(3)], np.int32))
    for i, r in enumerate(runs):
      assert np.array_equal(obs[i], r.frames[t + 1]), f'env {i} step {t + 1}: pixels'
      assert rew[i] == np.float32(r.rewards[t]) and bool(done[i]) == r.dones[t], f'env {i} step {t + 1}: reward / done'
      if (t + 1) % 4 == 0 or t + 1 == ec.T:
        check_row(hs, i, r.snapshots[t + 1], f'env {i} step {t + 1}')
  assert not hs.rec['status'].any()


# ------------------------------------------------------------------ 3. refusals
REFUSALS = ec.refusals()


@pytest.fixture(scope='module')
def refused():
  """Every refusal case at once: env j, in the garden world right behind its reset, gets case j's tape in ONE call."""
  names = sorted(REFUSALS)
  hs = HostSimEnv([100 + j for j in range(len(names))], auto_reset=False)
  bank = ec.bank_of(hs, [1])
  assert worlds_build.reset_worlds(hs, bank) == 0
  before = [hs.snapshot(j) for j in range(len(names))]
  assert eb.edit(hs, list(range(len(names))), np.stack([REFUSALS[n] for n in names])) == 0
  return hs, names, before


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refusals_on_the_device(refused, name):
  """ST_BAD_EDIT is set; the row equals the oracle given clean_edits' tape, at once and six steps on; the tape's other ops are applied."""
  hs, names, before = refused
  j = names.index(name)
  assert hs.rec[j]['status'] == abi.STATUS_BAD_EDIT
  clean, flagged = E.clean_edits(hs, before[j], REFUSALS[name])
  assert flagged and 2 <= len(clean) <= 3
  o = EditedOracle(seed=100 + j)
  o.world = ec.garden()
  o.reset()
  o.edit(clean)
  snap = hs.snapshot(j)
  check_row(hs, j, o.snapshot(), name)
  assert snap['mat'][5, 5] == ec.MAT['sand'] and snap['inventory'][ec.ITEMS.index('wood')] == 3


def test_refused_rows_play_on(refused):
  """... and six steps on (every row of the batch in one walk; last, because it moves the fixture's rows)."""
  hs, names, before = refused
  orcs = []
  for j, name in enumerate(names):
    o = EditedOracle(seed=100 + j)
    o.world = ec.garden()
    o.reset()
    o.edit(E.clean_edits(hs, before[j], REFUSALS[name])[0])
    orcs.append(o)
  hs.rec['status'] = 0
  for a in (ec.ACT['do'], ec.ACT['move_left'], ec.ACT['noop'], ec.ACT['move_down'], ec.ACT['do'], ec.ACT['place_table']):
    obs, _, _ = hs.step(np.full(len(names), a, np.int32))
    for j, o in enumerate(orcs):
      assert np.array_equal(obs[j], o.step(a)[0]), names[j]
  for j, o in enumerate(orcs):
    check_row(hs, j, o.snapshot(), names[j])
  assert not hs.rec['status'].any()


def test_what_is_no_refusal_and_overflow():
  cases = ec.not_refused()
  hs = HostSimEnv([131, 132], auto_reset=False)
  assert worlds_build.reset_worlds(hs, ec.bank_of(hs, [1])) == 0
  before = raw_state(hs)
  assert eb.edit(hs, [0, 1], np.stack([cases['move_in_place'], cases['cow_facing']])) == 0
  for k in STATE_BUFFERS:
    assert np.array_equal(hs.buf[k], before[k]), k
  for j, name in enumerate(('move_in_place', 'cow_facing')):
    clean, flagged = E.clean_edits(hs, hs.snapshot(j), cases[name])
    assert not flagged and len(clean) == 0
  # a full slot table stays ST_OBJ_OVERFLOW, as obj_add reports it everywhere, and the row stays consistent
  small = HostSimEnv([133], auto_reset=False, max_objects=16)
  assert worlds_build.reset_worlds(small, ec.bank_of(small, [1])) == 0
  assert small.rec[0]['nobj'] == 16 and small.rec[0]['status'] == abi.ST_OBJ_OVERFLOW   # (the world alone overflows it)
  small.rec['status'] = 0
  assert eb.edit(small, [0], [E.remove(32, 33), E.add('cow', 20, 20), E.add('cow', 21, 21)]) == 0
  assert small.rec[0]['status'] == abi.ST_OBJ_OVERFLOW and small.rec[0]['nobj'] == 16
  assert (ec.COW, 20, 20) in [o[:3] for o in small.snapshot(0)['objects']] and (ec.COW, 21, 21) not in [o[:3] for o in small.snapshot(0)['objects']]
  small.step(np.array([0], np.int32))


# ------------------------------------------------------------------ 4. unnamed rows, the index check
def test_unnamed_rows_are_bit_identical():
  hs = HostSimEnv([61, 62, 63, 64, 65], auto_reset=False, want_semantic=True)
  hs.reset()
  for t in range(3):
    hs.step(np.full(5, t + 1, np.int32))
  before, obs, rew, done = raw_state(hs), hs.obs.copy(), hs.reward.copy(), hs.done.copy()
  pos = {i: hs.snapshot(i)['objects'][0][1:3] for i in (1, 3)}
  tapes = [[E.set_cell(*pos[i], 'sand'), E.move(*pos[i], 1 + i, 2), E.set_item('wood', 4), E.set_clock(200)] for i in (1, 3)]
  assert eb.edit(hs, [3, 1], tapes[::-1]) == 0
  for i in (0, 2, 4):
    for k in STATE_BUFFERS:
      assert np.array_equal(hs.buf[k][i], before[k][i]), (i, k)
  assert np.array_equal(hs.obs, obs) and np.array_equal(hs.reward, rew) and np.array_equal(hs.done, done)
  for i in (1, 3):
    s = hs.snapshot(i)
    assert s['objects'][0][1:3] == (1 + i, 2) and s['mat'][pos[i]] == ec.MAT['sand'] and s['step'] == 200
    for k in ('mt', 'semantic', 'terminal'):   # what an edit never touches, of the named rows too
      assert np.array_equal(hs.buf[k][i], before[k][i]), (i, k)
    r, b = hs.rec[i], state.rec_view(before['rec'])[i]
    for f in ('mt_pos', 'episode', 'seed_lane', 'player_last_health', 'env_last_health', 'unlocked', 'dhealth', 'new_unlocked', 'dead', 'done',
              'needs_reset', 'ep_dhealth', 'ep_unlock_steps', 'status'):
      assert r[f] == b[f], (i, f)
  # a bad index list refuses the whole call: ST_BAD_COPY in the named rows that exist, nothing else changes
  mid = raw_state(hs)
  for idx, flagged in (([0, 2, 0], [0, 2]), ([4, 5], [4]), ([-1], [0])):
    assert eb.edit(hs, idx, [E.set_item('wood', 1)]) == 1
    for i in flagged:
      assert hs.rec[i]['status'] == abi.ST_BAD_COPY
    hs.rec['status'] = 0
    for k in STATE_BUFFERS:
      assert np.array_equal(hs.buf[k], mid[k]), (idx, k)
  # what the entry point refuses on the host; n == 0 does nothing
  one = E.encode(hs, [E.NOP], 1)
  lib, C, p = eb.lib(), eb.C, eb._p
  call = lambda idx, n, ops, per: lib.hostsim_edit_envs(C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), idx, n, ops, per, p(np.zeros(6, np.int32)), 1, None)
  i0 = np.zeros(1, np.int32)
  assert call(p(i0), 0, p(one), 1) == 0 and call(None, 0, None, 0) == 0
  for bad in ((None, 1, p(one), 1), (p(i0), 1, None, 1), (p(i0), 1, p(one), 0), (p(i0), -1, p(one), 1), (p(i0), 6, p(one), 1),
              (p(i0), 1, C.c_void_p(p(one).value + 4), 1)):
    assert call(*bad) == -1, bad


def test_clock_edit_refreshes_the_dispatch_hint():
  """An ordered handle keeps next_step[env] = the number of the step the env runs next: a SET_CLOCK writes the named env's entry,
  a refused one and a tape without one write nothing, no other entry changes."""
  hs = HostSimEnv([141, 142, 143, 144], auto_reset=False)
  hs.reset()
  hint = np.full(4, -7, np.int32)
  tapes = [[E.set_item('wood', 1), E.set_clock(200), E.set_clock(321)], [E.set_item('wood', 2)], [eb.edits.NOP]]
  assert eb.edit(hs, [3, 0, 2], tapes, next_step=hint) == 0
  assert hint.tolist() == [-7, -7, -7, 322] and [int(s) for s in hs.rec['step']] == [0, 0, 0, 321]
  assert eb.edit(hs, [1], np.array([[ec.raw(abi.EDIT_SET_CLOCK, 10000), ec.raw(abi.EDIT_SET_CLOCK, 5)]], np.int32), next_step=hint) == 0
  assert hint.tolist() == [-7, 6, -7, 322] and hs.rec[1]['status'] == abi.STATUS_BAD_EDIT and hs.rec[1]['step'] == 5


def test_clock_edit_without_an_episode_length():
  """Env(length=None): the clock is bounded by the daylight table alone."""
  hs = HostSimEnv([151, 152], auto_reset=False, length=None, n_daylight=700)
  assert hs.cfg.length == 0 and hs.cfg.n_daylight == 700
  hs.reset()
  assert eb.edit(hs, [0, 1], [[E.set_clock(640)], [E.set_clock(699)]]) == 0
  assert not hs.rec['status'].any() and [int(s) for s in hs.rec['step']] == [640, 699]
  with pytest.raises(ValueError):
    E.encode(hs, [E.set_clock(700)], 1)
  assert eb.edit(hs, [0], np.array([[ec.raw(abi.EDIT_SET_CLOCK, 700)]], np.int32)) == 0
  assert hs.rec[0]['status'] == abi.STATUS_BAD_EDIT and hs.rec[0]['step'] == 640
  hs.rec['status'] = 0
  o = EditedOracle(seed=151, length=None)
  o.reset()
  o.edit(ec.rows([E.set_clock(640)]))
  for a in (1, 2, 5, 0):
    obs, _, done = hs.step(np.array([a, 0], np.int32))
    want, _, wdone, _ = o.step(a)
    assert np.array_equal(obs[0], want) and bool(done[0]) == bool(wdone)
  assert_same(hs.snapshot(0), o.snapshot(), 'step 644 of an unbounded episode')


# ------------------------------------------------------------------ 5. a tape of NOPs
def test_nop_tape_changes_nothing():
  a, b = (HostSimEnv([71, 72], auto_reset=False) for _ in range(2))
  rs = np.random.RandomState(4)
  tape = rs.randint(0, 17, size=(30, 2)).astype(np.int32)
  for hs in (a, b):
    hs.reset()
    for t in range(10):
      hs.step(tape[t])
  before, snap = raw_state(a), a.snapshot(1)
  lane = state.seed_lanes([72])[0]
  assert eb.edit(a, [1], [[E.NOP] * 70]) == 0   # (two rounds of the op loop: 64 + 6)
  assert eb.edit(a, [0], np.zeros((1, 1, 8), np.int32)) == 0
  for k in STATE_BUFFERS:
    assert np.array_equal(a.buf[k], before[k]), k
  assert_same(a.snapshot(1), snap, 'NOP tape')
  assert state.fingerprint_host(a.snapshot(1), lane) == state.fingerprint_host(snap, lane)
  for t in range(10, 30):
    oa, ra, da = a.step(tape[t])
    ob, rb, db = b.step(tape[t])
    assert np.array_equal(oa, ob) and np.array_equal(ra, rb) and np.array_equal(da, db), t
  for k in STATE_BUFFERS:
    assert np.array_equal(a.buf[k], b.buf[k]), k


# ------------------------------------------------------------------ 6. other geometries
@pytest.mark.parametrize('area,view,size', [((42, 30), (7, 9), (84, 72)), ((132, 132), (9, 9), (64, 64)), ((256, 256), (9, 9), (64, 64))],
                         ids=['42x30-lds', '132x132-lds-beyond-64K', '256x256-global'])
def test_other_geometries(area, view, size):
  """Maps staged in LDS with unaligned rows, the largest LDS-resident worlds (the kernel's LDS exceeds the 64 KB a launch gets
  without asking), and the large-world layout -- maps, slot map and slot table in global memory, edited in place: a handful of
  edits behind a few steps (holes in the table), then 30 steps against the oracle."""
  hs = HostSimEnv([81, 82], area=area, view=view, size=size, auto_reset=False)
  assert bool(hs.lib.hostsim_slot_map_derived(eb.C.byref(hs.cfg))) == (area[0] < 256)
  world = wc.small_world(area)
  assert worlds_build.reset_worlds(hs, WorldBank(hs, world['mat'][None], [world['objects']], [world['inventory']])) == 0
  first, second = ec.geometry_edits(area)
  rs = np.random.RandomState(9)
  tape = rs.randint(0, 17, size=34)
  orcs = []
  for i in range(2):
    o = EditedOracle(seed=81 + i, area=area, view=view, size=size)
    o.world = world
    assert np.array_equal(hs.obs[i], o.reset())
    orcs.append(o)
  geo = dict(area=area, n_daylight=int(hs.cfg.n_daylight), length=10000)
  for t in range(34):
    if t in (0, 4):
      ops = first if t == 0 else second
      assert eb.edit(hs, [1, 0], ops) == 0
      for i, o in enumerate(orcs):
        o.edit(E.encode(geo, ops, 1)[0])
        check_row(hs, i, o.snapshot(), f'env {i} edited before step {t + 1}')
    obs, _, _ = hs.step(np.full(2, tape[t], np.int32))
    for i, o in enumerate(orcs):
      assert np.array_equal(obs[i], o.step(int(tape[t]))[0]), (t, i)
  for i, o in enumerate(orcs):
    check_row(hs, i, o.snapshot(), f'env {i} step 34')
  assert not hs.rec['status'].any()


def test_edit_layout_sizes():
  """The kernel's LDS: the env's tables and nothing else (DESIGN.md 4's figures)."""
  sizes = {}
  for area in ((64, 64), (42, 30), (256, 256), (132, 132)):
    hs = HostSimEnv([1], area=area, auto_reset=False)
    sizes[area] = eb.lds_bytes(hs)
  assert sizes == {(64, 64): EDIT_LDS[0], (42, 30): EDIT_LDS[1], (256, 256): EDIT_LDS[2], (132, 132): EDIT_LDS[3]}, sizes
  assert EDIT_LDS[3] > 64 * 1024   # (crafter_create allows the kernel that much: handle.hpp big_lds_kernels)


EDIT_LDS = (20352, 11296, 14272, 66912)


# ------------------------------------------------------------------ 7. the stand-alone program
def test_sanitized_standalone_program(tmp_path):
  """The body under -fsanitize=address,undefined in a program of its own (never loaded into Python), fed every refusal case,
  tapes of out-of-range words, a refused index list and the parity cases' edits, every array a heap block of exactly its size: it
  must finish clean and print what the shared library computes."""
  exe = eb.build_sanitized()
  names = sorted(REFUSALS)
  rs = np.random.RandomState(12)
  wild = rs.randint(-2 ** 31, 2 ** 31 - 1, size=(4, 80, 8), dtype=np.int64).astype(np.int32)
  wild[:, :, 0] = rs.randint(-1, 10, size=(4, 80))   # mostly known kinds, with arguments from all over the int32 range
  edge = np.array([[[k, v, v, v, v, v, v, v] for k in range(10) for v in (-2 ** 31, -1, 0, 63, 64, 2 ** 31 - 1)]] * 2, np.int32)
  def garden_envs(n, **kw):
    hs = HostSimEnv([100 + j for j in range(n)], auto_reset=False, **kw)
    assert worlds_build.reset_worlds(hs, ec.bank_of(hs, [1])) == 0
    return hs
  calls = [(lambda: garden_envs(len(names)), list(range(len(names))), np.stack([REFUSALS[n] for n in names])),
           (lambda: garden_envs(4), [3, 1, 0, 2], wild), (lambda: garden_envs(2), [0, 1], edge),
           (lambda: garden_envs(3), [0, 2, 2], wild[:3]),
           (lambda: garden_envs(3), [2, 0], [ec.SCHEDULES[1][0], ec.SCHEDULES[0][0]])]
  big = HostSimEnv([81, 82], area=(256, 256), auto_reset=False)
  world = wc.small_world((256, 256))
  bank = WorldBank(big, world['mat'][None], [world['objects']], [world['inventory']])
  def big_env():
    hs = HostSimEnv([81, 82], area=(256, 256), auto_reset=False)
    assert worlds_build.reset_worlds(hs, bank) == 0
    return hs
  calls.append((big_env, [1, 0], np.concatenate([edge, wild[:2, :60]], axis=1)))
  for k, (make, idx, ops) in enumerate(calls):
    hs = make()
    blob = tmp_path / f'call{k}.blob'
    eb.dump(hs, blob, idx, ops)
    proc = subprocess.run([str(exe), str(blob)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    verdict = eb.edit(hs, idx, ops)
    assert verdict == (1 if k == 3 else 0)
    assert proc.stdout.splitlines() == eb.lines(hs, verdict), k
    if verdict == 0:
      hs.step(np.zeros(hs.cfg.num_envs, np.int32))   # the rows are steppable whatever the tape held


# ------------------------------------------------------------------ 8. encode()
def test_encode_and_its_errors():
  geo = dict(area=(64, 64), n_daylight=10002, length=10000)
  t = E.encode(geo, [E.set_cell(1, 2, 'stone'), E.add('Zombie', 3, 4), E.add(ec.ARROW, 5, 6, facing=(-1, 0), aux=0), E.remove(7, 8),
                     E.move(1, 2, 3, 4), E.set_object(9, 9, health=2, aux=7), E.set_object(9, 9, facing=(0, -1)), E.set_item('wood', 9),
                     E.set_player(sleeping=True, recover2=-30), E.set_clock(9999), E.NOP], 2)
  assert t.shape == (2, 12, 8) and t.dtype == np.int32 and np.array_equal(t[0], t[1])
  assert t[0].tolist() == [[1, 1, 2, ec.MAT['stone'], 0, 0, 0, 0], [2, 3, 3, 4, 5, 0, 0, 0], [2, 5, 5, 6, 0, -1, 0, 0], [3, 7, 8, 0, 0, 0, 0, 0],
                           [4, 1, 2, 3, 4, 0, 0, 0], [5, 9, 9, 5, 2, 0, 0, 7], [5, 9, 9, 2, 0, 0, -1, 0], [6, ec.ITEMS.index('wood'), 9, 0, 0, 0, 0, 0],
                           [7, 0, 1, 0, 0, 0, 0, 0], [7, 4, -30, 0, 0, 0, 0, 0], [8, 9999, 0, 0, 0, 0, 0, 0], [0] * 8]
  per = E.encode(geo, [[E.remove(1, 1)], [], [E.NOP, E.set_clock(0)]], 3)
  assert per.shape == (3, 2, 8) and per[1].tolist() == [[0] * 8] * 2 and per[2, 1, 0] == abi.EDIT_SET_CLOCK
  assert E.encode(geo, [], 2).shape == (2, 1, 8) and E.encode(dict(area=(8, 8)), [E.set_clock(10 ** 6)], 1)[0, 0, 1] == 10 ** 6
  bad = [E.set_cell(64, 0, 'stone'), E.set_cell(0, -1, 'stone'), E.set_cell(0, 0, 'mud'), E.set_cell(0, 0, 0), E.set_cell(0, 0, 13),
         E.add('player', 1, 1), E.add('dragon', 1, 1), E.add(0, 1, 1), E.add(7, 1, 1), E.add('cow', 64, 1), E.add('arrow', 1, 1, facing=(1, 1)),
         E.add('cow', 1, 1, health=128), E.add('cow', 1, 1, aux=2 ** 31), E.remove(-1, 0), E.move(0, 0, 0, 64), E.move(64, 0, 0, 0),
         E.set_object(0, 64, aux=1), E.set_object(0, 0, facing=(0, 0)), E.set_object(0, 0, health=-129), E.set_item('gold', 1),
         E.set_item(16, 1), E.set_item('wood', 10), E.set_item('health', -1), E.set_player(mood=1), E.set_player(sleeping=2),
         E.set_player(hunger2=51), E.set_player(fatigue2=-21), E.set_player(recover2=51), E.set_clock(-1), E.set_clock(10000),
         (99,), (abi.EDIT_REMOVE, 1), 'remove', (1.5, 2), E.set_cell(1.9, 2, 'stone'), E.set_cell(1, 2.0, 'stone'), E.move(1, 1, 2.5, 1),
         E.add('cow', 1, 1, health=2.0), E.add('cow', 1, 1, aux=0.5), E.add('arrow', 1, 1, facing=(1.0, 0)), E.set_object(1, 1, aux=1.5),
         E.set_item('wood', 2.0), E.set_player(hunger2=1.5), E.set_clock(3.0), E.set_cell('1', 2, 'stone')]
  for op in bad:
    with pytest.raises(ValueError):
      E.encode(geo, [E.NOP, op], 1)
  with pytest.raises(ValueError):
    E.encode(geo, [[E.NOP], [E.NOP]], 3)
  with pytest.raises(ValueError):
    E.encode(dict(area=(64, 64), n_daylight=500), [E.set_clock(500)], 1)
  assert E.encode(geo, [E.set_cell(64, 0, 13), E.add('player', 1, 1), E.set_clock(-1)], 1, validate=False)[0, :, 0].tolist() == [1, 2, 8]


# ------------------------------------------------------------------ 9. the library
def test_entry_point_header_and_constants(tmp_path):
  """crafter_edit_envs is declared in a header of its own, listed in lib.EXTENSIONS and build.sources(), exported by the library;
  the header is pedantic C99 by itself and its constants are the Python ones."""
  from crafter_amd import build, lib as hiplib
  assert 'crafter_edit_envs' not in (ROOT / 'include' / 'crafter_hip.h').read_text() and 'crafter_edit_envs' not in hiplib.SIGNATURES
  assert ROOT / 'include' / 'crafter_hip_edit.h' in build.sources() and len(build.UNITS) == 5
  where, restype, argtypes = hiplib.EXTENSIONS['crafter_edit_envs']
  assert where == 'crafter_hip_edit.h' and len(argtypes) == 6 and argtypes[2] is hiplib.C.c_int32 and argtypes[4] is hiplib.C.c_int32
  nm = subprocess.run(['nm', '-D', '--defined-only', str(build.build())], capture_output=True, text=True, check=True).stdout
  assert 'crafter_edit_envs' in set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert hiplib.load().crafter_abi_version() == 7
  assert abi.STATUS_BAD_EDIT == 256 and 'ST_BAD_EDIT' in abi.ALL_STATUS_NAMES[abi.STATUS_BAD_EDIT] and crafter_amd.edits is E
  if not shutil.which('gcc'):
    pytest.skip('needs gcc')
  names = ['ST_BAD_EDIT', 'EDIT_WORDS', 'EDIT_NOP', 'EDIT_SET_CELL', 'EDIT_ADD', 'EDIT_REMOVE', 'EDIT_MOVE', 'EDIT_SET_OBJECT', 'EDIT_SET_ITEM',
           'EDIT_SET_PLAYER', 'EDIT_SET_CLOCK', 'EDIT_KINDS', 'EDIT_HEALTH', 'EDIT_FACING', 'EDIT_AUX', 'EDIT_SLEEPING', 'EDIT_HUNGER2',
           'EDIT_THIRST2', 'EDIT_FATIGUE2', 'EDIT_RECOVER2', 'EDIT_FIELDS']
  src = tmp_path / 'edit.c'
  src.write_text('#include <stdio.h>\n#include "crafter_hip_edit.h"\nint main(void) {\n' +
                 ''.join(f'  printf("{n} %ld\\n", (long)CRAFTER_{n});\n' for n in names) + '  return 0;\n}\n')
  subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', f'-I{ROOT / "include"}', str(src), '-o', str(tmp_path / 'edit')], check=True)
  out = subprocess.run([str(tmp_path / 'edit')], capture_output=True, text=True, check=True).stdout
  got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
  want = {'ST_BAD_EDIT': abi.STATUS_BAD_EDIT, 'EDIT_WORDS': abi.EDIT_WORDS, 'EDIT_KINDS': abi.EDIT_KINDS, 'EDIT_HEALTH': abi.EDIT_HEALTH,
          'EDIT_FACING': abi.EDIT_FACING, 'EDIT_AUX': abi.EDIT_AUX, 'EDIT_FIELDS': len(abi.EDIT_FIELDS)}
  want.update({f'EDIT_{n.upper()}': i for i, n in enumerate(abi.EDIT_FIELDS)})
  want.update({n: getattr(abi, n) for n in names if n not in want})
  assert got == want


def test_edit_kernel_budget():
  """The edit kernel's resource report, from the compiler's own output (DESIGN.md 4's row): no scratch, no spill."""
  from crafter_amd import build
  usage = {k: v for k, v in build.resource_usage().items() if k.startswith('crafter_edit_envs_kernel')}
  assert list(usage) == ['crafter_edit_envs_kernel'], sorted(usage)
  u = usage['crafter_edit_envs_kernel']
  assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, u
  assert u['vgprs'] == EDIT_VGPRS and u['occupancy'] == EDIT_OCCUPANCY, u
  assert u['sgprs'] == EDIT_SGPRS and u['sgpr_spill'] == EDIT_SGPR_SPILL, u


EDIT_VGPRS, EDIT_OCCUPANCY, EDIT_SGPRS, EDIT_SGPR_SPILL = 76, 6, 106, 21
