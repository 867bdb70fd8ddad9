"""Authored worlds on the CPU: the body of crafter_reset_worlds (csrc/env_worlds.hpp) through WaveHost against the oracle whose
world function is "write this map, World.add these objects" (tests/worlds_ref.py), the device-side validation, masked and
unnamed rows, the export -> bank round trip, other geometries, the stand-alone sanitised build, and the host side of WorldBank."""
import subprocess

import numpy as np
import pytest

from crafter_amd import abi, state
from crafter_amd.worlds import WorldBank, worlds_of
from tests import worlds_cases as wc
from tests.hostsim import worlds_build
from tests.hostsim.driver import HostSimEnv
from tests.parity import assert_same, diff_snapshots
from tests.worlds_ref import AuthoredOracle, clean_world

SEEDS = [31, 32, 33]
STATE_BUFFERS = ('mat', 'objmap', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'semantic', 'terminal')


def raw_state(hs):
  return {k: hs.buf[k].copy() for k in STATE_BUFFERS}


def follow(hs, runs, rows, steps, every=1):
  """Steps HostSimEnv rows `rows` along their cases' tapes next to the recorded oracle runs: pixels, reward, done at every step,
  the state every `every` steps."""
  n = hs.cfg.num_envs
  for t in range(steps):
    acts = np.zeros(n, np.int32)
    for i, k in rows.items():
      acts[i] = wc.tape(k)[t]
    obs, rew, done = hs.step(acts)
    for i, k in rows.items():
      r = runs[i]
      assert np.array_equal(obs[i], r.frames[t + 1]), f'env {i} step {t + 1}: pixels'
      assert rew[i] == np.float32(r.rewards[t]) and bool(done[i]) == r.dones[t], f'env {i} step {t + 1}: reward / done'
      if (t + 1) % every == 0 or t + 1 == steps:
        assert_same(hs.snapshot(i), r.snapshots[t + 1], f'env {i} step {t + 1}')


def test_parity_three_worlds_through_a_night():
  runs = {i: wc.oracle_run(i, SEEDS[i]) for i in range(3)}
  # what the tape must show on the oracle ALONE, or a wrong census / aux / facing / chunk order would pass unnoticed
  health = wc.ITEMS.index('health')
  r0, r1 = runs[0], runs[1]
  assert max(r.balance[-1] for r in runs.values()) >= 1, 'no balance spawn or despawn'
  assert r0.snapshots[1]['inventory'][health] == r0.snapshots[0]['inventory'][health] - 2, 'the authored zombie did not hit at step 1'
  assert r0.snapshots[0]['objects'][0][1:3] == (10, 12) and r0.snapshots[0]['chunk_order'][0] == (24, 36, 24, 36) and \
      r0.snapshots[0]['chunk_order'][1] == (0, 12, 12, 24), 'the player was not authored into another chunk'
  assert r0.snapshots[3]['achievements'][wc.RULES['achievements'].index('make_wood_pickaxe')] == 1, 'make_wood_pickaxe was not legal'
  assert r1.snapshots[1]['achievements'][wc.RULES['achievements'].index('eat_plant')] == 1, 'the ripe plant was not eaten'
  arrows = [[o for o in s['objects'] if o[0] == wc.ARROW and o[4] == 1] for s in r1.snapshots[:8]]
  assert [a[0][1] for a in arrows[:5]] == [34, 35, 36, 37, 38] and not arrows[5], 'the authored arrow did not fly and vanish'
  assert r1.snapshots[6]['mat'][26, 35] == wc.MAT['path'], 'the second arrow did not break the table'

  hs = HostSimEnv(SEEDS, auto_reset=False)
  bank = wc.bank_of(hs, range(3))
  assert worlds_build.reset_worlds(hs, bank) == 0
  for i in range(3):
    assert np.array_equal(hs.obs[i], runs[i].frames[0]), f'env {i}: first frame'
    assert_same(hs.snapshot(i), runs[i].snapshots[0], f'env {i} reset')
  follow(hs, runs, {0: 0, 1: 1, 2: 2}, wc.T)
  assert not hs.rec['status'].any()


def oracle_on(world, seed, steps, tape):
  o = AuthoredOracle(seed=seed, world=world)
  frames, snaps = [o.reset()], [o.snapshot()]
  for a in tape[:steps]:
    frames.append(o.step(int(a))[0])
    snaps.append(o.snapshot())
  return frames, snaps


@pytest.mark.parametrize('name', sorted(wc.bad_cases()))
def test_validation_on_the_device(name):
  """Each flagged case sets ST_BAD_WORLD in its env only; the repaired world is the oracle's on the cleaned input, at the reset
  and 12 steps on (a skipped record leaves no trace in any table)."""
  world = wc.edited_garden(wc.bad_cases()[name])
  with pytest.raises(ValueError):
    WorldBank(dict(area=(64, 64)), world['mat'][None], [world['objects']], [world['inventory']])
  good = wc.edited_garden(lambda w: None)
  hs = HostSimEnv([41, 42], auto_reset=False)
  bank = WorldBank(hs, np.stack([world['mat'], good['mat']]), [world['objects'], good['objects']], [world['inventory']] * 2, validate=False)
  assert worlds_build.reset_worlds(hs, bank) == 0
  assert list(hs.rec['status']) == [abi.STATUS_BAD_WORLD, 0]
  mat, objs, flagged = clean_world(world, (64, 64), len(wc.MAT), wc.MAT['grass'])
  assert flagged
  tape = wc.tape(1)
  for i, w in enumerate([dict(mat=mat, objects=objs, inventory=world['inventory']), good]):
    frames, snaps = oracle_on(w, 41 + i, 12, tape)
    assert np.array_equal(hs.obs[i], frames[0])
    assert_same(hs.snapshot(i), snaps[0], f'{name} env {i} reset')
  for t in range(12):
    obs, _, _ = hs.step(np.full(2, tape[t], np.int32))
  for i, w in enumerate([dict(mat=mat, objects=objs, inventory=world['inventory']), good]):
    frames, snaps = oracle_on(w, 41 + i, 12, tape)
    assert np.array_equal(obs[i], frames[12])
    assert_same(hs.snapshot(i), snaps[12], f'{name} env {i} step 12')


def test_world_id_out_of_range_and_host_refusals():
  hs = HostSimEnv([51, 52, 53, 54], auto_reset=False)
  hs.reset()
  hs.step(np.array([1, 2, 3, 4], np.int32))
  bank = wc.bank_of(hs, [1])
  before, obs = raw_state(hs), hs.obs.copy()
  assert worlds_build.reset_worlds(hs, bank, world_ids=[1, -1, 0, 2 ** 31 - 1]) == 0
  after = raw_state(hs)
  for i in (0, 1, 3):   # untouched but for the bit
    assert hs.rec[i]['status'] == abi.STATUS_BAD_WORLD
    hs.rec[i]['status'] = 0
    for k in STATE_BUFFERS:
      assert np.array_equal(hs.buf[k][i], before[k][i]), (i, k)
    assert np.array_equal(hs.obs[i], obs[i])
  assert hs.rec[2]['status'] == 0 and hs.rec[2]['episode'] == 2 and hs.rec[2]['step'] == 0
  # overflow of the batch's slot table: ST_OBJ_OVERFLOW, as World.add sets it, and a consistent row
  small = HostSimEnv([55], auto_reset=False, max_objects=8)
  assert worlds_build.reset_worlds(small, wc.bank_of(small, [0])) == 0
  assert small.rec[0]['status'] == abi.ST_OBJ_OVERFLOW and small.rec[0]['nobj'] == 8
  small.step(np.array([0], np.int32))
  # what the entry point refuses on the host
  lib, C = worlds_build.lib(), worlds_build.C
  p = lambda a: a.ctypes.data_as(C.c_void_p)
  args = lambda **kw: [C.byref(hs.cfg), C.byref(hs.tb), C.byref(hs.st), None, None] + [
      kw.get(k, p(a)) for k, a in (('mat', bank.mat), ('objs', bank.objs), ('nobj', bank.nobj))] + [None, kw.get('n', 1), kw.get('cap', 1), p(hs.obs)]
  for bad in (dict(mat=None), dict(objs=None), dict(nobj=None), dict(n=0), dict(cap=-1)):
    assert lib.hostsim_reset_worlds(*args(**bad)) == -1, bad


def test_unmasked_rows_are_bit_identical():
  hs = HostSimEnv([61, 62, 63, 64, 65], auto_reset=False, want_semantic=True)
  hs.reset()
  for t in range(3):
    hs.step(np.full(5, t + 1, np.int32))
  before, obs = raw_state(hs), hs.obs.copy()
  bank = wc.bank_of(hs, [2, 0])
  assert worlds_build.reset_worlds(hs, bank, mask=[0, 1, 0, 0, 7], world_ids=[9, 1, 9, 9, 0]) == 0
  for i in (0, 2, 3):
    for k in STATE_BUFFERS:
      assert np.array_equal(hs.buf[k][i], before[k][i]), (i, k)
    assert np.array_equal(hs.obs[i], obs[i])
  for i, k in ((1, 0), (4, 2)):
    r = wc.oracle_run(k, 61 + i, steps=5, first_episode=2)
    assert np.array_equal(hs.obs[i], r.frames[0])
    assert_same(hs.snapshot(i), r.snapshots[0], f'env {i}')
    base = len(wc.MAT)
    sem = hs.buf['semantic'][i].reshape(64, 64)
    want = r.snapshots[0]['mat'].copy()
    for o in r.snapshots[0]['objects']:
      want[o[1], o[2]] = base + o[0]
    assert np.array_equal(sem, want)
  assert not hs.rec['status'].any()


def test_round_trip_export_bank_reset():
  """A generated world, played for a while (holes in the slot table, a changed inventory), exported and reset into other rows:
  mat, the live objects in compacted slot order and the inventory come back, and the copies then live the life the oracle
  lives on the exported world."""
  hs = HostSimEnv([71, 72, 73], auto_reset=False)
  hs.reset()
  rs = np.random.RandomState(3)
  for t in range(40):
    hs.step(rs.choice([1, 2, 3, 4, 5, 5], size=3).astype(np.int32))
  n_items = len(wc.ITEMS)
  export = lambda rows: worlds_of(hs.buf['mat'][rows].reshape(-1, 64, 64), state.objs_view(hs.buf['objs'])[rows], hs.rec[rows], n_items)
  w = export([0])
  assert w['objects'][0][0][0] == wc.PLAYER and len(w['objects'][0]) > 5
  bank = WorldBank(hs, **w)
  assert worlds_build.reset_worlds(hs, bank, mask=[0, 1, 1]) == 0
  back = export([1, 2])
  for j in range(2):
    assert np.array_equal(back['mat'][j], w['mat'][0]) and back['objects'][j] == w['objects'][0]
    assert np.array_equal(back['inventory'][j], w['inventory'][0])
    assert list(hs.rec[1 + j]['inv'][:n_items]) == list(w['inventory'][0])
  world = dict(mat=w['mat'][0], objects=w['objects'][0], inventory=w['inventory'][0])
  orcs = []
  for i in (1, 2):
    o = AuthoredOracle(seed=71 + i)
    o.reset()
    o.world = world
    assert np.array_equal(hs.obs[i], o.reset())
    assert_same(hs.snapshot(i), o.snapshot(), f'copy {i}')
    orcs.append(o)
  for t in range(25):
    a = int(rs.randint(0, 17))
    obs, _, _ = hs.step(np.full(3, a, np.int32))
    for i, o in zip((1, 2), orcs):
      assert np.array_equal(obs[i], o.step(a)[0]), (t, i)
  for i, o in zip((1, 2), orcs):
    assert_same(hs.snapshot(i), o.snapshot(), f'copy {i} after 25 steps')


@pytest.mark.parametrize('area,view,size', [((42, 30), (7, 9), (84, 72)), ((256, 256), (9, 9), (64, 64))], ids=['42x30-lds', '256x256-global'])
def test_other_geometries(area, view, size):
  """A non-default view / area whose maps are LDS-resident (W * H = 1260 is no multiple of 16: env 0 copies 78 vectors and a
  12-byte tail, env 1's row is not 16-byte aligned and is copied byte by byte), and the
  large-world layout (maps and slot table in global memory, big_reset_layout)."""
  hs = HostSimEnv([81, 82], area=area, view=view, size=size, auto_reset=False)
  assert bool(hs.lib.hostsim_slot_map_derived(worlds_build.C.byref(hs.cfg))) == (area[0] < 256)
  hs.reset()
  world = wc.small_world(area)
  bank = WorldBank(hs, world['mat'][None], [world['objects']], [world['inventory']])
  assert worlds_build.reset_worlds(hs, bank) == 0
  rs = np.random.RandomState(9)
  tape = rs.randint(0, 17, size=30)
  orcs = []
  for i in range(2):
    o = AuthoredOracle(seed=81 + i, area=area, view=view, size=size)
    o.reset()
    o.world = world
    assert np.array_equal(hs.obs[i], o.reset())
    assert_same(hs.snapshot(i), o.snapshot(), f'env {i} reset')
    orcs.append(o)
  for t in range(30):
    obs, _, _ = hs.step(np.full(2, tape[t], np.int32))
    for i, o in enumerate(orcs):
      assert np.array_equal(obs[i], o.step(int(tape[t]))[0]), (t, i)
  for i, o in enumerate(orcs):
    assert_same(hs.snapshot(i), o.snapshot(), f'env {i} step 30')
  assert not hs.rec['status'].any()


def test_sanitized_standalone_program(tmp_path):
  """The body under -fsanitize=address,undefined in a program of its own (never loaded into Python), fed the validation cases,
  a masked row, world ids in and out of range, and a bank whose arrays are heap blocks of exactly their size: it must finish
  clean and print what the shared library computes."""
  exe = worlds_build.build_sanitized()
  def make():
    return HostSimEnv([91, 92, 93, 94], auto_reset=False)
  worlds = [wc.edited_garden(e) for _, e in sorted(wc.bad_cases().items())] + [wc.meadow(), wc.cave()]
  hs = make()
  bank = WorldBank(hs, np.stack([w['mat'] for w in worlds]), [w['objects'] for w in worlds], validate=False)
  for ids, mask in (([0, 1, 2, 3], None), ([4, 5, 6, 7], None), ([8, 9, 10, 11], [1, 1, 0, 1]), ([12, 13, 14, -3], None)):
    hs = make()
    blob = tmp_path / 'call.blob'
    worlds_build.dump(hs, bank, blob, mask=mask, world_ids=ids)
    proc = subprocess.run([str(exe), str(blob)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert worlds_build.reset_worlds(hs, bank, mask=mask, world_ids=ids) == 0
    assert proc.stdout.splitlines() == worlds_build.lines(hs, mask), ids


def test_world_bank_host_side(tmp_path):
  names = np.full((1, 64, 64), 'grass', dtype=object)
  names[0, 3, 4] = 'table'
  bank = WorldBank(dict(area=(64, 64)), names, [[dict(type='player', x=3, y=5, facing=(0, -1)), ('cow', 9, 9), ('plant', 8, 8, 1, (0, 1), 5)]],
                   [dict(wood=3)])
  assert bank.mat[0, 3, 4] == wc.MAT['table'] and bank.mat[0, 0, 0] == wc.MAT['grass']
  assert bank.worlds()['objects'][0] == [(1, 3, 5, 0, (0, -1), 0), (2, 9, 9, 3, (0, 1), 0), (6, 8, 8, 1, (0, 1), 5)]
  assert bank.inv[0, wc.ITEMS.index('wood')] == 3 and bank.inv[0, wc.ITEMS.index('health')] == 9 and bank.max_objects == 5
  bank.save(tmp_path / 'bank.npz')
  again = WorldBank.load(tmp_path / 'bank.npz')
  assert np.array_equal(again.mat, bank.mat) and np.array_equal(again.objs, bank.objs) and np.array_equal(again.inv, bank.inv)
  for kw in (dict(mat=np.zeros((1, 64, 63), np.uint8)), dict(mat=np.full((1, 64, 64), 'mud', dtype=object)),
             dict(objects=[[('dragon', 1, 1)]]), dict(objects=[[('cow', 1, 1)], []]), dict(inventory=[dict(gold=1)]), dict(inventory=[dict(wood=10)])):
    args = dict(mat=np.full((1, 64, 64), 2, np.uint8), objects=[[]], inventory=None)
    args.update(kw)
    with pytest.raises(ValueError):
      WorldBank(dict(area=(64, 64)), **args)
