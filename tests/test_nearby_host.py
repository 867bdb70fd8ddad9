"""Nearby queries, the parts that need no GPU: crafter_nearby's body on the CPU (tests/hostsim/nearby_host.cpp) against the numpy
mirror (crafter_amd.nearby_host) on generated worlds of every geometry, both window rules and both object walks; the mirror against
what the untouched reference answered (tests/golden/reference_runs/nearby_ref.npz); authored worlds with literal rows; the mask,
the batch tail and the argument checks of the harness entry and of BatchedEnv.nearby's host side; the sanitised stand-alone
program on a dumped env and on rows of random bytes; the entry point, its constants and the kernels' resource budget."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import crafter_amd
from crafter_amd import abi, state
from tests import nearby_cases as nc

ROOT = pathlib.Path(__file__).resolve().parent.parent
GEOS = {'64x64': dict(area=(64, 64)), '42x30': dict(area=(42, 30), view=(7, 9), size=(84, 72)), '48x40': dict(area=(48, 40)),
        '144x144': dict(area=(144, 144)), '256x256': dict(area=(256, 256))}
SEEDS = {'64x64': [5, 6, 7, 8, 9, 10], '42x30': [5, 6, 7, 8], '48x40': [5, 6, 7, 8], '144x144': [5, 6, 7, 8], '256x256': [5, 6, 7, 8]}
DISTANCES, KS = (0, 1, 3, 9, -1), (0, 1, 16, 32)
FILL32, FILL16 = 0x7E7E7E7E, 0x7E7E


def _hostsim(seeds, **kw):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv(seeds, render_obs=False, **kw)
  hs.reset()
  return hs


def _mirror(hs, distance, k, classes, numpy_slices, rows=None):
  rows = range(hs.cfg.num_envs) if rows is None else rows
  got = [state.nearby_host(hs.snapshot(i), nc.N_MATERIALS, distance, k, classes, numpy_slices) for i in rows]
  return np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), np.array([g[2] for g in got], np.int32)


def _assert_equal(got, want, what):
  for name, g, w in zip(('counts', 'ents', 'n'), got, want):
    assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.argwhere(g != w)
    assert not len(bad), f'{what}: {name} differs at {bad[:6].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}'


def _move_players_to_borders(hs, map_state):
  """Env i's player record moved next to border i % 4 (west, east, north, south), onto the first cell there that holds no object;
  where the slot map is state its entry moves too.  -> the cells."""
  cfg = hs.cfg
  objs = state.objs_view(hs.buf['objs'])
  cells = []
  for i in range(cfg.num_envs):
    occupied = hs.snapshot(i)['occupied']
    border = i % 4
    for j in range(3, 30):
      x, y = [(1, j), (cfg.W - 2, j), (j, 1), (j, cfg.H - 2)][border]
      if not occupied[x, y]:
        break
    if map_state:
      objmap = hs.buf['objmap'][i].reshape(cfg.W, cfg.H)
      objmap[int(objs[i, 1]['x']), int(objs[i, 1]['y'])] = 0
      objmap[x, y] = 1
    objs[i, 1]['x'], objs[i, 1]['y'] = x, y
    cells.append((x, y))
  return cells


# ------------------------------------------------------------------ 1. the body against the mirror, generated worlds
@pytest.mark.parametrize('geo', list(GEOS))
def test_body_equals_mirror(geo):
  """After reset, after 30 random steps and with the players then moved next to the four borders: every d of DISTANCES, every K of KS,
  both window rules (NUMPY: d >= 0), every integer equal to the mirror's (computed once per window at K = 32: a shorter list is
  its head).  144 x 144 and 256 x 256 take the 256-thread instance and read objmap where the window is short; on 144 x 144 both
  object walks are forced as well.  The compared cases hold an env with n > K, one with n = 0, and a window clipped at each border."""
  from tests.hostsim import nearby_build as nb
  hs = _hostsim(SEEDS[geo], **GEOS[geo])
  W, H = GEOS[geo]['area']
  wide = geo in ('144x144', '256x256')
  assert nb.in_wave(hs) == (not wide) and nb.map_is_state(hs) == wide
  assert nb.lds_bytes(hs, 0) == 288 and nb.lds_bytes(hs, 16) == 288 + 4 * hs.cfg.max_objects   # 
  acts = np.random.RandomState(17).randint(0, 17, size=(30, len(SEEDS[geo]))).astype(np.int32)
  seen = dict(more=0, none=0, west=0, east=0, north=0, south=0, empty=0)
  for stage in ('reset', 'steps', 'borders'):
    if stage == 'steps':
      for t in range(30):
        hs.step(acts[t])
    if stage == 'borders':
      _move_players_to_borders(hs, wide)
    pos = [(o[1], o[2]) for o in (hs.snapshot(i)['objects'][0] for i in range(hs.cfg.num_envs))]
    for d in DISTANCES:
      for rule in (False, True):
        if rule and d < 0:
          continue
        want = _mirror(hs, d, 32, nc.NOT_PLAYER, rule)
        for k in KS:
          walks = (-1, 0, 1) if geo == '144x144' else (-1,)
          for walk in walks:
            c, e, n = nb.nearby(hs, d, k, nc.NOT_PLAYER, rule, walk=walk)
            what = f'{geo} {stage} d={d} k={k} numpy={rule} walk={walk}'
            _assert_equal((c, e, n) if k else (c,), (want[0], want[1][:, :k], want[2]) if k else (want[0],), what)
            if k:
              seen['more'] += int((n > k).sum())
              seen['none'] += int((n == 0).sum())
        if not rule and d > 0:
          for (x, y) in pos:
            seen['west'] += x - d < 0
            seen['east'] += x + d >= W
            seen['north'] += y - d < 0
            seen['south'] += y + d >= H
        seen['empty'] += int((want[0][:, 0] == 0).sum())
  assert all(seen.values()), seen
  assert not hs.rec['status'].any()


def test_player_class_and_single_classes():
  """The class set: the player alone, zombies alone, every object class -- the body's rows are the mirror's; a list holds no class
  outside its set; the whole-world counts add up to the area and to the live objects."""
  from tests.hostsim import nearby_build as nb
  hs = _hostsim([21, 22, 23], **GEOS['64x64'])
  for t in range(12):
    hs.step(np.array([1, 3, 5], np.int32))
  for classes in (1 << (nc.N_MATERIALS + nc.PLAYER), 1 << (nc.N_MATERIALS + nc.ZOMBIE), nc.ALL_OBJECTS, 1 << (nc.N_MATERIALS + nc.COW) | 1 << (nc.N_MATERIALS + nc.PLANT)):
    for d in (None, 12):
      got = nb.nearby(hs, d, 32, classes)
      _assert_equal(got, _mirror(hs, d, 32, classes, False), f'classes {classes:#x} d={d}')
      c, e, n = got
      for i in range(3):
        rows = e[i, :min(n[i], 32)]
        assert all(classes >> int(r[0]) & 1 for r in rows)
        assert n[i] == sum(int(c[i, cls]) for cls in range(nc.N_MATERIALS + 1, nc.N_CLASSES) if classes >> cls & 1)
  c = nb.nearby(hs, None, 0, 0)[0]
  assert (c[:, 0] == 64 * 64).all() and (c[:, 1: nc.N_MATERIALS + 1].sum(1) == 64 * 64).all()
  assert c[:, nc.N_MATERIALS + 1:].sum(1).tolist() == [len(hs.snapshot(i)['objects']) for i in range(3)]


# ------------------------------------------------------------------ 2. the mirror against the reference fixture
def _check_against_fixture(entry, s, area, snapshot, what):
  """The mirror's NUMPY-window answers for one recorded state against the reference's: material sets, class counts, object
  tuples in the header's order, the window's cells; the whole-world counts against World.count."""
  for di, d in enumerate(nc.DISTANCES):
    mats, by_type, rows, cells = nc.expected(entry, s, di, area)
    counts, ents, n = state.nearby_host(snapshot, nc.N_MATERIALS, d, 32, nc.ALL_OBJECTS, True)
    got_mats = sum(1 << m for m in range(1, nc.N_MATERIALS + 1) if counts[m])
    assert got_mats == mats and counts[0] == cells, (what, d, got_mats, mats, counts[0], cells)
    assert counts[nc.N_MATERIALS + 1:].tolist() == by_type and n == len(rows), (what, d)
    assert [tuple(r) for r in ents[:min(n, 32)].tolist()] == rows[:32], (what, d)
    assert not ents[min(n, 32):].any()
  whole = state.nearby_host(snapshot, nc.N_MATERIALS, None, 0)[0]
  assert whole[1: nc.N_MATERIALS + 1].tolist() == entry['count'][s][1:].tolist() and whole[0] == area[0] * area[1], what


@pytest.mark.parametrize('area', [(64, 64), (42, 30)], ids=['64x64', '42x30'])
def test_mirror_equals_the_reference(area):
  """The recorded runs replayed on the oracle: at every recorded state the mirror gives what World.nearby and World.count gave.
  Then the poked states, where the fixture is asserted to hold both empty and re-clipped numpy windows."""
  from oracle.crafter_oracle import OracleEnv
  fix = nc.load_fixture()
  for a, seed in nc.RUNS:
    if a != area:
      continue
    entry = fix[nc.run_key(a, seed)]
    orc = OracleEnv(area=a, seed=seed)
    orc.reset()
    s = 0
    _check_against_fixture(entry, s, a, orc.snapshot(), f'{seed} reset')
    for t, act in enumerate(nc.tape(seed)):
      orc.step(int(act))
      if (t + 1) % nc.EVERY == 0:
        s += 1
        snap = orc.snapshot()
        assert tuple(entry['pos'][s]) == snap['objects'][0][1:3]
        _check_against_fixture(entry, s, a, snap, f'{seed} step {t + 1}')
    assert s + 1 == len(entry['pos']) == 1 + nc.STEPS // nc.EVERY
  entry = fix[f'{area[0]}x{area[1]}/poke']
  empty = reclipped = 0
  for s, pos in enumerate(nc.poke_positions(area)):
    orc = OracleEnv(area=area, seed=nc.POKE_SEED)
    orc.reset()
    nc.poke_oracle(orc, pos)
    assert tuple(entry['pos'][s]) == pos
    _check_against_fixture(entry, s, area, orc.snapshot(), f'poke {pos}')
    for di, d in enumerate(nc.DISTANCES):
      empty += entry['mats'][s][di] == 0
      reclipped += entry['mats'][s][di] != 0 and (pos[0] - d + area[0] < 0 or pos[1] - d + area[1] < 0)
  assert empty >= 8 and reclipped >= 4, (empty, reclipped)


def test_body_equals_the_reference_on_poked_states():
  """The poked states written into a CPU-harness batch: the BODY's NUMPY windows give the recorded answers, empty windows included."""
  from tests.hostsim import nearby_build as nb
  area = (64, 64)
  positions = nc.poke_positions(area)
  hs = _hostsim([nc.POKE_SEED] * len(positions), area=area)
  objs = state.objs_view(hs.buf['objs'])
  for i, pos in enumerate(positions):
    objs[i, 1]['x'], objs[i, 1]['y'] = pos
  entry = nc.load_fixture()['64x64/poke']
  for di, d in enumerate(nc.DISTANCES):
    c, e, n = nb.nearby(hs, d, 32, nc.ALL_OBJECTS, True)
    for s in range(len(positions)):
      mats, by_type, rows, cells = nc.expected(entry, s, di, area)
      assert sum(1 << m for m in range(1, nc.N_MATERIALS + 1) if c[s, m]) == mats and c[s, 0] == cells, (s, d)
      assert c[s, nc.N_MATERIALS + 1:].tolist() == by_type and n[s] == len(rows), (s, d)
      assert [tuple(r) for r in e[s, :min(n[s], 32)].tolist()] == rows[:32], (s, d)


# ------------------------------------------------------------------ 3. authored worlds
@pytest.mark.parametrize('geo', ['64x64', '42x30', '144x144'])
def test_authored_worlds(geo):
  """The cases of tests/nearby_cases.py authored(): ties in the distance, the facing code, aux beyond int16, class sets that name
  nothing, the player in each corner -- the literal rows and counts, under both window rules where they agree, and the mirror."""
  from tests.hostsim import nearby_build as nb
  from tests.hostsim import worlds_build as wb
  W, H = GEOS[geo]['area']
  cases = nc.authored(W, H)
  hs = _hostsim([0] * len(cases), **GEOS[geo])
  bank = crafter_amd.WorldBank(dict(area=(W, H)), np.stack([c['mat'] for c in cases]), [c['objects'] for c in cases])
  assert wb.reset_worlds(hs, bank, world_ids=np.arange(len(cases))) == 0
  assert not hs.rec['status'].any()
  for i, case in enumerate(cases):
    mask = np.zeros(len(cases), np.uint8)
    mask[i] = 1
    for walk in ((-1, 0, 1) if geo == '144x144' else (-1,)):
      c, e, n = nb.nearby(hs, case['distance'], case['k'], case['classes'], mask=mask, walk=walk)
      rows = [tuple(r) for r in e[i].tolist()]
      live = min(case['n'], case['k'])
      assert n[i] == case['n'] and rows[:live] == case['rows'][:live] and rows[live:] == [(0,) * 6] * (case['k'] - live), (case['name'], rows, n[i])
      for name, count in case['counts'].items():
        assert c[i, nc.CLASSES.index(name)] == count, (case['name'], name, c[i].tolist())
      assert (c[mask == 0] == FILL32).all()
      want = state.nearby_host(hs.snapshot(i), nc.N_MATERIALS, case['distance'], case['k'], case['classes'])
      assert np.array_equal(c[i], want[0]) and np.array_equal(e[i], want[1]) and n[i] == want[2], case['name']
  # the corners under numpy's slices: the west and north ones see nothing at all, the south-east one what the clipped square holds
  names = [c['name'] for c in cases]
  c, e, n = nb.nearby(hs, 2, 4, nc.NOT_PLAYER, True)
  for corner, cells in (('nw', 0), ('ne', 0), ('sw', 0), ('se', 9)):
    i = names.index(f'e-corner-{corner}')
    assert c[i, 0] == cells and n[i] == (2 if cells else 0) and int(c[i].sum()) == (cells + 9 + 3 if cells else 0), (corner, c[i].tolist())


# ------------------------------------------------------------------ 4. mask, tail, arguments
def test_body_rows_tail_mask_and_arguments():
  """Five envs with a row mask, written into sentinel-filled buffers inside larger ones: masked rows and the words around the
  outputs stay as they were, a row never reset gives zeros (the body is also called for one env beyond the batch); what
  crafter_nearby refuses is refused with a message that names the argument, and nothing is written."""
  from tests.hostsim import nearby_build as nb
  from tests.hostsim.driver import HostSimEnv
  hs = _hostsim([11, 12, 13, 14, 15], **GEOS['64x64'])
  hs.step(np.array([1, 2, 3, 4, 5], np.int32))
  C, K = nc.N_CLASSES, 4
  full = nb.nearby(hs, 6, K, nc.NOT_PLAYER)
  raw = np.full(5 * C + 8, FILL32, np.int32), np.full(5 * K * 6 + 8, FILL16, np.int16), np.full(5 + 8, FILL32, np.int32)
  out = raw[0][4:4 + 5 * C].reshape(5, C), raw[1][4:4 + 5 * K * 6].reshape(5, K, 6), raw[2][4:9]
  mask = np.array([1, 0, 0, 1, 0], np.uint8)
  assert nb.call(hs, mask, 6, 0, nc.NOT_PLAYER, K, *out) == 0
  for i in range(5):
    for o, f, fill in zip(out, full, (FILL32, FILL16, FILL32)):
      assert (o[i] == (f[i] if mask[i] else fill)).all()
  for r, fill in zip(raw, (FILL32, FILL16, FILL32)):
    assert (r[:4] == fill).all() and (r[-4:] == fill).all()
  assert nb.call(hs, mask, 6, 0, nc.NOT_PLAYER, 0, out[0], None, None) == 0   # k = 0: ents and n may be null
  before = [o.copy() for o in out]
  refused = [((6, 0, nc.NOT_PLAYER, -1), 'k'), ((6, 0, nc.NOT_PLAYER, 33), 'k'), ((6, 2, nc.NOT_PLAYER, K), 'flags'), ((6, -1, nc.NOT_PLAYER, K), 'flags'),
             ((6, 0, 1 << 6, K), 'classes'), ((6, 0, 1 << 19, K), 'classes'), ((6, 0, 1, K), 'classes'), ((-1, 1, nc.NOT_PLAYER, K), 'distance')]
  for (d, flags, classes, k), word in refused:
    rc = nb.call(hs, None, d, flags, classes, k, *out)
    assert rc != 0 and word in nb.error_text(rc), (d, flags, classes, k, nb.error_text(rc))
  for o, word in (((None, out[1], out[2]), 'counts'), ((out[0], None, out[2]), 'ents or n'), ((out[0], out[1], None), 'ents or n')):
    rc = nb.call(hs, None, 6, 0, nc.NOT_PLAYER, K, *o)
    assert rc != 0 and word in nb.error_text(rc)
  assert all(np.array_equal(a, b) for a, b in zip(before, out))
  never = HostSimEnv([1, 2], render_obs=False, **GEOS['64x64'])   # never reset
  c, e, n = nb.nearby(never, None, 3, nc.ALL_OBJECTS)
  assert not c.any() and not e.any() and not n.any()
  assert [state.nearby_host(never.snapshot(0), nc.N_MATERIALS, None, 3, nc.ALL_OBJECTS)[j].any() for j in (0, 1)] == [False, False]
  tall = HostSimEnv([1], render_obs=False, area=(520, 40))   # a side above NEARBY_MAX_SIDE: the counts only
  tall.reset()
  assert nb.call(tall, None, 3, 0, 0, 0, np.zeros((1, C), np.int32), None, None) == 0
  rc = nb.call(tall, None, 3, 0, 0, 1, np.zeros((1, C), np.int32), np.zeros((1, 1, 6), np.int16), np.zeros(1, np.int32))
  assert rc != 0 and '512' in nb.error_text(rc)
  c = nb.nearby(tall, None, 0, 0)[0]
  assert np.array_equal(c[0], state.nearby_host(tall.snapshot(0), nc.N_MATERIALS, None, 0)[0]) and c[0, 0] == 520 * 40


def test_check_nearby_without_a_device():
  """BatchedEnv.nearby's host side: what it passes on, and every ValueError, with no device in sight."""
  check = lambda *a, **k: crafter_amd.BatchedEnv._check_nearby(nc.CLASSES, nc.N_MATERIALS, (64, 64), 256, *a, **k)
  assert check() == (-1, abi.NEARBY_CLIP, nc.NOT_PLAYER)
  assert check(4, 32, ['zombie', 'skeleton'], True) == (4, abi.NEARBY_NUMPY, 1 << 15 | 1 << 16)
  assert check(-3, 0, 'cow') == (-1, 0, 1 << 14) and check(np.int64(2), np.int32(8), [13, 'plant']) == (2, 0, 1 << 13 | 1 << 18)
  assert check(10 ** 12, 1, [])[0] == 1 << 20 and check(1, 1, [])[2] == 0 and check(0, 1, nc.OBJECT_NAMES)[2] == nc.ALL_OBJECTS
  bad = [dict(k=-1), dict(k=33), dict(k=1.5), dict(k=True), dict(distance=1.5), dict(distance='4'), dict(numpy_slices=True),
         dict(distance=-1, numpy_slices=True), dict(classes=['tree']), dict(classes=['none']), dict(classes=[0]), dict(classes=[19]),
         dict(classes='wood'), dict(classes=[['cow']]), dict(classes=3.0)]
  for kw in bad:
    with pytest.raises(ValueError):
      check(**kw)
  with pytest.raises(ValueError):
    crafter_amd.BatchedEnv._check_nearby(nc.CLASSES, nc.N_MATERIALS, (600, 64), 1200, 4, 1)
  with pytest.raises(ValueError):
    crafter_amd.BatchedEnv._check_nearby(nc.CLASSES, nc.N_MATERIALS, (64, 64), 20000, 4, 1)
  assert crafter_amd.BatchedEnv._check_nearby(nc.CLASSES, nc.N_MATERIALS, (600, 64), 20000, 4, 0)[0] == 4   # the counts alone: any world
  with pytest.raises(ValueError):
    crafter_amd.BatchedEnv._check_nearby(['none'] + [f'm{i}' for i in range(31)], 25, (64, 64), 256)
  assert crafter_amd.nearby_host is state.nearby_host
  for kw in (dict(k=33), dict(classes=1 << 6), dict(distance=-1, numpy_slices=True)):
    with pytest.raises(ValueError):
      state.nearby_host(dict(mat=np.ones((4, 4), np.uint8), objects=[(1, 0, 0, 9, 0, 1, 0)], sleeping=False), nc.N_MATERIALS, **kw)


# ------------------------------------------------------------------ 5. the stand-alone program
def _in_range(rows, hs, k):
  cells, slots = hs.cfg.W * hs.cfg.H, hs.cfg.max_objects
  for row in rows:
    if row is None:
      continue
    counts, n, ents = row
    assert 0 <= counts[0] <= cells and all(0 <= v <= counts[0] for v in counts[1: nc.N_MATERIALS + 1]) and sum(counts[1: nc.N_MATERIALS + 1]) <= counts[0]
    assert all(0 <= v < slots for v in counts[nc.N_MATERIALS + 1:]) and 0 <= n <= sum(counts[nc.N_MATERIALS + 1:])
    for j, r in enumerate(ents):
      if j >= min(n, k):
        assert r == [0] * 6
      else:
        assert nc.N_MATERIALS + 1 <= r[0] < nc.N_CLASSES and abs(r[1]) < hs.cfg.W and abs(r[2]) < hs.cfg.H and 0 <= r[4] <= 5


@pytest.mark.parametrize('geo', ['64x64', '42x30', '144x144', '256x256'])
def test_body_sanitized_standalone(geo, tmp_path):
  """The body as a stand-alone program under -fsanitize=address,undefined, every buffer of exactly its size: a dumped env after 20
  steps (a row mask; both window rules; on 144 x 144 both object walks), then rows of uniformly random bytes -- one never reset,
  one with counts in range so that every pass runs its full length on garbage.  It exits clean, every output is in range, and
  the rows are the ones the body loaded into Python computes."""
  from tests.hostsim import nearby_build as nb
  hs = _hostsim([41, 42, 43], **GEOS[geo])
  rs = np.random.RandomState(5)
  for t in range(20):
    hs.step(rs.randint(0, 17, size=3).astype(np.int32))
  mask = np.array([1, 0, 1], np.uint8)
  queries = [(5, 16, False, -1), (None, 32, False, -1), (2, 4, True, -1), (70, 0, True, -1)] + ([(9, 16, False, 0), (9, 16, False, 1)] if geo == '144x144' else [])
  for d, k, rule, walk in queries:
    nb.dump(hs, tmp_path / 'env.blob', d, k, nc.ALL_OBJECTS, rule, mask=mask, walk=walk)
    rows = nb.run_sanitized(tmp_path / 'env.blob', nc.N_CLASSES, k)
    c, e, n = nb.nearby(hs, d, k, nc.ALL_OBJECTS, rule, walk=walk)
    assert rows[1] is None and len(rows) == 3
    for i in (0, 2):
      assert rows[i] == (c[i].tolist(), int(n[i]) if k else 0, e[i].tolist()), (geo, d, k, i)
    _in_range(rows, hs, k)
  buf = {name: hs.buf[name].copy() for name in nb.BUFFERS}
  for name in buf:
    raw = buf[name].view(np.uint8)
    raw[...] = rs.randint(0, 256, size=raw.shape, dtype=np.uint8)
  rec = state.rec_view(buf['rec'])
  objs = state.objs_view(buf['objs'])
  rec['episode'] = [0, 7, -3]
  rec['nobj'][2] = hs.cfg.max_objects - 1
  objs[1, 1]['x'], objs[1, 1]['y'] = 3, 2            # (a player inside the world: the passes run)
  objs[2, 1]['x'], objs[2, 1]['y'] = hs.cfg.W - 1, hs.cfg.H - 2
  objs[2, 2:]['x'] %= hs.cfg.W                        # ... and records that pass the bounds, on cells that collide
  objs[2, 2:]['y'] %= hs.cfg.H
  objs[2, 2:]['type'] %= 8
  for d, k, rule, walk in [(None, 32, False, -1), (3, 32, True, -1), (40, 7, False, 1), (300, 32, True, 0), (1 << 30, 1, False, -1)]:
    nb.dump(hs, tmp_path / 'random.blob', d, k, nc.ALL_OBJECTS, rule, walk=walk, buf=buf)
    rows = nb.run_sanitized(tmp_path / 'random.blob', nc.N_CLASSES, k)
    assert rows[0] == ([0] * nc.N_CLASSES, 0, [[0] * 6] * k)
    c, e, n = nb.nearby(hs, d, k, nc.ALL_OBJECTS, rule, walk=walk, buf=buf)
    assert [r[0] for r in rows] == c.tolist() and [r[1] for r in rows] == n.tolist()
    assert c[2, nc.N_MATERIALS + 1:].sum() > 0 or d == 3
    for row in rows:   # counts in range; the rows may repeat a cell (colliding records), never a class outside the classes
      counts, total, ents = row
      assert 0 <= counts[0] <= hs.cfg.W * hs.cfg.H and all(0 <= v <= counts[0] for v in counts[1: nc.N_MATERIALS + 1])
      assert all(0 <= v < hs.cfg.max_objects for v in counts[nc.N_MATERIALS + 1:]) and 0 <= total <= sum(counts[nc.N_MATERIALS + 1:])
      assert all(r == [0] * 6 or nc.N_MATERIALS + 1 <= r[0] < nc.N_CLASSES for r in ents)


# ------------------------------------------------------------------ 6. the library
def test_entry_point_header_and_constants(tmp_path):
  """crafter_nearby is declared in a header of its own, listed in lib.EXTENSIONS and build.sources(), exported by the library; the
  header is pedantic C99 by itself and its constants are the Python ones."""
  from crafter_amd import build, lib as hiplib
  assert 'crafter_nearby' not in (ROOT / 'include' / 'crafter_hip.h').read_text() and 'crafter_nearby' not in hiplib.SIGNATURES
  assert ROOT / 'include' / 'crafter_hip_nearby.h' in build.sources() and ROOT / 'crafter_amd' / 'csrc' / 'nearby.hpp' in build.sources()
  assert len(build.UNITS) == 5
  header = (ROOT / 'include' / 'crafter_hip_nearby.h').read_text()
  assert re.search(r'\bint crafter_nearby\(crafter_handle\* h, const uint8_t\* mask, int32_t distance, int32_t flags, uint32_t classes, int32_t k,\s+'
                   r'int32_t\* counts, int16_t\* ents, int32_t\* n, void\* stream\);', header)
  where, restype, argtypes = hiplib.EXTENSIONS['crafter_nearby']
  vp, i32, u32 = hiplib.vp, hiplib.i32, hiplib.C.c_uint32
  assert where == 'crafter_hip_nearby.h' and restype is i32 and list(argtypes) == [vp, vp, i32, i32, u32, i32, vp, vp, vp, vp]
  nm = subprocess.run(['nm', '-D', '--defined-only', str(build.build())], capture_output=True, text=True, check=True).stdout
  assert 'crafter_nearby' in set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  so = hiplib.load()
  assert so.crafter_nearby.restype is i32 and so.crafter_abi_version() == 7
  if not shutil.which('gcc'):
    pytest.skip('needs gcc')
  names = ['CLIP', 'NUMPY', 'MAX_ENTS', 'ROW', 'MAX_SIDE']
  assert set(re.findall(r'\bCRAFTER_NEARBY_([A-Z_]+)\b', header)) == set(names)
  src = tmp_path / 'nearby.c'
  src.write_text('#include <stdio.h>\n#include "crafter_hip_nearby.h"\nint main(void) {\n' +
                 ''.join(f'  printf("{n} %ld\\n", (long)CRAFTER_NEARBY_{n});\n' for n in names) + '  return 0;\n}\n')
  subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', f'-I{ROOT / "include"}', str(src), '-o', str(tmp_path / 'nearby')], check=True)
  out = subprocess.run([str(tmp_path / 'nearby')], capture_output=True, text=True, check=True).stdout
  assert {k: int(v) for k, v in (line.split() for line in out.splitlines())} == {n: getattr(abi, f'NEARBY_{n}') for n in names}
  assert crafter_amd.NEARBY_MAX_ENTS == 32 and len(abi.NEARBY_COLUMNS) == abi.NEARBY_ROW == 6 and crafter_amd.NEARBY_NUMPY == 1


def test_nearby_kernel_budget():
  """Both instances (one wave or 256 threads), each with objmap state or not: no scratch, no spilled register, and registers for
  eight waves per SIMD -- the bar the read-only siblings set."""
  from crafter_amd import build
  usage = {k: v for k, v in build.resource_usage().items() if k.startswith('crafter_nearby_kernel')}
  assert sorted(usage) == ['crafter_nearby_kernel<256,0>', 'crafter_nearby_kernel<256,1>', 'crafter_nearby_kernel<64,0>', 'crafter_nearby_kernel<64,1>']
  for name, u in usage.items():
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0 and u.get('sgpr_spill', 0) == 0, (name, u)
    assert u['vgprs'] <= 64 and u['occupancy'] >= 8, (name, u)
