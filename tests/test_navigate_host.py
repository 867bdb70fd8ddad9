"""Navigation queries, the parts that need no GPU: crafter_navigate's bodies on the CPU (tests/hostsim/navigate_host.cpp) against
the Python mirror (crafter_amd.navigate_host) on generated and authored worlds, the definition against the reference's rules on
oracle envs, the harness's mask / tail / argument checks, the sanitised stand-alone program, the new entry point, its constant
and the kernels' resource budget, and BatchedEnv._check_targets without a device."""
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import crafter_amd
from crafter_amd import abi, state
from tests import navigate_cases as nc

ROOT = pathlib.Path(__file__).resolve().parent.parent
GEOS = {'64x64': dict(area=(64, 64)), '42x30': dict(area=(42, 30), view=(7, 9), size=(84, 72)), '48x40': dict(area=(48, 40)),
        '144x144': dict(area=(144, 144)), '256x256': dict(area=(256, 256))}
SEEDS = {'64x64': [5, 6, 7, 8, 9, 10], '42x30': [5, 6, 7, 8], '48x40': [5, 6, 7, 8], '144x144': [5, 6, 7, 8], '256x256': [5, 6, 7, 8]}
WALK = nc.class_set(nc.WALKABLE)


def _hostsim(seeds, **kw):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv(seeds, render_obs=False, **kw)
  hs.reset()
  return hs


def _mirror(hs, targets, passable=WALK, rows=None):
  rows = range(hs.cfg.num_envs) if rows is None else rows
  got = [state.navigate_host(hs.snapshot(i), nc.N_MATERIALS, targets, passable, nc.MOVES) for i in rows]
  return tuple(np.array([g[j] for g in got]).astype(dt) for j, dt in enumerate((np.int32, np.int32, np.uint8)))


def _assert_equal(got, want, what):
  for name, g, w in zip(('dist', 'first', 'facing'), got, want):
    bad = np.argwhere(g != w)
    assert not len(bad), f'{what}: {name} differs at (env, target) {bad[:6].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}'


def _authored(geo):
  """A HostSimEnv reset into the authored cases of tests/navigate_cases.py, one env each -> (hs, cases)."""
  from tests.hostsim import worlds_build as wb
  W, H = GEOS[geo]['area']
  cases = nc.cases(W, H)
  hs = _hostsim([0] * len(cases), **GEOS[geo])
  bank = crafter_amd.WorldBank(dict(area=(W, H)), np.stack([c['mat'] for c in cases]), [c['objects'] for c in cases])
  assert wb.reset_worlds(hs, bank, world_ids=np.arange(len(cases))) == 0
  assert not hs.rec['status'].any()
  return hs, cases


# ------------------------------------------------------------------ 1. the bodies against the mirror, generated worlds
@pytest.mark.parametrize('geo', list(GEOS))
def test_body_equals_mirror(geo):
  """K = 16 and K = 1 after reset and after 30 random steps, every env.  The areas above 64 cells a side go through the LDS
  instance; their slot map is state, so the library reads objmap, and 144 x 144 is also walked through the slot table (what an area
  like 80 x 72 takes on that instance: test_authored_worlds_lds_instance).  The compared (env, target) pairs hold a -1, a walk of more
  than 20 steps and a faced target."""
  from tests.hostsim import navigate_build as nb
  hs = _hostsim(SEEDS[geo], **GEOS[geo])
  assert nb.in_registers(hs) == (geo in ('64x64', '42x30', '48x40'))
  assert nb.map_is_state(hs) == (geo in ('144x144', '256x256'))
  acts = np.random.RandomState(17).randint(0, 17, size=(30, len(SEEDS[geo]))).astype(np.int32)
  t16, t1 = nc.sets(nc.TARGETS16), nc.sets(['tree'])
  seen = []
  for t in range(31):
    if t in (0, 30):
      got = nb.navigate(hs, t16, WALK)
      _assert_equal(got, _mirror(hs, t16), f'step {t}, K = 16')
      _assert_equal(nb.navigate(hs, t1, WALK), tuple(a[:, 5:6] for a in got), f'step {t}, K = 1')
      assert (got[0][:, nc.TARGETS16.index('player')] == -1).all()
      if geo == '144x144':
        _assert_equal(nb.navigate(hs, t16, WALK, force_map=0), got, f'step {t}, slot table')
      seen.append(got)
    if t < 30:
      hs.step(acts[t])
  dist = np.concatenate([g[0] for g in seen])
  facing = np.concatenate([g[2] for g in seen])
  assert (dist == -1).any() and (dist > 20).any() and (facing == 1).any() and (dist != 0).all()
  assert ((dist == -1) == (np.concatenate([g[1] for g in seen]) == -1)).all()


def test_register_body_objmap_path():
  """The register instance that reads objmap (a world of at most 64 x 64 cells whose slot map is state): objmap written here from
  the slot table, with a hole and a stale record behind nobj, gives what the slot-table path gives."""
  from tests.hostsim import navigate_build as nb
  hs = _hostsim([31, 32, 33], **GEOS['48x40'])
  for t in range(10):
    hs.step(np.array([2, 4, 1], np.int32))
  cfg = hs.cfg
  objs = state.objs_view(hs.buf['objs'])
  objmap = hs.buf['objmap'].reshape(cfg.num_envs, cfg.W, cfg.H)
  objmap[:] = 0
  for i in range(cfg.num_envs):
    for s in range(1, int(hs.rec['nobj'][i])):
      if objs[i, s]['type'] != abi.T_NONE:
        objmap[i, objs[i, s]['x'], objs[i, s]['y']] = s
  t16 = nc.sets(nc.TARGETS16)
  _assert_equal(nb.navigate(hs, t16, WALK, force_map=1), nb.navigate(hs, t16, WALK, force_map=0), 'objmap path')
  _assert_equal(nb.navigate(hs, t16, WALK, force_map=1), _mirror(hs, t16), 'objmap path, mirror')


# ------------------------------------------------------------------ 2. authored worlds
@pytest.mark.parametrize('geo', ['64x64', '42x30'])
def test_authored_worlds(geo):
  """The cases of tests/navigate_cases.py: the literal values, and the mirror."""
  from tests.hostsim import navigate_build as nb
  hs, cases = _authored(geo)
  for i, c in enumerate(cases):
    mask = np.zeros(len(cases), np.uint8)
    mask[i] = 1
    targets = nc.sets(c['targets'])
    passable = WALK if c['passable'] is None else nc.class_set(c['passable'])
    got = tuple(a[i].tolist() for a in nb.navigate(hs, targets, passable, mask=mask))
    assert list(zip(*got)) == [tuple(e) for e in c['expect']], c['name']
    want = state.navigate_host(hs.snapshot(i), nc.N_MATERIALS, targets, passable, nc.MOVES)
    assert got == tuple(np.asarray(w).astype(int).tolist() for w in want), c['name']
  assert cases[0]['expect'][0][0] == {'64x64': 2078, '42x30': 649}[geo]   # the serpentine: every lane and bit boundary is crossed


@pytest.mark.parametrize('area', [(144, 144), (80, 72)], ids=['144x144', '80x72'])
def test_authored_worlds_lds_instance(area):
  """The border cases (e) and the serpentine on the LDS instance: nothing is carried from a column's last word into the next
  column's first, nor beyond row H - 1 of a last word that is not full (H = 72)."""
  from tests.hostsim import navigate_build as nb
  from tests.hostsim import worlds_build as wb
  W, H = area
  cases = [c for c in nc.cases(W, H) if c['name'][0] in 'ae']
  hs = _hostsim([0] * len(cases), area=area)
  assert not nb.in_registers(hs) and nb.map_is_state(hs) == (area == (144, 144))
  bank = crafter_amd.WorldBank(dict(area=area), np.stack([c['mat'] for c in cases]), [c['objects'] for c in cases])
  assert wb.reset_worlds(hs, bank, world_ids=np.arange(len(cases))) == 0
  targets = nc.sets(['tree', 'coal', 'table'])
  dist, first, facing = nb.navigate(hs, targets, WALK)
  for i, c in enumerate(cases):
    for name, e in zip(c['targets'], c['expect']):
      k = ['tree', 'coal', 'table'].index(name)
      assert (dist[i, k], first[i, k], facing[i, k]) == tuple(e), (c['name'], name)
  _assert_equal((dist, first, facing), _mirror(hs, targets), 'mirror')


# ------------------------------------------------------------------ 3. the definition against the reference's rules
@pytest.mark.parametrize('seed', [3, 11])
def test_definition_agrees_with_the_oracle(seed):
  """A walker on an oracle env that follows `first` of the mirror towards one target after the other: where dist > 1 the move
  puts the player exactly onto the predicted neighbour; where dist == 1 (a material target) the cell in front is then a target."""
  from oracle.crafter_oracle import OracleEnv
  orc = OracleEnv(seed=seed, area=(64, 64), length=10000)
  orc.reset()
  names = ['tree', 'water', 'stone', 'cow', ['coal', 'iron'], 'table']
  targets = nc.sets(names)
  steps = dict(zip(nc.MOVES, ((-1, 0), (1, 0), (0, -1), (0, 1))))
  moved = faced = 0
  goal = 0
  for t in range(160):
    snap = orc.snapshot()
    dist, first, facing = state.navigate_host(snap, nc.N_MATERIALS, targets, WALK, nc.MOVES)
    tp, px, py, _, fx, fy, _ = snap['objects'][0]
    assert tp == abi.T_PLAYER
    for _ in range(len(names)):
      if dist[goal] > 0 and not (dist[goal] == 1 and (facing[goal] or names[goal] == 'cow')):
        break
      goal = (goal + 1) % len(names)
    else:
      break
    d, a = int(dist[goal]), int(first[goal])
    if snap['sleeping']:
      break
    if orc.step(a)[2]:
      break
    after = orc.snapshot()
    _, qx, qy, _, gx, gy, _ = after['objects'][0]
    if d > 1:
      assert (qx, qy) == (px + steps[a][0], py + steps[a][1]), (t, names[goal], d)
      moved += 1
    else:
      assert (qx, qy) == (px, py) and (gx, gy) == steps[a]
      assert targets[goal] >> int(after['mat'][qx + gx, qy + gy]) & 1 and not after['occupied'][qx + gx, qy + gy], (t, names[goal])
      faced += 1
      goal = (goal + 1) % len(names)
  assert moved >= 20 and faced >= 2, (moved, faced)


# ------------------------------------------------------------------ 4. mask, tail, arguments
def test_body_rows_tail_mask_and_arguments():
  """Five envs (four to a workgroup) with a row mask, written into sentinel-filled buffers inside larger ones: masked rows and
  the words around [N][k] stay as they were; what crafter_navigate refuses is refused with a message that names the argument."""
  from tests.hostsim import navigate_build as nb
  hs = _hostsim([11, 12, 13, 14, 15], **GEOS['64x64'])
  hs.step(np.array([1, 2, 3, 4, 5], np.int32))
  targets = np.array(nc.sets(['tree', 'water', 'cow']), np.uint32)
  full = nb.navigate(hs, targets.tolist(), WALK)
  raw = [np.full(5 * 3 + 8, 0x5E, dt) for dt in (np.int32, np.int32, np.uint8)]
  out = [r[4:19].reshape(5, 3) for r in raw]
  mask = np.array([1, 0, 0, 1, 0], np.uint8)
  assert nb.call(hs, targets, 3, WALK, mask, *out) == 0
  for i in range(5):
    for o, f in zip(out, full):
      assert (o[i] == (f[i] if mask[i] else 0x5E)).all()
  for r in raw:
    assert (r[:4] == 0x5E).all() and (r[19:] == 0x5E).all()
  facing = out[2].copy()
  assert nb.call(hs, targets, 3, WALK, mask, out[0], out[1], None) == 0 and (out[2] == facing).all()   # facing may be null
  classes = len(nc.CLASSES)
  refused = [((targets, 0), 'k'), ((targets, 17), 'k'), ((None, 3), 'targets'), ((np.array([0, 2, 4], np.uint32), 3), 'targets'),
             ((np.array([2, 3, 4], np.uint32), 3), 'targets'), ((np.array([2, 1 << classes, 4], np.uint32), 3), 'targets')]
  for (tg, k), word in refused:
    rc = nb.call(hs, tg, k, WALK, None, *out)
    assert rc != 0 and word in nb.error_text(rc), (k, word, nb.error_text(rc))
  for passable in (WALK | 1, WALK | 1 << (nc.N_MATERIALS + 1)):
    rc = nb.call(hs, targets, 3, passable, None, *out)
    assert rc != 0 and 'passable' in nb.error_text(rc)
  for o in ((None, out[1], out[2]), (out[0], None, out[2])):
    rc = nb.call(hs, targets, 3, WALK, None, *o)
    assert rc != 0 and 'dist or first' in nb.error_text(rc)
  big = np.full(17, 4, np.uint32)
  assert nb.call(hs, big, 16, WALK, None, np.zeros((5, 16), np.int32), np.zeros((5, 16), np.int32), None) == 0
  for i in range(5):   # nothing of the refused calls was written
    for o, f in zip(out, full):
      assert (o[i] == (f[i] if mask[i] else 0x5E)).all()


# ------------------------------------------------------------------ 5. the stand-alone program
def test_body_sanitized_standalone(tmp_path):
  """The bodies as a stand-alone program under -fsanitize=address,undefined, every buffer of exactly its size: generated worlds
  of the register instance (both column loads) and of the LDS instance (both object paths) after 20 steps, one with a row mask,
  and the authored worlds.  Same rows."""
  from tests.hostsim import navigate_build as nb
  rs = np.random.RandomState(5)
  t16 = nc.sets(nc.TARGETS16)
  for geo, mask, targets in (('64x64', None, t16), ('42x30', np.array([1, 0, 1], np.uint8), t16), ('144x144', None, t16[:6]),
                             ('256x256', np.array([0, 1, 1], np.uint8), t16[5:12])):
    hs = _hostsim([41, 42, 43], **GEOS[geo])
    for t in range(20):
      hs.step(rs.randint(0, 17, size=3).astype(np.int32))
    nb.dump(hs, tmp_path / f'{geo}.blob', targets, WALK, mask=mask)
    rows = nb.run_sanitized(tmp_path / f'{geo}.blob')
    want = nb.navigate(hs, targets, WALK)
    assert len(rows) == 3
    for i, row in enumerate(rows):
      if mask is not None and not mask[i]:
        assert row is None, geo
      else:
        assert row == tuple(w[i].tolist() for w in want), (geo, i)
  hs, cases = _authored('42x30')
  targets = nc.sets(['table', 'tree', 'coal', 'cow', 'sand', 'water', 'diamond'])
  nb.dump(hs, tmp_path / 'authored.blob', targets, WALK)
  want = nb.navigate(hs, targets, WALK)
  assert nb.run_sanitized(tmp_path / 'authored.blob') == [tuple(w[i].tolist() for w in want) for i in range(len(cases))]


# ------------------------------------------------------------------ 6. the library
def test_entry_point_header_and_constant(tmp_path):
  """crafter_navigate is declared in a header of its own, listed in lib.EXTENSIONS and build.sources(), exported by the library;
  the header is pedantic C99 by itself and CRAFTER_NAV_MAX_TARGETS is the Python constant."""
  from crafter_amd import build, lib as hiplib
  assert 'crafter_navigate' not in (ROOT / 'include' / 'crafter_hip.h').read_text() and 'crafter_navigate' not in hiplib.SIGNATURES
  assert ROOT / 'include' / 'crafter_hip_navigate.h' in build.sources() and len(build.UNITS) == 5
  where, restype, argtypes = hiplib.EXTENSIONS['crafter_navigate']
  assert where == 'crafter_hip_navigate.h' and len(argtypes) == 9 and argtypes[3] is hiplib.C.c_int32 and argtypes[4] is hiplib.C.c_uint32
  nm = subprocess.run(['nm', '-D', '--defined-only', str(build.build())], capture_output=True, text=True, check=True).stdout
  assert 'crafter_navigate' in set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert hiplib.load().crafter_abi_version() == 7
  if not shutil.which('gcc'):
    pytest.skip('needs gcc')
  src = tmp_path / 'nav.c'
  src.write_text('#include <stdio.h>\n#include "crafter_hip_navigate.h"\nint main(void) {\n'
                 '  printf("%ld\\n", (long)CRAFTER_NAV_MAX_TARGETS);\n  return 0;\n}\n')
  subprocess.run(['gcc', '-std=c99', '-pedantic', '-Wall', '-Werror', f'-I{ROOT / "include"}', str(src), '-o', str(tmp_path / 'nav')], check=True)
  out = subprocess.run([str(tmp_path / 'nav')], capture_output=True, text=True, check=True).stdout
  assert int(out) == crafter_amd.NAV_MAX_TARGETS == abi.NAV_MAX_TARGETS == 16


def test_navigate_kernel_budget():
  """Both register instances: no scratch, no spill, eight waves per SIMD -- the bar test_legal_kernel_budget and
  test_fingerprint_kernel_budget set.  The LDS instance: no scratch."""
  from crafter_amd import build
  usage = build.resource_usage()
  reg = {k: v for k, v in usage.items() if k.startswith('crafter_navigate_kernel')}
  assert sorted(reg) == ['crafter_navigate_kernel<0>', 'crafter_navigate_kernel<1>'], sorted(reg)
  for name, u in reg.items():
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, (name, u)
    assert u['occupancy'] >= 8 and u['vgprs'] <= 64, (name, u)
  lds = {k: v for k, v in usage.items() if k.startswith('crafter_navigate_lds_kernel')}
  assert len(lds) == 2, sorted(lds)
  for name, u in lds.items():
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, (name, u)


# ------------------------------------------------------------------ 7. the Python checks, without a device
def test_check_targets_without_a_device():
  check = lambda targets, passable=None: crafter_amd.BatchedEnv._check_targets(nc.CLASSES, nc.N_MATERIALS, nc.WALKABLE, targets, passable)
  sets, walk = check(['tree', 6, ['coal', 'iron', 10], 'cow', [14, 'zombie'], np.int64(1)])
  assert sets == [1 << 6, 1 << 6, 1 << 8 | 1 << 9 | 1 << 10, 1 << 14, 1 << 14 | 1 << 15, 2]
  assert walk == WALK == (1 << 2 | 1 << 4 | 1 << 5)
  assert check(['tree'], ['grass', 'lava'])[1] == (1 << 2 | 1 << 7) and check(['tree'], [2, 5])[1] == (1 << 2 | 1 << 5)
  assert len(check(['tree'] * 16)[0]) == 16 and check(nc.TARGETS16)[0] == nc.sets(nc.TARGETS16)
  bad = [[], ['tree'] * 17, ['wood'], ['none'], [0], [19], [-1], [[]], [1.5], [True], 'tree', 6, [['tree', 'nothing']], None]
  for targets in bad:
    with pytest.raises(ValueError):
      check(targets)
  for passable in (['cow'], ['none'], [0], [13], [], 'player'):
    with pytest.raises(ValueError):
      check(['tree'], passable)
  with pytest.raises(ValueError):
    crafter_amd.BatchedEnv._check_targets(['none'] + [f'm{i}' for i in range(31)], 25, ['m0'], ['m1'])


def test_mirror_is_exported():
  assert crafter_amd.navigate_host is state.navigate_host
