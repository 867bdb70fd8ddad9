"""The symbolic observation, the parts that need no GPU: the oracle's restatement (tests/symbolic_ref.py) against the
reference fixture (tools/make_symbolic_golden.py), what the fixture covers, crafter_symbolic's body on the CPU
(tests/hostsim/symbolic_host.cpp) against the restatement, the new entry point and the kernel's resource budget."""
import functools
import pathlib
import re
import subprocess

import numpy as np
import pytest

from crafter_amd import state
from tests import symbolic_ref as sr

ROOT = pathlib.Path(__file__).resolve().parent.parent
FIXTURE = ROOT / 'tests' / 'golden' / 'reference_runs' / 'symbolic_ref.npz'
GENERIC = dict(view=(7, 9), size=(84, 72), area=(32, 32))


@functools.lru_cache(None)
def oracle_trace(case):
  return sr.oracle_trace(case)


@functools.lru_cache(None)
def fixture():
  return np.load(FIXTURE)


def assert_pair(got, want, what):
  (gl, gs), (wl, ws) = got, want
  assert gl.dtype == np.uint8 and gs.dtype == np.float32 and gl.shape == wl.shape and gs.shape == ws.shape, what
  assert np.array_equal(gl, wl), f'{what}: local differs at {np.argwhere(gl != wl)[:4].tolist()}'
  assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), f'{what}: stats {gs} != {ws}'


@pytest.mark.parametrize('case', list(sr.CASES))
def test_restatement_equals_reference(case):
  gold = fixture()
  _, seed, steps, area, poke = sr.CASES[case]
  assert list(gold[f'{case}/meta']) == [seed, steps, area[0], area[1]] + list(poke)
  local, stats = oracle_trace(case)
  want_local, want_stats = gold[f'{case}/local'], gold[f'{case}/stats']
  assert local.shape == want_local.shape == (steps + 1, 2, 9, 7) and stats.shape == want_stats.shape == (steps + 1, 20)
  for t in range(steps + 1):
    assert_pair((local[t], stats[t]), (want_local[t], want_stats[t]), f'{case} row {t}')


def _pairs(local):
  return {(int(i), int(v)) for i, v in zip(local[:, 0].ravel(), local[:, 1].ravel())}


def test_fixture_covers_what_it_is_there_for():
  gold = fixture()
  classes, columns = sr.names(__import__('crafter_amd.tables', fromlist=['x']).load_rules())
  player, skeleton, arrow, plant = (classes.index(n) for n in ('player', 'skeleton', 'arrow', 'plant'))
  assert (player, skeleton, arrow, plant) == (13, 16, 17, 18)
  sleeper = _pairs(gold['sleeper/local'])
  assert {(player, v) for v in (1, 2, 3, 4, 5)} <= sleeper and {(arrow, v) for v in (1, 2, 3, 4)} <= sleeper
  stats = gold['sleeper/stats']
  assert set(stats[:, columns.index('sleeping')].tolist()) == {0.0, 1.0}
  assert stats[:, columns.index('daylight')].min() < 0.5 < stats[:, columns.index('daylight')].max()   # into the night
  fighter = gold['fighter/local']
  outside = sum(1 for t in range(1, fighter.shape[0]) if (fighter[t, 0] == 0).any())
  assert outside >= 100, outside
  assert (fighter[:, 0] == skeleton).any() and (fighter[:, 0] == arrow).any()
  assert (plant, 1) in _pairs(gold['planter/local']) and (plant, 0) in _pairs(gold['planter/local'])


# ------------------------------------------------------------------ the body on the CPU
def _hostsim(seeds, **kw):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv(seeds, render_obs=False, **kw)
  hs.reset()
  return hs


def _run_case_on_hostsim(case, **geo):
  from tests.hostsim import symbolic_build as sb
  acts, gifts, seed, area, poke = sr.tape(case)
  hs = _hostsim([seed], **{**dict(area=area), **geo})
  items = list(hs.rules_dict['items'])
  got = [sb.symbolic(hs)]
  for t, a in enumerate(acts):
    for item, amount in gifts.get(t, {}).items():
      hs.rec['inv'][0][items.index(item)] = amount
    if t in poke:
      sr.poke_objs(state.objs_view(hs.buf['objs'])[0], hs.rec['nobj'][0])
    hs.step(np.array([a], np.int32))
    got.append(sb.symbolic(hs))
  return hs, got


@pytest.mark.parametrize('case', list(sr.CASES))
def test_body_equals_restatement(case):
  from tests.hostsim import symbolic_build as sb
  hs, got = _run_case_on_hostsim(case)
  assert not sb.map_is_state(hs)
  local, stats = oracle_trace(case)
  assert len(got) == local.shape[0]
  for t, (l, s) in enumerate(got):
    assert_pair((l[0], s[0]), (local[t], stats[t]), f'{case} row {t}')


def test_body_generic_geometry():
  """view (7, 9) on an 84 x 72 frame: a 7 x 6 window (three inventory rows)."""
  hs, got = _run_case_on_hostsim('fighter', **GENERIC)
  local, stats = sr.oracle_trace('fighter', **GENERIC)
  assert local.shape[1:] == (2, 7, 6) and len(got) == 201
  for t, (l, s) in enumerate(got):
    assert_pair((l[0], s[0]), (local[t], stats[t]), f'generic row {t}')


def test_body_objmap_path():
  """area (256, 256): the maps stay in global memory, objmap is state and the body reads it instead of the slot table."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import symbolic_build as sb
  hs = _hostsim([3], area=(256, 256))
  assert sb.map_is_state(hs)
  orc = OracleEnv(area=(256, 256), seed=3)
  orc.reset()
  l, s = sb.symbolic(hs)
  assert_pair((l[0], s[0]), sr.symbolic_of(orc), 'after reset')
  seen = set()
  for t, a in enumerate(np.random.RandomState(3).randint(0, 17, size=40)):
    hs.step(np.array([a], np.int32))
    orc.step(int(a))
    l, s = sb.symbolic(hs)
    assert_pair((l[0], s[0]), sr.symbolic_of(orc), f'step {t}')
    seen |= set(np.unique(l[0, 0]).tolist())
  assert 13 in seen and len(seen) > 3


def test_body_rows_tail_mask_and_alignment():
  """Five envs (rows of 126 bytes: every other one starts in the middle of a dword) written into buffers that start at each
  of the four byte phases; masked rows and the bytes around the rows stay as they were."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import symbolic_build as sb
  seeds = [11, 12, 13, 11, 12]
  hs = _hostsim(seeds)
  orcs = {s: OracleEnv(seed=s) for s in set(seeds)}
  for o in orcs.values():
    o.reset()
  acts = np.random.RandomState(5).randint(0, 17, size=(6, 3))
  for t in range(6):
    hs.step(np.array([acts[t, s - 11] for s in seeds], np.int32))
    for s, o in orcs.items():
      o.step(int(acts[t, s - 11]))
  want = {s: sr.symbolic_of(o) for s, o in orcs.items()}
  n, row = len(seeds), 2 * 9 * 7
  for phase in range(4):
    raw = np.full(phase + n * row + 8, 0xFF, np.uint8)
    raw_stats = np.full(n * 20 + 4, np.float32(-7))
    local, stats = raw[phase: phase + n * row].reshape(n, 2, 9, 7), raw_stats[2: 2 + n * 20].reshape(n, 20)
    mask = np.array([1, 0, 1, 1, 1], np.uint8)
    sb.symbolic(hs, mask=mask, out=(local, stats))
    for i, s in enumerate(seeds):
      if mask[i]:
        assert_pair((local[i], stats[i]), want[s], f'phase {phase} env {i}')
      else:
        assert (local[i] == 0xFF).all() and (stats[i] == -7).all()
    assert (raw[:phase] == 0xFF).all() and (raw[phase + n * row:] == 0xFF).all()
    assert (raw_stats[:2] == -7).all() and (raw_stats[2 + n * 20:] == -7).all()
    only_stats = np.zeros((n, 20), np.float32)
    sb.symbolic(hs, out=(None, only_stats))
    assert np.array_equal(only_stats[0], want[seeds[0]][1])


# ------------------------------------------------------------------ the library
def test_entry_point_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_symbolic\(crafter_handle\* h, const uint8_t\* mask, uint8_t\* local, float\* stats, void\* stream\);', header)
  assert 'crafter_symbolic' in hiplib.EXPORTS and 'crafter_symbolic' in exported
  so = hiplib.load()
  assert len(so.crafter_symbolic.argtypes) == 5
  assert so.crafter_abi_version() == 7


def test_symbolic_kernel_budget():
  """No scratch, no spill, eight waves per SIMD -- like the copy kernels, a handful of registers."""
  from crafter_amd import build
  usage = {k: v for k, v in build.resource_usage().items() if k.startswith('crafter_symbolic_kernel')}
  assert len(usage) == 2, sorted(usage)   # MAP 0 (slot table scan) and MAP 1 (objmap)
  for name, u in usage.items():
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, (name, u)
    assert u['occupancy'] >= 8, (name, u)
