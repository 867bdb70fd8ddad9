"""The legal-action mask, the parts that need no GPU: the oracle's restatement (tests/legal_ref.py) against the reference fixture
(tools/make_legal_golden.py), what the fixture covers, crafter_legal_actions' body on the CPU (tests/hostsim/legal_host.cpp)
against the restatement, the new entry point and the kernel's resource budget."""
import copy
import functools
import pathlib
import re
import subprocess

import numpy as np
import pytest

from crafter_amd import state, tables
from tests import legal_ref as lr
from tests import symbolic_ref as sr

ROOT = pathlib.Path(__file__).resolve().parent.parent
FIXTURE = ROOT / 'tests' / 'golden' / 'reference_runs' / 'legal_ref.npz'
GENERIC = dict(view=(7, 9), size=(84, 72), area=(32, 32))
ACTIONS = list(tables.load_rules()['actions'])
MOVES = [a for a, n in enumerate(ACTIONS) if n.startswith('move_')]
MAKES = [a for a, n in enumerate(ACTIONS) if n.startswith('make_')]
DO = ACTIONS.index('do')
COW, ZOMBIE, SKELETON, ARROW, PLANT = 2, 3, 4, 5, 6


@functools.lru_cache(None)
def oracle_trace(case):
  return lr.oracle_trace(case)


@functools.lru_cache(None)
def fixture():
  return np.load(FIXTURE)


def assert_rows(got, want, what):
  assert got.dtype == np.uint8 and got.shape == want.shape, what
  bad = np.argwhere(got != want)
  assert not len(bad), f'{what}: differs at (row, action) {bad[:4].tolist()}: {got[bad[0][0]].tolist()} != {want[bad[0][0]].tolist()}'


@pytest.mark.parametrize('case', list(lr.CASES))
def test_restatement_equals_reference(case):
  gold = fixture()
  _, seed, steps, area, poke = lr.CASES[case]
  assert list(gold[f'{case}/meta']) == [seed, steps, area[0], area[1]] + list(poke)
  assert gold[f'{case}/legal'].shape == (steps + 1, len(ACTIONS))
  assert_rows(oracle_trace(case), gold[f'{case}/legal'], case)


def test_restatement_equals_reference_on_the_edge_states():
  gold = fixture()
  assert list(gold['edge/meta']) == [lr.EDGE_SEED, 12] + list(lr.EDGE_AREA)
  assert_rows(lr.edge_trace(), gold['edge/legal'], 'edge states')


def test_fixture_covers_what_it_is_there_for():
  gold = fixture()
  legal = np.concatenate([gold[f'{c}/legal'] for c in lr.CASES])
  target = np.concatenate([gold[f'{c}/target'] for c in lr.CASES])   # class on target, ripe, sleeping, energy < max
  assert (legal[:, 0] == 1).all()
  for a, name in enumerate(ACTIONS):
    assert (legal[:, a] == 1).any(), name
    assert name == 'noop' or (legal[:, a] == 0).any(), name
  asleep = (target[:, 2] == 1) & (target[:, 3] == 1)
  assert asleep.sum() >= 10 and (legal[asleep, 1:] == 0).all() and (legal[asleep, 0] == 1).all()
  ripe, unripe, arrow = (target[:, 0] == PLANT) & (target[:, 1] == 1), (target[:, 0] == PLANT) & (target[:, 1] == 0), target[:, 0] == ARROW
  awake = ~asleep
  assert (ripe & awake).any() and (legal[ripe & awake, DO] == 1).all()
  assert unripe.any() and (legal[unripe, DO] == 0).all()
  assert arrow.any() and (legal[arrow, DO] == 0).all()
  creature = np.isin(target[:, 0], (COW, ZOMBIE, SKELETON))
  assert (creature & awake).any() and (legal[creature & awake, DO] == 1).all()
  # the edge states: numpy's slices make the window empty at x == 0 or y == 0 although a table is adjacent, and clip it at the
  # far edges; nothing can be done towards the outside
  edge = gold['edge/legal']
  for row, e in zip(edge, lr.edge_states()):
    x, y = e['pos']
    assert (row[MAKES] == (0 if x == 0 or y == 0 else 1)).all(), (e, row.tolist())
    if e['outward']:
      move = ACTIONS.index('move_' + {v: k for k, v in lr.DIRS.items()}[e['facing']])
      assert row[move] == 0 and row[DO] == 0 and not any(row[a] for a, n in enumerate(ACTIONS) if n.startswith('place_')), (e, row.tolist())
  assert any(r[DO] == 1 for r, e in zip(edge, lr.edge_states()) if not e['outward'])


def test_fixture_behaviour():
  """What the mask means, from what the reference did (deep copies stepped with each action and with noop)."""
  gold = fixture()
  legal_nonmove = same = 0
  for case in lr.CASES:
    legal, behaviour, target = gold[f'{case}/legal'], gold[f'{case}/behaviour'], gold[f'{case}/target']
    assert (legal[:, MOVES] == behaviour[:, MOVES]).all(), case
    others = [a for a in range(1, len(ACTIONS)) if a not in MOVES]
    assert not ((legal[:, others] == 0) & (behaviour[:, others] == 1)).any(), case
    inert = (legal[:, others] == 1) & (behaviour[:, others] == 0)
    creature = np.isin(target[:, 0], (COW, ZOMBIE, SKELETON))
    assert not inert[:, [i for i, a in enumerate(others) if a != DO]].any() and not inert[~creature].any(), case
    legal_nonmove += int((legal[:, others] == 1).sum())
    same += int(inert.sum())
  assert same <= 0.01 * legal_nonmove, (same, legal_nonmove)


# ------------------------------------------------------------------ the body on the CPU
def _hostsim(seeds, **kw):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv(seeds, render_obs=False, **kw)
  hs.reset()
  return hs


def _run_case_on_hostsim(case, actions=None, **kw):
  from tests.hostsim import legal_build as lb
  acts, gifts, seed, area, poke = lr.tape(case)
  hs = _hostsim([seed], **{**dict(area=area), **kw})
  items = list(hs.rules_dict['items'])
  got = [lb.legal(hs)[0]]
  for t, a in enumerate(acts if actions is None else actions):
    for item, amount in gifts.get(t, {}).items():
      hs.rec['inv'][0][items.index(item)] = amount
    if t in poke:
      sr.poke_objs(state.objs_view(hs.buf['objs'])[0], hs.rec['nobj'][0])
    hs.step(np.array([a], np.int32))
    got.append(lb.legal(hs)[0])
  return hs, np.stack(got)


@pytest.mark.parametrize('case', list(lr.CASES))
def test_body_equals_restatement(case):
  from tests.hostsim import legal_build as lb
  hs, got = _run_case_on_hostsim(case)
  assert not lb.map_is_state(hs)
  assert_rows(got, oracle_trace(case), case)


def _edge_hostsim(edge, **kw):
  hs = _hostsim([lr.EDGE_SEED], area=lr.EDGE_AREA, **kw)
  W, H = lr.EDGE_AREA
  lr.edge_arrays(edge, hs.rules_dict, hs.buf['mat'][0].reshape(W, H), state.objs_view(hs.buf['objs'])[0], hs.rec['inv'][0])
  return hs


def test_body_on_the_edge_states():
  from tests.hostsim import legal_build as lb
  got = np.stack([lb.legal(_edge_hostsim(e))[0] for e in lr.edge_states()])
  assert_rows(got, lr.edge_trace(), 'edge states')


def test_body_generic_geometry():
  """view (7, 9) on an 84 x 72 frame over a 32 x 32 world: the generic step instance's states."""
  hs, got = _run_case_on_hostsim('builder', **GENERIC)
  assert_rows(got, lr.oracle_trace('builder', **GENERIC), 'generic')


def test_body_objmap_path():
  """area (256, 256): the maps stay in global memory, objmap is state and the body reads it instead of the slot table."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import legal_build as lb
  hs = _hostsim([3], area=(256, 256))
  assert lb.map_is_state(hs)
  orc = OracleEnv(area=(256, 256), seed=3)
  orc.reset()
  assert_rows(lb.legal(hs)[0], lr.legal_of(orc), 'after reset')
  for t, a in enumerate(np.random.RandomState(3).randint(0, 17, size=40)):
    hs.step(np.array([a], np.int32))
    orc.step(int(a))
    assert_rows(lb.legal(hs)[0], lr.legal_of(orc), f'step {t}')


def test_body_objmap_path_on_the_border():
  """The objmap path with the player on the border of a 256 x 256 world: poked states (the poke moves the player's slot id in
  objmap too), observed only -- the same env and the same oracle poked from one state to the next."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import legal_build as lb
  area = (256, 256)
  hs = _hostsim([3], area=area)
  assert lb.map_is_state(hs)
  orc = OracleEnv(area=area, seed=3)
  orc.reset()
  makes_seen = set()
  for k, e in enumerate(lr.edge_states(area, ((0, 5), (5, 0), (0, 0), (255, 5), (5, 255), (255, 255)))):
    lr.poke_edge_oracle(orc, e)
    lr.edge_arrays(e, hs.rules_dict, hs.buf['mat'][0].reshape(area), state.objs_view(hs.buf['objs'])[0], hs.rec['inv'][0],
                   objmap=hs.buf['objmap'][0].reshape(area))
    want = lr.legal_of(orc)
    assert_rows(lb.legal(hs)[0], want, f'border state {k}')
    assert (want[MAKES] == (0 if 0 in e['pos'] else 1)).all(), (e, want.tolist())
    makes_seen.add(int(want[MAKES][0]))
    if e['outward']:
      assert want[DO] == 0 and want[ACTIONS.index('move_' + {v: n for n, v in lr.DIRS.items()}[e['facing']])] == 0
  assert makes_seen == {0, 1}


def test_body_rows_tail_mask_and_alignment():
  """Five envs with a row mask, written into a buffer pre-filled with 0xFF at an odd byte offset (rows of 17 bytes): masked
  rows and the bytes around the buffer stay as they were."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import legal_build as lb
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
  want = {s: lr.legal_of(o) for s, o in orcs.items()}
  n, na = len(seeds), len(ACTIONS)
  raw = np.full(3 + n * na + 8, 0xFF, np.uint8)
  out = raw[3: 3 + n * na].reshape(n, na)
  mask = np.array([1, 0, 1, 1, 1], np.uint8)
  lb.legal(hs, mask=mask, out=out)
  for i, s in enumerate(seeds):
    if mask[i]:
      assert_rows(out[i], want[s], f'env {i}')
    else:
      assert (out[i] == 0xFF).all()
  assert (raw[:3] == 0xFF).all() and (raw[3 + n * na:] == 0xFF).all()


EDITED = ('make_wood_sword', 'make_wood_pickaxe', 'place_stone', 'do')   # the actions whose rule custom_rules() edits


def custom_rules():
  """A rule set on which a compiled-in shortcut would show: the actions in another order, a second `nearby` material for two
  make rules, another `where` for one place rule and a `require` for one collect rule."""
  rules = copy.deepcopy(tables.load_rules())
  rules['actions'] = list(reversed(rules['actions']))
  rules['make']['wood_sword']['nearby'] = ['table', 'tree']
  rules['make']['wood_pickaxe']['nearby'] = ['table', 'furnace']
  rules['place']['stone']['where'] = ['tree', 'sand', 'path', 'water', 'lava']   # grass out, tree in
  rules['collect']['grass']['require'] = {'stone_pickaxe': 2}
  return rules


def test_body_custom_rules():
  """The body against the restatement under custom_rules(); and, state by state, the restatement under the default tables on the
  SAME state: each edited rule must change its action's bit somewhere, so a shortcut through any one compiled-in table shows."""
  from oracle.crafter_oracle import Tables
  rules = custom_rules()
  acts, _, _, _, _ = lr.tape('builder')
  names = tables.load_rules()['actions']
  remapped = [rules['actions'].index(names[a]) for a in acts[:300]]   # the same tape, by name
  hs, got = _run_case_on_hostsim('builder', actions=remapped, rules=rules)
  orc, _, gifts, _ = lr.oracle_run('builder', rules=rules)
  custom, default = orc.t, Tables(tables.load_rules())

  def both():
    orc.t = default
    d = lr.legal_of(orc)
    orc.t = custom
    return lr.legal_of(orc), d
  rows = [both()]
  for t, a in enumerate(remapped):
    if t in gifts:
      sr.gift_oracle(orc, gifts[t])
    orc.step(int(a))
    rows.append(both())
  want, under_default = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
  assert_rows(got, want, 'custom rules')
  for name in names:
    differs = int((want[:, rules['actions'].index(name)] != under_default[:, names.index(name)]).sum())
    assert (differs > 0) == (name in EDITED), (name, differs)
    if name in EDITED:   # ... and the edited rule is seen both ways
      assert set(want[:, rules['actions'].index(name)].tolist()) == {0, 1}, name


def test_body_sanitized_standalone(tmp_path):
  """The body as a stand-alone program under -fsanitize=address,undefined, every buffer of exactly its size: the builder tape's
  state after 150 steps on the slot-table path, a 256 x 256 world on the objmap path, border states and a row mask."""
  from tests.hostsim import legal_build as lb
  hs, got = _run_case_on_hostsim('builder', actions=lr.tape('builder')[0][:150])
  lb.dump(hs, tmp_path / 'builder.blob')
  assert_rows(lb.run_sanitized(tmp_path / 'builder.blob'), got[-1:], 'builder')
  big = _hostsim([3, 4], area=(256, 256))
  big.step(np.array([5, 2], np.int32))
  lb.dump(big, tmp_path / 'big.blob', mask=np.array([0, 1], np.uint8))
  rows = lb.run_sanitized(tmp_path / 'big.blob')
  assert (rows[0] == 0xFF).all()
  assert_rows(rows[1:], lb.legal(big)[1:], 'objmap path')
  for k, e in enumerate(lr.edge_states()):
    hs = _edge_hostsim(e)
    lb.dump(hs, tmp_path / 'edge.blob')
    assert_rows(lb.run_sanitized(tmp_path / 'edge.blob'), lb.legal(hs), f'edge {k}')


# ------------------------------------------------------------------ the library
def test_entry_point_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_legal_actions\(crafter_handle\* h, const uint8_t\* mask, uint8_t\* legal, void\* stream\);', header)
  assert 'crafter_legal_actions' in hiplib.EXPORTS and 'crafter_legal_actions' in exported
  so = hiplib.load()
  assert len(so.crafter_legal_actions.argtypes) == 4
  assert so.crafter_abi_version() == 7


def test_legal_kernel_budget():
  """No scratch, no spill, eight waves per SIMD: the bar test_symbolic_kernel_budget sets for its sibling."""
  from crafter_amd import build
  usage = {k: v for k, v in build.resource_usage().items() if k.startswith('crafter_legal_actions_kernel')}
  assert len(usage) == 2, sorted(usage)   # MAP 0 (slot table scan) and MAP 1 (objmap)
  for name, u in usage.items():
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, (name, u)
    assert u['occupancy'] >= 8, (name, u)
    assert u['vgprs'] <= 16, (name, u)   # (8: the env's facts are wave-uniform and live in scalar registers)
