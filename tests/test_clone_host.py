"""Copies of environments, the parts that need no GPU: the reference's deepcopy / pickle pinned on the oracle, the new C entry
points and status bit, the store layout and the copy kernels' resource budget."""
import copy
import ctypes
import pathlib
import pickle
import re
import subprocess

import numpy as np

from tests import reference_runs as rr

ROOT = pathlib.Path(__file__).resolve().parent.parent
FIXTURE = ROOT / 'tests' / 'golden' / 'reference_runs' / 'deepcopy.npz'
NEW_ENTRY_POINTS = ('crafter_copy_envs', 'crafter_save_envs', 'crafter_load_envs')


def _make_oracle(seed, length):
  from oracle.crafter_oracle import OracleEnv
  return OracleEnv(seed=seed, length=length), rr.OracleSide


def _replay(copier):
  import importlib.util
  spec = importlib.util.spec_from_file_location('make_clone_runs', ROOT / 'tools' / 'make_clone_runs.py')
  mk = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mk)
  gold = np.load(FIXTURE)
  checked = 0
  for name, seed, length, k, steps in mk.CASES:
    assert list(gold[f'{name}/meta']) == [seed, length, k, steps]
    keys = ['original', 'copy'] + (['pickle'] if copier is not copy.deepcopy else [])
    if copier is not copy.deepcopy and f'{name}/pickle' not in gold.files:
      continue
    orig, twin = mk.run(_make_oracle, copier, seed, length, k, steps)
    for key, got in zip(keys, (orig, twin, twin)):
      want = gold[f'{name}/{key}']
      assert got.shape == want.shape, (name, key, got.shape, want.shape)
      bad = np.nonzero((got != want).any(axis=1))[0]
      assert not bad.size, f'{name}/{key}: first difference in row {bad[0]} ({rr.KINDS[int(want[bad[0], 0])]})'
      checked += 1
  assert checked


def test_oracle_deepcopy_matches_reference():
  """copy.deepcopy of the reference Env at a step by day and one at night: the original and the copy, stepped with different
  tapes through an episode end and a render(512x512), live the same futures on the oracle as on the reference."""
  _replay(copy.deepcopy)


def test_oracle_pickle_matches_reference():
  _replay(lambda env: pickle.loads(pickle.dumps(env)))


def test_new_entry_points_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  for name in NEW_ENTRY_POINTS:
    assert re.search(rf'\bint {name}\(', header), name
    assert name in hiplib.EXPORTS, name
    assert name in exported, name
  so = hiplib.load()
  for name in NEW_ENTRY_POINTS:
    assert getattr(so, name).argtypes, name
  assert so.crafter_abi_version() == 7


def test_bad_copy_status_bit_consistent():
  """The seven status bits of abi.py are distinct, each has its text, and each is the C header's value of that name."""
  from crafter_amd import abi
  from tests import abi_layout
  assert abi.ST_BAD_COPY == 64 and 'ST_BAD_COPY' in abi.STATUS_NAMES[abi.ST_BAD_COPY]
  bits = {name: value for name, value in abi_layout.python_values().items() if name.startswith('ST_')}
  assert len(bits) == 7 and len(set(bits.values())) == 7 and set(bits.values()) == set(abi.STATUS_NAMES)
  header = abi_layout.header_report()[2]
  assert header['ST_BAD_COPY'] == abi.ST_BAD_COPY
  assert {name: header[name] for name in bits} == bits
  assert len({abi.ST_OBJ_OVERFLOW, abi.ST_BAD_ACTION, abi.ST_STEP_OVERFLOW, abi.ST_CHUNK_OVERFLOW, abi.ST_POOL_MISMATCH,
              abi.ST_PIPE_STALL, abi.ST_BAD_COPY}) == 7


def test_store_spec_shapes():
  from crafter_amd import abi, state, tables
  rules = tables.load_rules()
  cfg, _ = tables.make_config(4096, rules)
  spec = state.store_spec(cfg, 5)
  assert set(spec) == {'mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'terminal', 'obs', 'reward', 'done'}
  assert spec['mat'] == ((5, 64 * 64), np.uint8)
  assert spec['objs'] == ((5, cfg.max_objects, 16), np.uint8)
  assert spec['mt'] == ((5, abi.MT_N), np.uint32)
  assert spec['rec'] == ((5, abi.REC_DTYPE.itemsize), np.uint8)
  assert spec['chunk_order'] == ((5, 36), np.uint16) and spec['chunk_seen'] == ((5, 36), np.uint8)
  assert spec['census'] == ((5, 36 * 5), np.int32) and spec['terminal'] == ((5, abi.MAX_ACH + 4), np.int32)
  assert spec['obs'] == ((5, 64, 64, 3), np.uint8) and spec['reward'] == ((5,), np.float32) and spec['done'] == ((5,), np.uint8)
  assert not any(name in spec for name in state.POOL_BUFFERS + ('reset_q',))
  big, _ = tables.make_config(1024, rules, area=(256, 256), want_semantic=True, max_objects=512)
  spec = state.store_spec(big, 3, slot_map_derived=False)
  assert spec['objmap'] == ((3, 256 * 256), np.uint16) and spec['semantic'] == ((3, 256 * 256), np.uint8)
  assert spec['objs'] == ((3, 512, 16), np.uint8)
  assert spec['chunk_order'] == ((3, 22 * 22), np.uint16) and spec['census'] == ((3, 22 * 22 * 5), np.int32)
  # every buffer but the pool's and the queues' has the state's row layout
  full = state.state_spec(big)
  for name, (shape, dt) in spec.items():
    if name in full:
      assert shape[1:] == full[name][0][1:] and dt == full[name][1], name


def test_copy_kernel_budget():
  """The copy kernels hold no scratch and keep eight waves per SIMD (their loops are a handful of registers)."""
  from crafter_amd import build
  usage = build.resource_usage()
  for name in ('crafter_copy_envs_kernel', 'crafter_copy_check_kernel'):
    u = usage[name]
    assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, (name, u)
    assert u['occupancy'] >= 8, (name, u)
