"""crafter_step_envs without a GPU: the launch rule's choice of the subset kernel, the index check's body and the subset kernel's
body (csrc/crafter_subset.hpp) through the CPU harness (tests/hostsim/subset_host.cpp) -- stepping a batch in two complementary
halves leaves what stepping it at once leaves, a refused list changes nothing --, the entry point's declaration and export, and
the register budgets of the new kernels."""
import ctypes as C
import copy
import itertools
import pathlib
import re
import subprocess

import numpy as np
import pytest

from crafter_amd import abi, tables

ROOT = pathlib.Path(__file__).resolve().parent.parent

RULES = tables.load_rules()
OTHER_RULES = copy.deepcopy(RULES)
OTHER_RULES['items']['health'] = {'max': 5, 'initial': 5}
# name: (rules, make_config arguments, instance) -- one per entry of CRAFTER_STEP_INSTANCES (csrc/launch_plan.hpp)
INSTANCES = {
    '111': (RULES, {}, 7),
    '110': (OTHER_RULES, {}, 6),
    '100': (RULES, dict(area=(32, 32)), 4),
    '021': (RULES, dict(area=(256, 256)), 9),
    '000': (RULES, dict(area=(256, 256), view=(7, 9), size=(84, 72)), 0),
}


# ------------------------------------------------------------------ kernel choice
@pytest.mark.parametrize('name', list(INSTANCES))
def test_choose_step_envs(name):
  """The wide kernel for instance 7 when frames are drawn and the call names at most 512 envs (CRAFTER_STEP_WIDE overriding),
  the fused instance otherwise: no split pair, no early-frame kernel."""
  from tests.hostsim import subset_build as sb
  rules, kw, instance = INSTANCES[name]
  default_rules = rules is RULES
  for n, frames, wide in itertools.product((1, 512, 513, 4096), (False, True), (-1, 0, 1)):
    cfg, _ = tables.make_config(4096, rules, **kw)
    kernel, inst = sb.choose(cfg, default_rules, n, frames, wide)
    assert inst == instance
    want = instance == 7 and frames and (wide == 1 or (wide == -1 and n <= 512))
    assert kernel == int(want), (name, n, frames, wide)


# ------------------------------------------------------------------ the bodies
N, LENGTH, CALLS = 12, 20, 60
# the queues hold what is left of earlier calls behind their counts, in the order the envs were dispatched: no state of an env
QUEUES = ('reset_q', 'gen_q')


def _hostsim(pool):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv([31 * i + 5 for i in range(N)], auto_reset=True, length=LENGTH, pool=pool)
  hs.reset()
  return hs


def _assert_equal(a, b, where):
  for name in a.buf:
    if name not in QUEUES:
      assert np.array_equal(a.buf[name], b.buf[name]), (where, name)
  assert np.array_equal(a.obs, b.obs) and np.array_equal(a.reward, b.reward) and np.array_equal(a.done, b.done), where


@pytest.mark.parametrize('pool', [False, True], ids=['inline', 'pool'])
def test_two_halves_equal_one_step(pool):
  """step_body is driven by an env index and by nothing else of the launch: two subset calls over random complementary halves
  leave every state buffer, obs, reward and done as HostSimEnv.step of all envs leaves them, call after call, auto-resets
  (from the pool or inline) included."""
  from tests.hostsim import subset_build as sb
  a, b = _hostsim(pool), _hostsim(pool)
  marks = sb.Marks(N)
  rs = np.random.RandomState(7)
  for t in range(CALLS):
    acts = rs.randint(0, 17, N).astype(np.int32)
    perm = rs.permutation(N)
    k = int(rs.randint(1, N))
    a.step(acts)
    for half in (perm[:k], perm[k:]):
      assert sb.step_envs(b, marks, half, acts[half]) == 0
    _assert_equal(a, b, t)
  assert a.rec['episode'].min() >= 3 and not a.rec['status'].any()
  if pool:
    assert a.buf['pool_stats'][0] > 0 and np.array_equal(a.buf['pool_stats'], b.buf['pool_stats'])


@pytest.mark.parametrize('idx, flagged', [([3, 7, 3], [3, 7]), ([2, N, 5], [2, 5]), ([N, -1], [0])],
                         ids=['duplicate', 'out-of-range', 'none-exists'])
def test_refused_lists_change_nothing(idx, flagged):
  """An env named twice or an entry out of range refuses the whole call: no byte changes but ST_BAD_COPY in the status of the
  named rows that exist (row 0 if none does)."""
  from tests.hostsim import subset_build as sb
  hs = _hostsim(True)
  marks = sb.Marks(N)
  assert sb.step_envs(hs, marks, np.arange(N), np.full(N, 5)) == 0   # a good call first: its marks must not count against the next
  before = {k: v.copy() for k, v in hs.buf.items()}
  out = hs.obs.copy(), hs.reward.copy(), hs.done.copy()
  assert sb.step_envs(hs, marks, idx, np.full(len(idx), 5)) == 1
  status = hs.rec['status'].copy()
  assert [i for i in range(N) if status[i] & abi.ST_BAD_COPY] == flagged and not (status & ~np.uint32(abi.ST_BAD_COPY)).any()
  hs.rec['status'] = 0
  for k, v in before.items():
    assert np.array_equal(hs.buf[k], v), k
  assert np.array_equal(hs.obs, out[0]) and np.array_equal(hs.reward, out[1]) and np.array_equal(hs.done, out[2])
  assert sb.step_envs(hs, marks, [3, 7], [5, 5]) == 0   # and the handle steps on
  assert hs.rec['step'][3] == before['rec'].view(abi.REC_DTYPE)['step'][3, 0] + 1


def test_host_side_refusals():
  from tests.hostsim import subset_build as sb
  hs = _hostsim(False)
  marks = sb.Marks(N)
  before = hs.buf['rec'].copy()
  assert sb.step_envs(hs, marks, np.zeros(0, np.int32), np.zeros(0, np.int32)) == 0   # n == 0: nothing happens
  assert sb.step_envs(hs, marks, np.arange(N + 1) % N, np.zeros(N + 1)) == -1         # n > num_envs
  assert np.array_equal(hs.buf['rec'], before)


# ------------------------------------------------------------------ the library
def test_entry_point_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_step_envs\(crafter_handle\* h, const int32_t\* idx, int32_t n, const int32_t\* actions,\s*'
                   r'uint8_t\* obs, float\* reward, uint8_t\* done, void\* stream\);', header)
  assert 'crafter_step_envs' in hiplib.EXPORTS and 'crafter_step_envs' in exported
  so = hiplib.load()
  assert len(so.crafter_step_envs.argtypes) == 8
  assert so.crafter_abi_version() == 7
  text = abi.STATUS_NAMES[abi.ST_BAD_COPY]
  assert abi.ST_BAD_COPY == 64 and 'ST_BAD_COPY' in text and 'step_envs' in text
  assert 'crafter_subset.hip' in {p.name for p in build.sources()}


def test_subset_kernels_keep_their_twins_register_budgets():
  """Each subset kernel is its twin's body behind one more load: no scratch, no spilled VGPR, and the waves per SIMD
  tests/test_host_logic.py asks of crafter_step_kernel<...> / crafter_step_wide_kernel.  The check kernel is a few loops."""
  from crafter_amd import build
  usage = build.resource_usage()
  budget = {'crafter_step_subset_kernel<1,1,1>': 6, 'crafter_step_subset_kernel<1,1,0>': 6, 'crafter_step_subset_kernel<1,0,0>': 5,
            'crafter_step_subset_kernel<0,0,0>': 6, 'crafter_step_subset_kernel<0,2,1>': 6, 'crafter_step_subset_wide_kernel': 6}
  for k, occ in budget.items():
    assert k in usage, (k, sorted(usage))
    assert usage[k]['scratch'] == 0 and usage[k]['vgpr_spill'] == 0, (k, usage[k])
    assert usage[k]['occupancy'] >= occ, (k, usage[k])
  check = usage['crafter_step_envs_check_kernel']
  assert check['vgprs'] <= 32 and check['scratch'] == 0 and check['vgpr_spill'] == 0, check
