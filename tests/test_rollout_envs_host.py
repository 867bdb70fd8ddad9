"""crafter_step_n_envs without a GPU: the index check's body, the rollout body and the regeneration body
(csrc/crafter_rollout_subset.hpp) through the CPU harness (tests/hostsim/rollout_envs_host.cpp) -- rolling a batch out in two
complementary halves with compact outputs leaves what rolling it out at once leaves, a refused list changes nothing --, the
entry point's declaration and export, and the register budgets of the new kernels."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

from crafter_amd import abi

ROOT = pathlib.Path(__file__).resolve().parent.parent

N, LENGTH, CALLS = 12, 20, 20
STEPS = (1, 3, 16, 37)
SENTINEL = 0xA5
# the queues hold what is left of earlier calls behind their counts, in the order the envs were dispatched: no state of an env
QUEUES = ('reset_q', 'gen_q')


def _hostsim(pool):
  from tests.hostsim.driver import HostSimEnv
  hs = HostSimEnv([31 * i + 5 for i in range(N)], auto_reset=True, length=LENGTH, pool=pool)
  hs.reset()
  return hs


@pytest.mark.parametrize('pool', [False, True], ids=['inline', 'pool'])
def test_two_halves_equal_one_rollout(pool):
  """rollout_envs_body is rollout_body but for where a step's outputs go: two subset rollouts over random complementary halves
  leave every state buffer as HostSimEnv.step_n of all envs leaves it, and their compact rows are the full rollout's columns,
  call after call, auto-resets (from the pool, inline in the rollout's own regeneration body, twice in a stretch) included."""
  from tests.hostsim import rollout_envs_build as rb
  a, b = _hostsim(pool), _hostsim(pool)
  marks = rb.Marks(N)
  rs = np.random.RandomState(11)
  seen = set()
  for call in range(CALLS):
    T = STEPS[call] if call < len(STEPS) else int(rs.choice(STEPS))
    seen.add(T)
    acts = rs.randint(0, 17, (T, N)).astype(np.int32)
    perm = rs.permutation(N)
    k = int(rs.randint(1, N))
    obs, reward, done = a.step_n(acts)
    for half in (perm[:k], perm[k:]):
      verdict, o, r, d = rb.rollout_envs(b, marks, half, acts[:, half])
      assert verdict == 0
      assert np.array_equal(o, obs[:, half]), (call, T)
      assert np.array_equal(r, reward[:, half]) and np.array_equal(d, done[:, half]), (call, T)
    for name in a.buf:
      if name not in QUEUES:
        assert np.array_equal(a.buf[name], b.buf[name]), (call, T, name)
  assert seen == set(STEPS)
  assert a.rec['episode'].min() >= 3 and not a.rec['status'].any()
  if pool:
    assert a.buf['pool_stats'][0] > 0 and np.array_equal(a.buf['pool_stats'], b.buf['pool_stats'])


def test_one_step_rollout_equals_step_envs():
  """T == 1 is crafter_step_envs but for the compact rows."""
  from tests.hostsim import rollout_envs_build as rb, subset_build as sb
  a, b = _hostsim(True), _hostsim(True)
  ma, mb = sb.Marks(N), rb.Marks(N)
  rs = np.random.RandomState(3)
  for call in range(30):
    idx = rs.permutation(N)[:int(rs.randint(1, N + 1))]
    acts = rs.randint(0, 17, idx.size).astype(np.int32)
    assert sb.step_envs(a, ma, idx, acts) == 0
    verdict, o, r, d = rb.rollout_envs(b, mb, idx, acts[None])
    assert verdict == 0
    assert np.array_equal(o[0], a.obs[idx]) and np.array_equal(r[0], a.reward[idx]) and np.array_equal(d[0], a.done[idx]), call
    for name in a.buf:
      if name not in QUEUES:
        assert np.array_equal(a.buf[name], b.buf[name]), (call, name)
  assert a.rec['episode'].max() >= 1


@pytest.mark.parametrize('idx, flagged', [([3, 7, 3], [3, 7]), ([2, N, 5], [2, 5]), ([N, -1], [0])],
                         ids=['duplicate', 'out-of-range', 'none-exists'])
def test_refused_lists_change_nothing(idx, flagged):
  """An env named twice or an entry out of range refuses the whole call: no byte of the state changes but ST_BAD_COPY in the
  status of the named rows that exist (row 0 if none does), and no byte of the outputs."""
  from tests.hostsim import rollout_envs_build as rb
  hs = _hostsim(True)
  marks = rb.Marks(N)
  T = 5
  assert rb.rollout_envs(hs, marks, np.arange(N), np.full((T, N), 5))[0] == 0   # a good call first: its marks must not count against the next
  before = {k: v.copy() for k, v in hs.buf.items()}
  n = len(idx)
  out = (np.full((T, n) + hs.obs.shape[1:], SENTINEL, np.uint8), np.full((T, n), -7.5, np.float32), np.full((T, n), SENTINEL, np.uint8))
  assert rb.rollout_envs(hs, marks, idx, np.full((T, n), 5), out=out)[0] == 1
  status = hs.rec['status'].copy()
  assert [i for i in range(N) if status[i] & abi.ST_BAD_COPY] == flagged and not (status & ~np.uint32(abi.ST_BAD_COPY)).any()
  hs.rec['status'] = 0
  for k, v in before.items():
    assert np.array_equal(hs.buf[k], v), k
  assert (out[0] == SENTINEL).all() and (out[1] == np.float32(-7.5)).all() and (out[2] == SENTINEL).all()
  assert rb.rollout_envs(hs, marks, [7, 3], np.full((T, 2), 5))[0] == 0   # and the handle steps on
  rec_before = before['rec'].view(abi.REC_DTYPE)
  for env in (3, 7):   # (length 20: the five steps may cross an episode's end)
    same_episode = hs.rec['episode'][env] == rec_before['episode'][env, 0]
    assert hs.rec['step'][env] == rec_before['step'][env, 0] + T if same_episode else hs.rec['episode'][env] == rec_before['episode'][env, 0] + 1


def test_host_side_refusals():
  from tests.hostsim import rollout_envs_build as rb
  hs = _hostsim(False)
  marks = rb.Marks(N)
  before = hs.buf['rec'].copy()
  assert rb.rollout_envs(hs, marks, np.zeros(0, np.int32), np.zeros((2, 0), np.int32))[0] == 0   # n == 0: nothing happens
  assert rb.rollout_envs(hs, marks, np.arange(N + 1) % N, np.zeros((2, N + 1)))[0] == -1          # n > num_envs
  assert np.array_equal(hs.buf['rec'], before)


# ------------------------------------------------------------------ the library
def test_entry_point_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_step_n_envs\(crafter_handle\* h, const int32_t\* idx, int32_t n, int32_t steps, const int32_t\* actions,\s*'
                   r'uint8_t\* obs, float\* reward, uint8_t\* done, void\* stream\);', header)
  assert 'crafter_step_n_envs' in hiplib.EXPORTS and 'crafter_step_n_envs' in exported
  so = hiplib.load()
  assert len(so.crafter_step_n_envs.argtypes) == 9
  assert so.crafter_abi_version() == 7
  assert 'crafter_rollout_subset.hip' in {p.name for p in build.sources()}


def test_subset_rollout_kernels_keep_their_twins_register_budgets():
  """Each subset rollout instance is its twin's loop behind one more load: no scratch, no spilled VGPR, and the waves per SIMD
  tests/test_host_logic.py asks of crafter_rollout_kernel<...>.  The regeneration kernel is bounded as its twin is (it may
  spill: it all but always finds its queue empty); the check kernel is a few loops."""
  from crafter_amd import build
  usage = build.resource_usage()
  budget = {'crafter_rollout_subset_kernel<1,1,1>': 6, 'crafter_rollout_subset_kernel<1,1,0>': 6, 'crafter_rollout_subset_kernel<1,0,0>': 3,
            'crafter_rollout_subset_kernel<0,0,0>': 4, 'crafter_rollout_subset_kernel<0,2,1>': 6}
  for k, occ in budget.items():
    assert k in usage, (k, sorted(usage))
    assert usage[k]['scratch'] == 0 and usage[k]['vgpr_spill'] == 0, (k, usage[k])
    assert usage[k]['occupancy'] >= occ, (k, usage[k])
  assert usage['crafter_requeue_rollout_subset_kernel']['occupancy'] >= 4, usage['crafter_requeue_rollout_subset_kernel']
  check = usage['crafter_rollout_envs_check_kernel']
  assert check['vgprs'] <= 32 and check['scratch'] == 0 and check['vgpr_spill'] == 0, check
