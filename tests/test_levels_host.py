"""Level selection without a GPU: crafter_reseed's declaration and export, its body (csrc/env_levels.hpp) on hand-made arrays and
behind the CPU harness against the oracle, BatchedEnv's host-side argument checks and the kernel's resource usage."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

from crafter_amd import abi, state, tables
from tests.parity import assert_same

ROOT = pathlib.Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------ the library
def test_entry_point_declared_listed_and_exported():
  from crafter_amd import build, lib as hiplib
  header = (ROOT / 'include' / 'crafter_hip.h').read_text()
  path = build.build()
  nm = subprocess.run(['nm', '-D', '--defined-only', str(path)], capture_output=True, text=True, check=True).stdout
  exported = set(re.findall(r'\b(crafter_[a-z_]+)$', nm, re.M))
  assert re.search(r'\bint crafter_reseed\(crafter_handle\* h, const uint8_t\* mask, const uint64_t\* seed_lane,\s*'
                   r'const int32_t\* episode, void\* stream\);', header)
  assert 'additive under abi revision 7: a binding looks it up by name' in header[header.index('Level selection'):].lower()
  assert 'crafter_reseed' in hiplib.EXPORTS and 'crafter_reseed' in exported
  so = hiplib.load()
  assert len(so.crafter_reseed.argtypes) == 5
  assert so.crafter_abi_version() == 7


def test_reseed_kernel_budget():
  """One thread per env and a handful of stores: no scratch, no spilled register."""
  from crafter_amd import build
  u = build.resource_usage()['crafter_reseed_kernel']
  assert u['scratch'] == 0 and u.get('vgpr_spill', 0) == 0, u


# ------------------------------------------------------------------ the body on hand-made arrays
N = 300   # two workgroups of the kernel's 256 threads, the second one partly beyond the batch


def _arrays(seed=1):
  """Config for N envs and rec / pool_hdr / gen_latest full of noise (every byte a reseed must not touch is then visible)."""
  rs = np.random.RandomState(seed)
  cfg, _ = tables.make_config(N, tables.load_rules())
  rec = rs.randint(0, 256, size=(N, abi.REC_DTYPE.itemsize)).astype(np.uint8)
  hdr = rs.randint(0, 256, size=(2, N, abi.POOL_HDR_DTYPE.itemsize)).astype(np.uint8)
  latest = rs.randint(5, 1000, size=N).astype(np.int32)
  lanes = rs.randint(0, 2 ** 63, size=N, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)   # (all 64 bits in use)
  return cfg, rec, hdr, latest, lanes


def _ptrs(rec, hdr=None, latest=None):
  p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p).value
  return abi.StatePtrs(rec=p(rec), pool_hdr=p(hdr), gen_latest=p(latest))


def _check_rows(before, after, named, lanes, want_rec_episode, pool=True):
  rec0, hdr0, latest0 = before
  rec1, hdr1, latest1 = after
  r0, r1 = state.rec_view(rec0), state.rec_view(rec1)
  h0, h1 = hdr0.view(abi.POOL_HDR_DTYPE).reshape(2, N), hdr1.view(abi.POOL_HDR_DTYPE).reshape(2, N)
  assert np.array_equal(r1['seed_lane'][named], lanes[named])
  assert np.array_equal(r1['episode'][named], want_rec_episode[named])
  # every other byte of rec, named rows included
  scrub = lambda r: [r[name] for name in abi.REC_DTYPE.names if name not in ('seed_lane', 'episode')]
  for a, b in zip(scrub(r0), scrub(r1)):
    assert np.array_equal(a, b)
  assert np.array_equal(rec0[~named], rec1[~named])
  if pool:
    assert (h1['ready'][:, named] == 0).all() and (h1['pending'][:, named] == 0).all()
    for name in abi.POOL_HDR_DTYPE.names:
      if name not in ('ready', 'pending'):
        assert np.array_equal(h0[name], h1[name]), name
    assert np.array_equal(hdr0[:, ~named], hdr1[:, ~named])
    assert np.array_equal(latest1[named], want_rec_episode[named]) and np.array_equal(latest1[~named], latest0[~named])
  else:
    assert np.array_equal(hdr0, hdr1) and np.array_equal(latest0, latest1)


def test_reseed_body_on_hand_made_arrays():
  from tests.hostsim import levels_build as lb
  cfg, rec, hdr, latest, lanes = _arrays()
  rs = np.random.RandomState(2)
  mask = (rs.randint(0, 3, size=N) > 0).astype(np.uint8)
  mask[[0, N - 1]] = 1, 0
  mask[mask > 0] = rs.randint(1, 256, size=int((mask > 0).sum()))   # any non-zero byte names a row
  eps = rs.randint(1, 2 ** 31 - 3, size=N).astype(np.int32)
  eps[:8] = [1, 2, 0, -5, 2 ** 31 - 3, 3, -2 ** 31, 7]
  before = rec.copy(), hdr.copy(), latest.copy()
  lb.reseed_raw(cfg, _ptrs(rec, hdr, latest), mask, lanes, eps)
  _check_rows(before, (rec, hdr, latest), mask != 0, lanes, np.maximum(eps, 1) - 1)
  assert (mask[:8] != 0).sum() >= 4

  # mask NULL: all envs; episode NULL: 1
  before = rec.copy(), hdr.copy(), latest.copy()
  lb.reseed_raw(cfg, _ptrs(rec, hdr, latest), None, lanes[::-1].copy(), None)
  _check_rows(before, (rec, hdr, latest), np.ones(N, bool), lanes[::-1], np.zeros(N, np.int32))

  # pool pointers NULL (no auto-reset, pool off): only the record is written
  cfg, rec, hdr, latest, lanes = _arrays(3)
  before = rec.copy(), hdr.copy(), latest.copy()
  lb.reseed_raw(cfg, _ptrs(rec), mask, lanes, eps)
  _check_rows(before, (rec, hdr, latest), mask != 0, lanes, np.maximum(eps, 1) - 1, pool=False)


# ------------------------------------------------------------------ behind the harness, against the oracle
LENGTH = 20


@pytest.mark.parametrize('episode', [1, 3])
@pytest.mark.parametrize('pool', [False, True], ids=['inline', 'pool'])
def test_reseeded_env_plays_the_oracles_level(pool, episode):
  """Envs of seeds [3, 4], ten steps in; env 0 is reseeded to (seed 0, `episode`) and reset under a mask.  From there it is
  OracleEnv(seed=0) from its episode-th reset(), across episode ends; env 1 is what it is in a run without the reseed.
  With the pool on, env 0's entries hold worlds 2 and 3 of seed 3 when it is reseeded: episode 1 then needs the numbers 2 and 3
  again (the stale-entry case), and gen_latest stands at 3 (the pool would never serve the env again)."""
  from oracle.crafter_oracle import OracleEnv
  from tests.hostsim import levels_build as lb
  from tests.hostsim.driver import HostSimEnv
  rs = np.random.RandomState(7)
  pre, post = rs.randint(0, 17, size=(10, 2)), rs.randint(0, 17, size=(40, 2))
  hs = HostSimEnv([3, 4], auto_reset=True, length=LENGTH, pool=pool)
  ctl = HostSimEnv([3, 4], auto_reset=True, length=LENGTH, pool=pool)
  for e in (hs, ctl):
    e.reset()
    for a in pre:
      e.step(a)
  if pool:
    assert sorted(hs.pool_hdr['ready'][:, 0] & 0xFFFFFFFF) == [2, 3] and hs.buf['gen_latest'][0] == 3
  mask = np.array([1, 0], np.uint8)
  lb.reseed(hs, [0, 'never read'], episodes=[episode, -9], mask=mask)
  assert hs.rec['episode'][0] == episode - 1 and hs.rec['step'][0] == 10   # the episode in progress: only its number changed
  hs.reset(mask)
  ctl.reset(mask)
  oracle = OracleEnv(seed=0, length=LENGTH)
  oracle._episode = episode - 1
  obs = oracle.reset()
  assert np.array_equal(hs.obs[0], obs)
  assert_same(hs.snapshot(0), oracle.snapshot(), 'reset')
  ends = 0
  for t, a in enumerate(post):
    hs.step(a)
    ctl.step(a)
    obs, reward, done, _ = oracle.step(int(a[0]))
    if done:
      ends += 1
      obs = oracle.reset()
    assert bool(hs.done[0]) == bool(done) and hs.reward[0] == np.float32(reward), t
    assert np.array_equal(hs.obs[0], obs), t
    assert np.array_equal(hs.obs[1], ctl.obs[1]) and hs.reward[1] == ctl.reward[1] and hs.done[1] == ctl.done[1], t
  assert ends >= 1
  assert_same(hs.snapshot(0), oracle.snapshot(), 'final')
  assert hs.rec['episode'][0] == episode + ends
  for name in ('mat', 'objs', 'mt', 'rec', 'chunk_order', 'chunk_seen', 'census', 'terminal', 'pool_hdr', 'gen_latest'):
    b0, b1 = hs.buf[name], ctl.buf[name]
    if name == 'pool_hdr':
      b0, b1 = b0[:, 1], b1[:, 1]
    else:
      b0, b1 = b0[1], b1[1]
    assert np.array_equal(b0, b1), name
  if pool:   # the pool serves the reseeded env again: every episode end behind the reseed found its world there
    assert hs.buf['pool_stats'][1] == ctl.buf['pool_stats'][1] == 0
    assert hs.buf['gen_latest'][0] == episode + ends + 2


# ------------------------------------------------------------------ BatchedEnv's host-side checks
def test_host_side_argument_checks():
  from crafter_amd.batched import BatchedEnv
  check = BatchedEnv._check_levels
  lanes, eps = check(4, [0, -3, 'a string', (1, 2)], None)
  assert np.array_equal(lanes, state.seed_lanes([0, -3, 'a string', (1, 2)])) and lanes.dtype == np.uint64 and eps is None
  assert check(4, None, 2)[1].tolist() == [2, 2, 2, 2] and check(4, None, 2)[1].dtype == np.int32
  assert check(3, np.array([5, 6, 7]), [1, 2, BatchedEnv.MAX_EPISODE])[1].tolist() == [1, 2, 2 ** 31 - 3]
  for seeds, episodes in (([1, 2, 3], None), ([1, 2, 3, 4, 5], None), ([1, 2, 3, 4], [1, 2, 3]), ([1, 2, 3, 4], 0), ([1, 2, 3, 4], [1, 1, 0, 1]),
                          ([1, 2, 3, 4], -1), ([1, 2, 3, 4], 2 ** 31 - 2), ([1, 2, 3, 4], [1.5, 1, 1, 1]), (None, [[1, 2], [3, 4], [5, 6]])):
    with pytest.raises(ValueError):
      check(4, seeds, episodes)
